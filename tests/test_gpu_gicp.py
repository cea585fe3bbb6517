"""GPU parity of Generalized ICP (gicp.hip through m3d.core.gicp / gicp_terms, m3d.prep and the
matcher drop-in) against the numpy restatement tests/gicp_restatement.py.

Bounds.
* Covariances from normals: |Δ| ≤ 1e-13 per entry — a handful of roundings times the factor
  1 / (1 + c) ≤ 100.
* One evaluation: per slot |gpu − ref| ≤ 1e-11·Σ|term| (Σ|term| = the slot's absolute-value sum of
  the restatement): κ(M) ≤ 1/ε = 1e3 times ≈ 100 u.  tests/test_gicp_cpu.py shows the restatement
  itself sits inside it (float64 against longdouble: 2.6e-14).  Correspondences, the count and
  Σd² 's inputs are the exact NN's; brute force, the grid and repeated calls agree in every bit.
* The loop: correspondences at every evaluation equal the restatement's (its fixtures have no
  near-ties, asserted in tests/test_gicp_cpu.py); iterations, fitness, converged equal; T within
  1e-9 (the project's tolerance for point-to-plane loops, tests/test_gpu_icp.py); inlier_rmse
  within 1e-12.
"""
import numpy as np
import pytest

import clean_restatement as CR
import gicp_restatement as G
import icp_oracle as I
import matcher
import prep_oracle as P
from m3d import prep, synth
from m3d.core import Cloud, gicp, gicp_terms
from m3d.types import PointCloud

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------ covariances from normals
def hand_normals():
    rng = np.random.default_rng(8)
    c = -0.99 + 1e-9
    s = np.sqrt(1 - c * c)
    r = rng.standard_normal((40, 3))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    return np.vstack([[1.0, 0, 0], [-1.0, 0, 0], [c, 0.6 * s, 0.8 * s], [-0.995, np.sqrt(1 - 0.995 ** 2), 0.0],
                      [0, 0, 1.0], [0, -1.0, 0], r])


def test_covariances_from_normals():
    assert prep.covariances_from_normals(np.zeros((0, 3))).shape == (0, 3, 3)
    n = hand_normals()
    for eps in (1e-3, 0.05):
        got = prep.covariances_from_normals(n, eps)
        ref = G.covariances_from_normals(n, eps)
        print("covariances: worst |diff|", np.abs(got - ref).max())
        assert np.abs(got - ref).max() <= 1e-13
        np.testing.assert_array_equal(got, np.swapaxes(got, 1, 2))
    np.testing.assert_array_equal(got[1], np.diag([0.05, 1, 1]))  # −e1: the c < −0.99 branch
    np.testing.assert_array_equal(got[3], np.diag([0.05, 1, 1]))
    with pytest.raises(ValueError):
        prep.covariances_from_normals(n, 0.0)


# ------------------------------------------------------------------------------- one evaluation
def eval_case(ns, nt=777, seed=3):
    src, sn, tgt, tn, T = G.bumpy_pair(ns, nt, seed)
    return src, sn, tgt, tn, T


def eval_ref(src, sn, tgt, tn, T, r):
    cs, ct = G.covariances_from_normals(sn, G.EPS), G.covariances_from_normals(tn, G.EPS)
    pcd = I.initial_points(T, src)
    if not I.is_identity(T):
        cs = G.rotate_covariances(T[:3, :3], cs)
    _, _, corr, _ = I.registration_result(pcd, tgt, r)
    j = np.full(len(src), -1, np.int64)
    j[corr[:, 0]] = corr[:, 1]
    sums, scale = G.gicp_terms(pcd, cs, tgt, ct, corr)
    return sums, scale, j


# 8453 sources = 34 blocks of 256: more block partials than the reduce's 32 groups (a group then
# adds more than one row) — the pass has its own single-block reduce, which takes any row count
@pytest.mark.parametrize("ns", [1, 257, 1000, 8453])
@pytest.mark.parametrize("identity", [False, True])
def test_one_evaluation(ns, identity):
    src, sn, tgt, tn, T = eval_case(ns)
    if identity:
        src, sn, T = synth.apply(T, src), sn @ T[:3, :3].T, np.eye(4)
    ref, scale, j = eval_ref(src, sn, tgt, tn, T, G.RADIUS)
    s, t = Cloud(src, sn), Cloud(tgt, tn)
    out = {}
    for nn in ("brute", "grid"):
        sums, idx = gicp_terms(s, t, T, G.RADIUS, nn=nn)
        out[nn] = (sums, idx.cpu().numpy())
    sums, idx = out["grid"]
    np.testing.assert_array_equal(idx, j)
    if ns > 1:
        assert 0 < (j >= 0).sum() < ns  # the radius leaves some sources unmatched
    assert sums[28] == ref[28] == (j >= 0).sum()
    err = np.abs(sums - ref)
    print(f"ns={ns}: worst |gpu - ref| / sum|term| =", (err[scale > 0] / scale[scale > 0]).max() if (scale > 0).any() else 0.0)
    assert np.all(err <= 1e-11 * scale)
    np.testing.assert_array_equal(out["brute"][0], sums)
    np.testing.assert_array_equal(out["brute"][1], idx)
    again, _ = gicp_terms(s, t, T, G.RADIUS, nn="grid")
    np.testing.assert_array_equal(again, sums)
    # explicit covariances equal to the from-normals ones: the same bits as None
    cs, ct = prep.covariances_from_normals(sn, G.EPS), prep.covariances_from_normals(tn, G.EPS)
    expl, idx2 = gicp_terms(Cloud(src), Cloud(tgt), T, G.RADIUS, src_cov=cs, tgt_cov=ct, nn="grid")
    np.testing.assert_array_equal(expl, sums)
    np.testing.assert_array_equal(idx2.cpu().numpy(), idx)


@pytest.mark.parametrize("nn", ["brute", "grid"])
def test_one_evaluation_without_matches_and_empty_clouds(nn):
    src, sn, tgt, tn, T = eval_case(257)
    s, t = Cloud(src, sn), Cloud(tgt, tn)
    sums, idx = gicp_terms(s, t, T, 1e-6, nn=nn)  # no target that close
    np.testing.assert_array_equal(sums, np.zeros(30))
    np.testing.assert_array_equal(idx.cpu().numpy(), np.full(257, -1))
    e = Cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    sums, idx = gicp_terms(e, t, T, G.RADIUS, nn=nn)
    np.testing.assert_array_equal(sums, np.zeros(30))
    assert len(idx) == 0
    sums, idx = gicp_terms(s, e, T, G.RADIUS, nn=nn)
    np.testing.assert_array_equal(sums, np.zeros(30))
    np.testing.assert_array_equal(idx.cpu().numpy(), np.full(257, -1))


def test_terms_reject_bad_arguments():
    src, sn, tgt, tn, T = eval_case(257)
    s, t = Cloud(src, sn), Cloud(tgt, tn)
    with pytest.raises(ValueError):
        gicp_terms(s, t, T, 0.0)
    with pytest.raises(ValueError):
        gicp_terms(s, t, T, G.RADIUS, epsilon=0.0)
    with pytest.raises(ValueError):
        gicp_terms(s, t, T, G.RADIUS, nn="octree")
    with pytest.raises(ValueError):  # neither covariances nor normals
        gicp_terms(Cloud(src), t, T, G.RADIUS)
    with pytest.raises(ValueError):
        gicp(s, Cloud(tgt), G.RADIUS)


# --------------------------------------------------------------------------------------- the loop
def clouds_of(case):
    return Cloud(case["src"], case["sn"]), Cloud(case["tgt"], case["tn"])


def corr_of(out, ns):
    j = np.full(ns, -1, np.int64)
    j[out.correspondence_set[:, 0]] = out.correspondence_set[:, 1]
    return j


@pytest.mark.parametrize("kind", ["identity", "perturbed"])
def test_loop_matches_restatement(kind):
    case = G.loop_case(kind)
    ref, evals, init = case["ref"], case["evals"], case["init"]
    s, t = clouds_of(case)
    ns = len(case["src"])
    # correspondences at every evaluation: a run stopped after k updates ends on evaluation k
    for k in range(len(evals) - 1):
        out = gicp(s, t, G.LOOP_RADIUS, init, epsilon=G.EPS, max_iteration=k)
        np.testing.assert_array_equal(corr_of(out, ns), evals[k][1], err_msg=f"evaluation {k}")
        assert out.iterations == k and not out.converged
        if k == 0:
            np.testing.assert_array_equal(out.transformation, init)
            assert out.fitness == (evals[0][1] >= 0).mean()
    out = gicp(s, t, G.LOOP_RADIUS, init, epsilon=G.EPS)
    np.testing.assert_array_equal(corr_of(out, ns), evals[-1][1])
    assert (out.iterations, out.fitness, out.converged) == (ref["iterations"], ref["fitness"], ref["converged"])
    print(f"{kind}: |T - ref| {np.abs(out.transformation - ref['transformation']).max():.3e}, "
          f"|rmse - ref| {abs(out.inlier_rmse - ref['inlier_rmse']):.3e}, iterations {out.iterations}")
    np.testing.assert_allclose(out.transformation, ref["transformation"], rtol=0, atol=1e-9)
    assert abs(out.inlier_rmse - ref["inlier_rmse"]) <= 1e-12
    np.testing.assert_array_equal(out.correspondence_set, ref["correspondence_set"])
    # brute force and the grid: the same bits
    b = gicp(s, t, G.LOOP_RADIUS, init, epsilon=G.EPS, nn="brute")
    np.testing.assert_array_equal(b.transformation, out.transformation)
    assert (b.fitness, b.inlier_rmse, b.iterations, b.converged) == (out.fitness, out.inlier_rmse, out.iterations,
                                                                     out.converged)
    np.testing.assert_array_equal(b.correspondence_set, out.correspondence_set)


def test_loop_source_order_does_not_matter():
    """The caller's source order, covariances with it, permuted: the loop gathers both into its
    Morton slots, so T moves by summation rounding only (1e-12) and the correspondence set is the
    same set under the permutation."""
    case = G.loop_case("perturbed")
    ns = len(case["src"])
    t = Cloud(case["tgt"], case["tn"])
    cs = prep.covariances_from_normals(case["sn"].copy(), G.EPS)  # (the fixture's arrays are read-only)
    a = gicp(Cloud(case["src"]), t, G.LOOP_RADIUS, case["init"], src_cov=cs)
    perm = np.random.default_rng(4).permutation(ns)
    b = gicp(Cloud(case["src"][perm]), t, G.LOOP_RADIUS, case["init"], src_cov=cs[perm])
    np.testing.assert_allclose(b.transformation, a.transformation, rtol=0, atol=1e-12)
    assert (a.iterations, a.fitness) == (b.iterations, b.fitness)
    np.testing.assert_array_equal(corr_of(b, ns), corr_of(a, ns)[perm])
    # and the explicit covariances are the from-normals ones: the same bits as the normals path
    c = gicp(Cloud(case["src"], case["sn"]), t, G.LOOP_RADIUS, case["init"])
    np.testing.assert_array_equal(c.transformation, a.transformation)


def test_loop_on_empty_clouds():
    case = G.loop_case("identity")
    s, t = clouds_of(case)
    e = Cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    for a, b in ((e, t), (s, e)):
        out = gicp(a, b, G.LOOP_RADIUS)
        np.testing.assert_array_equal(out.transformation, np.eye(4))
        assert (out.fitness, out.inlier_rmse, len(out.correspondence_set)) == (0.0, 0.0, 0)


# ------------------------------------------------------------------------------------------- API
def test_registration_generalized_icp_api():
    case = G.loop_case("perturbed")
    ref, init = case["ref"], case["init"]
    src, sn, tgt, tn = case["src"], case["sn"], case["tgt"], case["tn"]
    got = matcher.registration_generalized_icp(PointCloud(src, sn), PointCloud(tgt, tn), G.LOOP_RADIUS, init)
    np.testing.assert_allclose(got.transformation, ref["transformation"], rtol=0, atol=1e-9)
    assert got.fitness == ref["fitness"] and abs(got.inlier_rmse - ref["inlier_rmse"]) <= 1e-12
    np.testing.assert_array_equal(got.correspondence_set, ref["correspondence_set"])
    # explicit covariances (they win over normals: wrong normals beside them change nothing)
    pc_s = PointCloud(src, np.roll(sn, 1, axis=0), covariances=case["cs"].copy())
    pc_t = PointCloud(tgt, covariances=case["ct"].copy())
    assert pc_s.has_covariances() and pc_t.has_covariances() and not PointCloud(src).has_covariances()
    cov = matcher.registration_generalized_icp(pc_s, pc_t, G.LOOP_RADIUS, init)
    np.testing.assert_allclose(cov.transformation, ref["transformation"], rtol=0, atol=1e-9)
    np.testing.assert_array_equal(cov.correspondence_set, ref["correspondence_set"])
    with pytest.raises(ValueError):
        matcher.registration_generalized_icp(pc_s, pc_t, 0.0, init)
    with pytest.raises(ValueError):
        matcher.registration_generalized_icp(pc_s, pc_t, G.LOOP_RADIUS, init, epsilon=0.0)
    with pytest.raises(ValueError):
        matcher.registration_generalized_icp(pc_s, pc_t, G.LOOP_RADIUS, init, epsilon=-1e-3)


def test_registration_generalized_icp_estimates_knn_normals():
    """Clouds with neither covariances nor normals: EstimateNormals(KDTreeSearchParamKNN(20)) first.
    Against the restatement fed by the device's own normals: 1e-9 as everywhere.  Against the
    restatement fed by prep_oracle's normals on exact 20-NN lists: those agree with the device's to
    1e-9 (tests/test_gpu_prep.py's tolerance), which moves a covariance C = ε·nnᵀ + (I − nnᵀ) by at
    most 2e-9 and M⁻¹, hence the update and its fixed point, by at most κ(M) = 1e3 times that
    relative: 1e-5 on T."""
    case = G.loop_case("perturbed")
    src, tgt, init = case["src"], case["tgt"], case["init"]
    got = matcher.registration_generalized_icp(src, PointCloud(tgt), G.LOOP_RADIUS, init)
    dn_s, dn_t = prep.estimate_normals_knn(src, 20), prep.estimate_normals_knn(tgt, 20)
    on_s = P.estimate_normals(src, None, 20, nbrs=CR.knn(src, 20))
    on_t = P.estimate_normals(tgt, None, 20, nbrs=CR.knn(tgt, 20))
    print("knn normals: worst |device - oracle|", max(np.abs(dn_s - on_s).max(), np.abs(dn_t - on_t).max()))
    np.testing.assert_allclose(dn_s, on_s, rtol=0, atol=1e-9)
    np.testing.assert_allclose(dn_t, on_t, rtol=0, atol=1e-9)
    for (ns_, nt_), tol in (((dn_s, dn_t), 1e-9), ((on_s, on_t), 1e-5)):
        ref = G.registration_generalized_icp(src, tgt, G.LOOP_RADIUS, init, G.covariances_from_normals(ns_),
                                             G.covariances_from_normals(nt_))
        print("knn path: |T - ref|", np.abs(got.transformation - ref["transformation"]).max(), "tolerance", tol)
        np.testing.assert_allclose(got.transformation, ref["transformation"], rtol=0, atol=tol)
        assert got.fitness == ref["fitness"]
        np.testing.assert_array_equal(got.correspondence_set, ref["correspondence_set"])


def test_point_cloud_carries_covariances():
    case = G.loop_case("identity")
    pc = PointCloud(case["src"][:50], case["sn"][:50], covariances=case["cs"][:50])
    T = synth.random_rigid(5, rot_range=0.3)
    R = T[:3, :3]
    moved = PointCloud(pc.points.copy(), pc.normals.copy(), pc.covariances.copy()).transform(T)
    np.testing.assert_allclose(moved.covariances, R @ case["cs"][:50] @ R.T, rtol=0, atol=1e-15)
    np.testing.assert_allclose(moved.covariances, G.rotate_covariances(R, case["cs"][:50]), rtol=0, atol=1e-14)
    sel = pc.select_by_index([3, 7, 9])
    np.testing.assert_array_equal(sel.covariances, case["cs"][[3, 7, 9]])
    assert not PointCloud(pc.points).select_by_index([1]).has_covariances()
    # and the device's covariances are what the cloud carries into the registration
    np.testing.assert_allclose(prep.covariances_from_normals(pc.normals.copy(), G.EPS), pc.covariances, rtol=0,
                               atol=1e-13)


# ----------------------------------------------------------------------------------- k-NN normals
@pytest.mark.parametrize("k", [2, 20])
def test_knn_normals_match_oracle(k):
    pts, true = synth.surface_points(500, seed=12)
    got = prep.estimate_normals_knn(pts, k)
    ref = P.estimate_normals(pts, None, k, nbrs=CR.knn(pts, k))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)
    if k == 2:  # fewer than three neighbours: Open3D's (0, 0, 1)
        np.testing.assert_array_equal(got, [[0, 0, 1]] * 500)
    else:
        assert np.abs(np.sum(got * true, axis=1)).mean() > 0.9  # they are the surface's normals
        oriented = prep.estimate_normals_knn(pts, k, normals=true)
        assert np.all(np.sum(oriented * true, axis=1) >= 0.0)
        np.testing.assert_allclose(np.abs(np.sum(oriented * got, axis=1)), 1.0, rtol=0, atol=1e-9)
    with pytest.raises(ValueError):
        prep.estimate_normals_knn(pts, 0)
    assert prep.estimate_normals_knn(np.zeros((0, 3)), k).shape == (0, 3)
