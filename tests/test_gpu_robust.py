"""GPU parity of the robust kernels (robust.hip through m3d.core.robust_terms / gicp_terms / icp /
gicp and the matcher drop-ins) against the numpy restatement tests/robust_restatement.py.

Bounds.
* One evaluation: per slot |gpu − ref| ≤ 1e-11·Σ|term| (Σ|term| = the slot's absolute-value sum of
  the restatement), the bound tests/test_gpu_gicp.py::test_one_evaluation holds gicp.hip to.
  Point-to-plane rows are a dozen roundings each: measured worst ratio 2.1e-15.  The Generalized
  ICP rows go through W = M^(−1/2), κ(M) ≤ 1/ε = 1e3: the device's Jacobi and the restatement's
  eigh differ by up to 6.9e-14 relative on such M (tests/test_robust_cpu.py), so r and J move by
  that much, and a weight multiplies it by its own condition — L1's 1/|r| near r = 0, Tukey's
  (1 − (r/k)²)² near |r| = k (the one-pair case has k = |r| of one row by construction).
  Measured on the device against the restatement, worst ratio per kind over the four sizes:
  L2 1.7e-14, L1 2.8e-12, Huber 6.6e-14, Cauchy 8.1e-14, GM 9.6e-14, Tukey 2.1e-12 (ns = 1;
  3.0e-14 otherwise).  The project's bound holds everywhere, by a factor 3.6 at the worst, and is
  kept.  Correspondences, the count and Σd² 's inputs are the exact NN's; brute force, the grid
  and repeated calls agree in every bit.
* The loops: correspondences at every evaluation equal the restatement's (the fixture has no
  near-ties, asserted in tests/test_robust_cpu.py); iterations, fitness, converged equal; T within
  1e-9, inlier_rmse within 1e-12, as tests/test_gpu_gicp.py::test_loop_matches_restatement.
"""
import numpy as np
import pytest

import gicp_restatement as G
import icp_oracle as I
import matcher
import robust_restatement as R
from m3d import _lib
from m3d.core import Cloud, colored_terms, gicp, gicp_terms, icp, robust_terms
from m3d.types import FastGlobalRegistrationOption, PointCloud

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

LOSS = {R.L2: lambda k: matcher.L2Loss(), R.L1: lambda k: matcher.L1Loss(), R.HUBER: matcher.HuberLoss,
        R.CAUCHY: matcher.CauchyLoss, R.GM: matcher.GMLoss, R.TUKEY: matcher.TukeyLoss}


def within(sums, ref, scale, what):
    err = np.abs(sums - ref)
    ok = scale > 0
    print(f"{what}: worst |gpu - ref| / sum|term| =", (err[ok] / scale[ok]).max() if ok.any() else 0.0)
    assert np.all(err <= 1e-11 * scale), what


# ------------------------------------------------------------------------------- one evaluation
@pytest.mark.parametrize("ns", R.EVAL_NS)
@pytest.mark.parametrize("kind", sorted(R.KINDS.values()))
def test_one_evaluation(ns, kind):
    c = R.eval_case(ns)
    s, t = Cloud(c["src"], c["sn"]), Cloud(c["tgt"], c["tn"])
    for est, k in (("plane", c["k_plane"]), ("gicp", c["k_gicp"])):
        loss = LOSS[kind](k)
        if est == "plane":
            ref, scale = R.robust_plane_sums(c["pcd"], c["tgt"], c["tn"], c["corr"], kind, k)
            call = lambda nn: robust_terms(s, t, c["T"], G.RADIUS, loss, nn=nn)
        else:
            ref, scale = R.robust_gicp_sums(c["pcd"], c["cs"], c["tgt"], c["ct"], c["corr"], kind, k)
            call = lambda nn: gicp_terms(s, t, c["T"], G.RADIUS, epsilon=G.EPS, nn=nn, kernel=loss)
        sums, idx = call("grid")
        idx = idx.cpu().numpy()
        np.testing.assert_array_equal(idx, c["j"])
        assert sums[28] == ref[28] == (c["j"] >= 0).sum()
        within(sums, ref, scale, f"{est} ns={ns} kind={kind}")
        b_sums, b_idx = call("brute")
        np.testing.assert_array_equal(b_sums, sums)
        np.testing.assert_array_equal(b_idx.cpu().numpy(), idx)
        again, _ = call("grid")
        np.testing.assert_array_equal(again, sums)
    if kind == R.L2 and len(c["corr"]):
        # L2 through the new plane pass against the point-to-plane oracle itself
        sums, _ = robust_terms(s, t, c["T"], G.RADIUS, matcher.L2Loss())
        JTJ, JTr, r2 = I.point_to_plane_terms(c["pcd"], c["tgt"], c["tn"], c["corr"])
        _, scale = R.robust_plane_sums(c["pcd"], c["tgt"], c["tn"], c["corr"])
        oracle = np.array([JTJ[a, b] for a, b in G.UPPER] + list(JTr) + [r2, sums[28], sums[29]])
        within(sums, oracle, scale, f"plane ns={ns} L2 against icp_oracle")


def test_l2_or_null_through_the_c_entry_points_is_the_call_without_a_kernel():
    """m3d_gicp_terms_robust / m3d_gicp_run_robust with NULL or kind L2 (the Python layer never
    sends either there): the bits of m3d_gicp_terms / m3d_gicp_run."""
    import ctypes as C

    from m3d.core import _T16, stream_handle

    c = R.eval_case(1000)
    s, t = Cloud(c["src"], c["sn"]), Cloud(c["tgt"], c["tn"])
    lib, T16 = s.ctx.lib, _T16(c["T"])
    plain, _ = gicp_terms(s, t, c["T"], G.RADIUS, epsilon=G.EPS, with_correspondences=False)
    run = gicp(s, t, G.RADIUS, c["T"], epsilon=G.EPS, max_iteration=3, with_correspondences=False)
    p = _lib.GicpParams(1e-6, 1e-6, 3, _lib.NN_GRID, G.EPS)
    for kernel in (None, C.byref(_lib.RobustKernel(_lib.ROBUST_L2, float("nan")))):
        sums = (C.c_double * 32)()
        s.ctx.check(lib.m3d_gicp_terms_robust(s.ctx.h, s.h, t.h, None, None, T16, G.RADIUS, _lib.NN_GRID, G.EPS,
                                              kernel, sums, None, stream_handle()), "gicp_terms_robust")
        np.testing.assert_array_equal(np.array(sums[:30]), plain)
        res = _lib.IcpResult()
        s.ctx.check(lib.m3d_gicp_run_robust(s.ctx.h, s.h, t.h, None, None, T16, G.RADIUS, C.byref(p), kernel,
                                            C.byref(res), None, stream_handle()), "gicp_run_robust")
        np.testing.assert_array_equal(np.array(res.T[:]).reshape(4, 4), run.transformation)
        assert (res.fitness, res.inlier_rmse, res.iterations) == (run.fitness, run.inlier_rmse, run.iterations)


@pytest.mark.parametrize("ns", [257, 256])
def test_every_side_terms_pass_shares_the_skeleton(ns):
    """What terms_pass.h does for every estimator — the winner, corr, the count and Σd² — is the
    same bits whichever estimator rides on it: plain Generalized ICP, robust point-to-plane L2,
    robust Generalized ICP Huber and Colored ICP (a constant colour on both clouds), grid and brute
    force.  257 sources: two blocks, the second with one live lane; 256 (the same case sliced; a
    source's winner does not depend on the other sources): exactly one full block."""
    c = R.eval_case(257)
    j = c["j"][:ns]
    assert (j < 0).any() and (j >= 0).any()  # some sources unmatched
    s, t = Cloud(c["src"][:ns], c["sn"][:ns]), Cloud(c["tgt"], c["tn"])
    sc, tc = np.full((ns, 3), 0.5), np.full((len(c["tgt"]), 3), 0.5)
    calls = {"gicp": lambda nn: gicp_terms(s, t, c["T"], G.RADIUS, epsilon=G.EPS, nn=nn),
             "plane l2": lambda nn: robust_terms(s, t, c["T"], G.RADIUS, matcher.L2Loss(), nn=nn),
             "gicp huber": lambda nn: gicp_terms(s, t, c["T"], G.RADIUS, epsilon=G.EPS, nn=nn,
                                                 kernel=matcher.HuberLoss(c["k_gicp"])),
             "colored": lambda nn: colored_terms(s, t, sc, tc, c["T"], G.RADIUS, nn=nn)}
    first = None
    for name, call in calls.items():
        for nn in ("grid", "brute"):
            sums, idx = call(nn)
            np.testing.assert_array_equal(idx.cpu().numpy(), j, err_msg=f"{name} {nn}")
            assert sums[28] == (j >= 0).sum(), (name, nn)
            first = sums if first is None else first
            assert (sums[28].tobytes(), sums[29].tobytes()) == (first[28].tobytes(), first[29].tobytes()), (name, nn)


# ---------------------------------------------------------------------------------------- loops
def clouds():
    f = R.outlier_pair()
    return Cloud(f["src"], f["sn"]), Cloud(f["tgt"], f["tn"])


def corr_of(out, ns):
    j = np.full(ns, -1, np.int64)
    j[out.correspondence_set[:, 0]] = out.correspondence_set[:, 1]
    return j


def run(est, s, t, init, loss, **kw):
    if est == "plane":
        return icp(s, t, G.LOOP_RADIUS, init, kernel=loss, **kw)
    return gicp(s, t, G.LOOP_RADIUS, init, epsilon=G.EPS, kernel=loss, **kw)


def same(a, b):
    np.testing.assert_array_equal(a.transformation, b.transformation)
    assert (a.fitness, a.inlier_rmse, a.iterations, a.converged) == (b.fitness, b.inlier_rmse, b.iterations, b.converged)
    np.testing.assert_array_equal(a.correspondence_set, b.correspondence_set)


@pytest.mark.parametrize("est", ["plane", "gicp"])
@pytest.mark.parametrize("kind", [R.TUKEY, R.HUBER])
@pytest.mark.parametrize("init_kind", ["identity", "perturbed"])
def test_loop_matches_restatement(est, kind, init_kind):
    c = R.loop_case(est, kind, init_kind)
    ref, evals, init, loss = c["ref"], c["evals"], c["init"], LOSS[kind](c["k"])
    s, t = clouds()
    ns = s.n
    # correspondences at every evaluation: a run stopped after k updates ends on evaluation k
    for k in range(len(evals) - 1):
        out = run(est, s, t, init, loss, max_iteration=k)
        np.testing.assert_array_equal(corr_of(out, ns), evals[k][1], err_msg=f"evaluation {k}")
        assert out.iterations == k and not out.converged
        if k == 0:
            np.testing.assert_array_equal(out.transformation, init)
            assert out.fitness == (evals[0][1] >= 0).mean()
    out = run(est, s, t, init, loss)
    np.testing.assert_array_equal(corr_of(out, ns), evals[-1][1])
    assert (out.iterations, out.fitness, out.converged) == (ref["iterations"], ref["fitness"], ref["converged"])
    print(f"{est} {kind} {init_kind}: |T - ref| {np.abs(out.transformation - ref['transformation']).max():.3e}, "
          f"|rmse - ref| {abs(out.inlier_rmse - ref['inlier_rmse']):.3e}, iterations {out.iterations}")
    np.testing.assert_allclose(out.transformation, ref["transformation"], rtol=0, atol=1e-9)
    assert abs(out.inlier_rmse - ref["inlier_rmse"]) <= 1e-12
    np.testing.assert_array_equal(out.correspondence_set, ref["correspondence_set"])
    same(run(est, s, t, init, loss, nn="brute"), out)  # brute force and the grid: the same bits
    same(run(est, s, t, init, loss), out)              # and a second run


# ------------------------------------------------------- the test that fails without the feature
def clouds_pc():
    f = R.outlier_pair()
    return PointCloud(f["src"], f["sn"]), PointCloud(f["tgt"], f["tn"])


@pytest.mark.parametrize("est", ["plane", "gicp"])
@pytest.mark.parametrize("init_kind", ["identity", "perturbed"])
def test_tukey_lands_closer_than_no_kernel(est, init_kind):
    f = R.outlier_pair()
    clean = f["src"][~f["outlier"]]
    src, tgt = clouds_pc()
    tukey, l2 = R.loop_case(est, R.TUKEY, init_kind), R.loop_case(est, R.L2, init_kind)
    init = tukey["init"]
    call = matcher.registration_icp if est == "plane" else matcher.registration_generalized_icp
    got = call(src, tgt, G.LOOP_RADIUS, init, kernel=matcher.TukeyLoss(tukey["k"]))
    none = call(src, tgt, G.LOOP_RADIUS, init, kernel=None)
    plain = call(src, tgt, G.LOOP_RADIUS, init)
    assert none.transformation.tobytes() == plain.transformation.tobytes()
    assert (none.fitness, none.inlier_rmse) == (plain.fitness, plain.inlier_rmse)
    np.testing.assert_array_equal(none.correspondence_set, plain.correspondence_set)
    l2_loss = call(src, tgt, G.LOOP_RADIUS, init, kernel=matcher.L2Loss())
    assert l2_loss.transformation.tobytes() == plain.transformation.tobytes()
    e = [R.pose_error(x, f["T_true"], clean) for x in (got.transformation, none.transformation)]
    e_ref = [R.pose_error(x["ref"]["transformation"], f["T_true"], clean) for x in (tukey, l2)]
    print(f"{est} {init_kind}: pose error Tukey {e[0]:.4e} / none {e[1]:.4e} = {e[0] / e[1]:.4f}; "
          f"restatement {e_ref[0]:.4e} / {e_ref[1]:.4e} = {e_ref[0] / e_ref[1]:.4f}")
    assert e[0] <= 0.5 * e[1]
    # by the factor the restatement shows: a transform within 1e-9 of the restatement's moves a pose
    # error by at most ≈ 1e-8 (|p| ≤ 10), 1e-6 relative of errors ≥ 1e-2: 1e-5 on the ratio with margin
    assert abs(e[0] / e[1] - e_ref[0] / e_ref[1]) <= 1e-5


# ---------------------------------------------------------------------------------------- edges
@pytest.mark.parametrize("nn", ["brute", "grid"])
def test_empty_clouds_and_no_matches(nn):
    c = R.eval_case(257)
    s, t = Cloud(c["src"], c["sn"]), Cloud(c["tgt"], c["tn"])
    e = Cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    loss = matcher.TukeyLoss(c["k_plane"])
    terms = (lambda a, b, r: robust_terms(a, b, c["T"], r, loss, nn=nn),
             lambda a, b, r: gicp_terms(a, b, c["T"], r, nn=nn, kernel=loss))
    for call in terms:
        for a, b, r, n in ((s, t, 1e-6, 257), (e, t, G.RADIUS, 0), (s, e, G.RADIUS, 257), (e, e, G.RADIUS, 0)):
            sums, idx = call(a, b, r)
            np.testing.assert_array_equal(sums, np.zeros(30))
            np.testing.assert_array_equal(idx.cpu().numpy(), np.full(n, -1))
    for est in ("plane", "gicp"):
        for a, b in ((e, t), (s, e), (e, e)):
            out = run(est, a, b, None, loss, nn=nn)
            np.testing.assert_array_equal(out.transformation, np.eye(4))
            assert (out.fitness, out.inlier_rmse, len(out.correspondence_set)) == (0.0, 0.0, 0)
    # a radius that matches nothing: the identity update, the loop ends as the restatement's does
    for est in ("plane", "gicp"):
        if est == "plane":
            out = icp(s, t, 1e-6, c["T"], kernel=loss, nn=nn)
        else:
            out = gicp(s, t, 1e-6, c["T"], kernel=loss, nn=nn)
        np.testing.assert_array_equal(out.transformation, c["T"])
        assert (out.fitness, out.inlier_rmse, out.iterations, out.converged) == (0.0, 0.0, 1, True)


@pytest.mark.parametrize("est", ["plane", "gicp"])
def test_tukey_below_every_residual_gives_a_zero_step(est):
    """k below every |r|: all weights are zero, the system is zero, the LDLT rule gives a zero step
    — the identity update — and the loop ends after it as the restatement's does."""
    f = R.outlier_pair()
    s, t = clouds()
    first = R.loop_case(est, R.TUKEY, "perturbed")
    init, (pcd, j) = first["init"], first["evals"][0]
    corr = np.stack([np.nonzero(j >= 0)[0], j[j >= 0]], axis=1)
    if est == "plane":
        r = R.plane_rows(pcd, f["tgt"], f["tn"], corr)[0]
        k = 0.5 * np.abs(r).min()
        ref = R.registration_icp_robust(f["src"], f["tgt"], f["tn"], G.LOOP_RADIUS, init, R.TUKEY, k)
    else:
        r = R.gicp_rows(pcd, G.rotate_covariances(init[:3, :3], f["cs"]), f["tgt"], f["ct"], corr)[0]
        k = 0.5 * np.abs(r).min()
        ref = R.registration_gicp_robust(f["src"], f["tgt"], G.LOOP_RADIUS, init, f["cs"], f["ct"], R.TUKEY, k)
    assert k > 0.0 and (ref["iterations"], ref["converged"]) == (1, True)
    out = run(est, s, t, init, matcher.TukeyLoss(k))
    np.testing.assert_array_equal(out.transformation, ref["transformation"])
    np.testing.assert_array_equal(out.transformation, init)
    assert (out.iterations, out.converged, out.fitness) == (1, True, ref["fitness"])
    np.testing.assert_array_equal(out.correspondence_set, ref["correspondence_set"])


# ----------------------------------------------------------------------------------- rejections
class Kind7:
    kind, k = 7, 1.0


def test_rejections():
    c = R.eval_case(257)
    s, t = Cloud(c["src"], c["sn"]), Cloud(c["tgt"], c["tn"])
    calls = (lambda loss: robust_terms(s, t, c["T"], G.RADIUS, loss),
             lambda loss: gicp_terms(s, t, c["T"], G.RADIUS, kernel=loss),
             lambda loss: icp(s, t, G.RADIUS, c["T"], kernel=loss),
             lambda loss: gicp(s, t, G.RADIUS, c["T"], kernel=loss))
    for call in calls:
        for kind in R.READS_K:
            for k in (0.0, -1.0, float("nan"), float("inf")):
                with pytest.raises(ValueError):
                    call(LOSS[kind](k))
        with pytest.raises(ValueError):
            call(Kind7())
        call(matcher.L1Loss())  # reads no k
    no_normals = Cloud(c["tgt"])
    with pytest.raises(ValueError):
        robust_terms(s, no_normals, c["T"], G.RADIUS, matcher.TukeyLoss(0.1))
    with pytest.raises(ValueError):
        icp(s, no_normals, G.RADIUS, c["T"], kernel=matcher.TukeyLoss(0.1))
    with pytest.raises(ValueError):
        robust_terms(s, t, c["T"], 0.0, matcher.TukeyLoss(0.1))
    with pytest.raises(ValueError):
        robust_terms(s, t, c["T"], G.RADIUS, matcher.TukeyLoss(0.1), nn="octree")
    with pytest.raises(ValueError):  # TransformationEstimationPointToPoint takes no kernel
        icp(s, t, G.RADIUS, c["T"], estimation=_lib.EST_POINT_TO_POINT, kernel=matcher.TukeyLoss(0.1))
    with pytest.raises(ValueError):
        matcher.registration_icp(PointCloud(c["src"]), PointCloud(c["tgt"], c["tn"]), G.RADIUS, c["T"],
                                 estimation="point_to_point", kernel=matcher.HuberLoss(0.1))
    with pytest.raises(ValueError):
        matcher.registration_icp(PointCloud(c["src"]), PointCloud(c["tgt"]), G.RADIUS, c["T"],
                                 kernel=matcher.HuberLoss(0.1))


# --------------------------------------------------------------------------------- pass-through
def test_refine_and_register_pass_the_kernel_through():
    f = R.outlier_pair()
    src, tgt = clouds_pc()
    c = R.loop_case("plane", R.TUKEY, "perturbed")
    loss, init = matcher.TukeyLoss(c["k"]), c["init"]
    voxel = G.LOOP_RADIUS / 0.4
    direct = matcher.registration_icp(src, tgt, voxel * 0.4, init, "point_to_plane", kernel=loss)
    got = matcher.refine_registration(src, tgt, init, voxel, kernel=loss)
    plain = matcher.refine_registration(src, tgt, init, voxel)
    assert got.transformation.tobytes() == direct.transformation.tobytes()
    assert (got.fitness, got.inlier_rmse) == (direct.fitness, direct.inlier_rmse)
    assert plain.transformation.tobytes() != got.transformation.tobytes()
    np.testing.assert_allclose(got.transformation, c["ref"]["transformation"], rtol=0, atol=1e-9)
    # register: the coarse stage on given correspondences (the true pose's), then the same ICP stage
    _, _, corr, _ = I.registration_result(I.transform_points(f["T_true"], f["src"]), f["tgt"], 0.1)
    assert len(corr) > 100
    option = FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * voxel)
    coarse = matcher.registration_fgr_based_on_correspondence(src, tgt, corr, option)
    want = matcher.registration_icp(src, tgt, voxel * 0.4, coarse.transformation, "point_to_plane", kernel=loss)
    res = matcher.register(src, tgt, voxel_size=voxel, correspondences=corr, coarse="fgr", kernel=loss)
    assert res.transformation.tobytes() == want.transformation.tobytes()
    assert (res.fitness, res.inlier_rmse) == (want.fitness, want.inlier_rmse)
    unweighted = matcher.register(src, tgt, voxel_size=voxel, correspondences=corr, coarse="fgr")
    assert unweighted.transformation.tobytes() != res.transformation.tobytes()
