"""GPU parity of Colored ICP (colored.hip through m3d.core.color_gradients / colored_terms /
colored_icp, PointCloud / Ply colours and the matcher drop-in) against the numpy restatement
tests/colored_restatement.py.

Bounds.
* Gradients: rows the restatement leaves at zero (fewer than 4 neighbours, uniform colours) are
  exactly zero.  For the rest, per fixture, |gpu − longdouble| ≤ 8·|fp64 restatement − longdouble|
  + 1e-13·‖g‖ (both maxima over the fixture, ‖g‖ the largest gradient norm): the fp64
  restatement's own rounding is the yardstick, the factor 8 allows for another summation order
  over at most 30 rows.  Two runs give the same bits.
* One evaluation: per slot |gpu − ref| ≤ 1e-11·Σ|term| (the project's Generalized-ICP bound,
  tests/test_gpu_gicp.py); correspondences and the count are the exact NN's; brute force, the grid
  and repeated calls agree in every bit; tgt_gradient=None equals passing color_gradients' output.
* The loop: correspondences at every evaluation equal the restatement's (its fixture has no
  near-ties, asserted in tests/test_colored_cpu.py); iterations, fitness, converged equal; T within
  1e-9 and inlier_rmse within 1e-12, the Generalized-ICP test's bounds.
"""
import numpy as np
import pytest

import colored_restatement as CI
import gicp_restatement as G
import matcher
import robust_restatement as R
from m3d import plyio, prep
from m3d.core import Cloud, color_gradients, colored_icp, colored_terms
from m3d.types import PointCloud
from matcher import robust as K

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("n", CI.GRADIENT_NS)
def test_gradients_match_restatement(n):
    f = CI.gradient_case(n)
    c = Cloud(f["pts"], f["nrm"])
    got = color_gradients(c, f["col"], f["radius"])
    assert got.shape == (n, 3)
    np.testing.assert_array_equal(color_gradients(c, f["col"], f["radius"]), got)  # two runs, equal bits
    lens = np.array([len(x) for x in f["lists"]], np.int64)
    zero = lens < 4
    np.testing.assert_array_equal(got[zero], np.zeros((int(zero.sum()), 3)))
    if n >= 257:
        assert zero.sum() == min(4, n // 64) and (lens == CI.MAX_NN).mean() > 0.5
        assert np.all(np.abs(got[~zero]).sum(axis=1) > 0)
        gld = f["gld"]
        yard = float(np.abs(f["g64"] - gld).max())
        norm = float(np.sqrt((gld.astype(np.float64) ** 2).sum(axis=1)).max())
        err = float(np.abs(got - gld).max())
        print(f"n={n}: |gpu - ld| {err:.3e}, |fp64 - ld| {yard:.3e}, worst ratio to the bound "
              f"{err / (8 * yard + 1e-13 * norm):.3f}, lists at the cap {(lens == CI.MAX_NN).sum()} of {n}")
        assert err <= 8 * yard + 1e-13 * norm
    else:
        assert zero.all()


def test_gradients_of_uniform_colours_are_exactly_zero():
    f = CI.gradient_case(2000, uniform=True)
    got = color_gradients(Cloud(f["pts"], f["nrm"]), f["col"], f["radius"])
    np.testing.assert_array_equal(got, np.zeros((2000, 3)))


def test_gradients_max_nn_below_the_cap_and_list_contract():
    """max_nn = 7: the list is cut at 7, so the rows are the 6 nearest others."""
    f = CI.gradient_case(257)
    lists = CI.hybrid_lists(f["pts"], f["radius"], 7)
    ref = CI.color_gradients(f["pts"], f["nrm"], f["col"], f["radius"], 7, lists=lists)
    got = color_gradients(Cloud(f["pts"], f["nrm"]), f["col"], f["radius"], 7)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-11 * np.abs(ref).max())
    np.testing.assert_array_equal(got[np.array([len(x) for x in lists]) < 4], 0.0)


# ------------------------------------------------------------------------------- one evaluation
def clouds_of(f):
    return Cloud(f["src"], f["sn"]), Cloud(f["tgt"], f["tn"])


@pytest.mark.parametrize("ns", CI.EVAL_NS)
@pytest.mark.parametrize("identity", [False, True])
def test_one_evaluation(ns, identity):
    f = CI.eval_case(ns, identity)
    ref, scale = CI.colored_terms(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], f["corr"])
    s, t = clouds_of(f)
    out = {}
    for nn in ("brute", "grid"):
        sums, idx = colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, tgt_gradient=f["grad"], nn=nn)
        out[nn] = (sums, idx.cpu().numpy())
    sums, idx = out["grid"]
    np.testing.assert_array_equal(idx, f["j"])
    if ns > 1:
        assert 0 < (f["j"] >= 0).sum() < ns  # the radius leaves some sources unmatched
    assert sums[28] == ref[28] == (f["j"] >= 0).sum()
    err = np.abs(sums - ref)
    pos = scale > 0
    print(f"ns={ns} identity={identity}: worst |gpu - ref| / sum|term| =", (err[pos] / scale[pos]).max() if pos.any() else 0.0)
    assert np.all(err <= 1e-11 * scale)
    np.testing.assert_array_equal(out["brute"][0], sums)
    np.testing.assert_array_equal(out["brute"][1], idx)
    again, _ = colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, tgt_gradient=f["grad"], nn="grid")
    np.testing.assert_array_equal(again, sums)


def test_one_evaluation_computes_its_own_gradients():
    """tgt_gradient=None is color_gradients(tgt, colours, 2·max_dist, 30), bit for bit."""
    f = CI.eval_case(1000)
    s, t = clouds_of(f)
    own, idx = colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS)
    dev = color_gradients(t, f["tc"], 2.0 * G.RADIUS, 30)
    given, idx2 = colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, tgt_gradient=dev)
    np.testing.assert_array_equal(own, given)
    np.testing.assert_array_equal(idx.cpu().numpy(), idx2.cpu().numpy())
    assert np.abs(dev - f["grad"]).max() <= 1e-9 * np.abs(f["grad"]).max()


KERNELS = {"l2": K.L2Loss, "l1": K.L1Loss, "huber": K.HuberLoss, "cauchy": K.CauchyLoss, "gm": K.GMLoss,
           "tukey": K.TukeyLoss}


@pytest.mark.parametrize("name", list(KERNELS))
def test_one_evaluation_with_each_kernel(name):
    f = CI.eval_case(1000)
    kind = R.KINDS[name]
    k = f["k"]
    kernel = KERNELS[name](k) if kind in R.READS_K else KERNELS[name]()
    ref, scale = CI.colored_terms(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], f["corr"], kind=kind, k=k)
    s, t = clouds_of(f)
    sums, idx = colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, tgt_gradient=f["grad"], kernel=kernel)
    np.testing.assert_array_equal(idx.cpu().numpy(), f["j"])
    err = np.abs(sums - ref)
    print(f"{name}: worst |gpu - ref| / sum|term| =", (err[scale > 0] / scale[scale > 0]).max())
    assert np.all(err <= 1e-11 * scale)
    if kind in (R.HUBER, R.TUKEY):  # both branches of the weight are taken
        r = CI.colored_rows(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], f["corr"])[0]
        assert 0 < (np.abs(r) > k).sum() < r.size
    if kind != R.L2:
        plain, _ = CI.colored_terms(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], f["corr"])
        assert np.abs(sums[:27] - plain[:27]).max() > 1e-6 * np.abs(plain[:27]).max()  # the weights act
        assert abs(sums[27] - plain[27]) <= 1e-11 * scale[27]                          # Σr² is unweighted


@pytest.mark.parametrize("nn", ["brute", "grid"])
def test_one_evaluation_without_matches_and_empty_clouds(nn):
    f = CI.eval_case(257)
    s, t = clouds_of(f)
    sums, idx = colored_terms(s, t, f["sc"], f["tc"], f["T"], 1e-6, nn=nn)  # no target that close
    np.testing.assert_array_equal(sums, np.zeros(30))
    np.testing.assert_array_equal(idx.cpu().numpy(), np.full(257, -1))
    e = Cloud(np.zeros((0, 3)), np.zeros((0, 3)))
    ec = np.zeros((0, 3))
    sums, idx = colored_terms(e, t, ec, f["tc"], f["T"], G.RADIUS, nn=nn)
    np.testing.assert_array_equal(sums, np.zeros(30))
    assert len(idx) == 0
    sums, idx = colored_terms(s, e, f["sc"], ec, f["T"], G.RADIUS, nn=nn)
    np.testing.assert_array_equal(sums, np.zeros(30))
    np.testing.assert_array_equal(idx.cpu().numpy(), np.full(257, -1))
    for a, ac, b, bc in ((e, ec, t, f["tc"]), (s, f["sc"], e, ec)):
        out = colored_icp(a, b, ac, bc, G.RADIUS, nn=nn)
        np.testing.assert_array_equal(out.transformation, np.eye(4))
        assert (out.fitness, out.inlier_rmse, len(out.correspondence_set)) == (0.0, 0.0, 0)
    assert color_gradients(e, ec, 0.5).shape == (0, 3)


def test_bad_arguments_raise():
    f = CI.eval_case(257)
    s, t = clouds_of(f)
    sc, tc, T = f["sc"], f["tc"], f["T"]
    with pytest.raises(ValueError):
        color_gradients(t, tc, 0.0)
    with pytest.raises(ValueError):
        color_gradients(Cloud(f["tgt"]), tc, 0.5)  # no normals
    with pytest.raises(ValueError):
        color_gradients(t, tc, 0.5, max_nn=65)
    with pytest.raises(ValueError):
        colored_terms(s, t, sc, tc, T, 0.0)
    for lam in (-0.1, 1.1):
        with pytest.raises(ValueError):
            colored_terms(s, t, sc, tc, T, G.RADIUS, lambda_geometric=lam)
        with pytest.raises(ValueError):
            colored_icp(s, t, sc, tc, G.RADIUS, lambda_geometric=lam)
    with pytest.raises(ValueError):
        colored_terms(s, Cloud(f["tgt"]), sc, tc, T, G.RADIUS)  # no target normals
    with pytest.raises(ValueError):
        colored_icp(s, Cloud(f["tgt"]), sc, tc, G.RADIUS)
    with pytest.raises(ValueError):
        colored_terms(s, t, None, tc, T, G.RADIUS)
    with pytest.raises(ValueError):
        colored_terms(s, t, sc, None, T, G.RADIUS)
    with pytest.raises(ValueError):
        colored_icp(s, t, sc, tc, G.RADIUS, max_iteration=-1)
    with pytest.raises(ValueError):
        colored_terms(s, t, sc, tc, T, G.RADIUS, nn="octree")
    pc_s, pc_t = PointCloud(f["src"], f["sn"], colors=sc), PointCloud(f["tgt"], f["tn"], colors=tc)
    with pytest.raises(ValueError):
        matcher.registration_colored_icp(PointCloud(f["src"], f["sn"]), pc_t, G.RADIUS)
    with pytest.raises(ValueError):
        matcher.registration_colored_icp(pc_s, PointCloud(f["tgt"], f["tn"]), G.RADIUS)
    with pytest.raises(ValueError):
        matcher.registration_colored_icp(pc_s, PointCloud(f["tgt"], colors=tc), G.RADIUS)
    with pytest.raises(ValueError):
        matcher.registration_colored_icp(pc_s, pc_t, 0.0)


# --------------------------------------------------------------------------------------- the loop
def corr_of(out, ns):
    j = np.full(ns, -1, np.int64)
    j[out.correspondence_set[:, 0]] = out.correspondence_set[:, 1]
    return j


@pytest.mark.parametrize("kind", ["identity", "perturbed"])
def test_loop_matches_restatement(kind):
    case = CI.loop_case(kind)
    ref, evals, init = case["ref"], case["evals"], case["init"]
    s, t = clouds_of(case)
    sc, tc = case["sc"], case["tc"]
    ns = len(case["src"])
    # correspondences at every evaluation: a run stopped after k updates ends on evaluation k
    for k in range(len(evals) - 1):
        out = colored_icp(s, t, sc, tc, G.LOOP_RADIUS, init, max_iteration=k)
        np.testing.assert_array_equal(corr_of(out, ns), evals[k][1], err_msg=f"evaluation {k}")
        assert out.iterations == k and not out.converged
        if k == 0:
            np.testing.assert_array_equal(out.transformation, init)
            assert out.fitness == (evals[0][1] >= 0).mean()
    out = colored_icp(s, t, sc, tc, G.LOOP_RADIUS, init)
    np.testing.assert_array_equal(corr_of(out, ns), evals[-1][1])
    assert (out.iterations, out.fitness, out.converged) == (ref["iterations"], ref["fitness"], ref["converged"])
    print(f"{kind}: |T - ref| {np.abs(out.transformation - ref['transformation']).max():.3e}, "
          f"|rmse - ref| {abs(out.inlier_rmse - ref['inlier_rmse']):.3e}, iterations {out.iterations}")
    np.testing.assert_allclose(out.transformation, ref["transformation"], rtol=0, atol=1e-9)
    assert abs(out.inlier_rmse - ref["inlier_rmse"]) <= 1e-12
    np.testing.assert_array_equal(out.correspondence_set, ref["correspondence_set"])
    # brute force and the grid: the same bits
    b = colored_icp(s, t, sc, tc, G.LOOP_RADIUS, init, nn="brute")
    np.testing.assert_array_equal(b.transformation, out.transformation)
    assert (b.fitness, b.inlier_rmse, b.iterations, b.converged) == (out.fitness, out.inlier_rmse, out.iterations,
                                                                     out.converged)
    np.testing.assert_array_equal(b.correspondence_set, out.correspondence_set)


def test_slide_fixture_through_the_matcher():
    f = CI.slide_pair()
    ref = CI.slide_run()
    src = PointCloud(f["src"], f["sn"], colors=f["sc"])
    tgt = PointCloud(f["tgt"], f["tn"], colors=f["tc"])
    got = matcher.registration_colored_icp(src, tgt, CI.SLIDE_RADIUS)
    print("slide: |T - ref|", np.abs(got.transformation - ref["transformation"]).max(), "offset error",
          got.transformation[:3, 3] + CI.SLIDE_SHIFT)
    np.testing.assert_allclose(got.transformation, ref["transformation"], rtol=0, atol=1e-9)
    assert got.fitness == ref["fitness"]
    assert abs(got.transformation[1, 3] + CI.SLIDE_SHIFT[1]) <= abs(CI.SLIDE_SHIFT[1]) / 50
    # point-to-plane on the same pair leaves the y offset: the ridge does not see it
    geo = matcher.registration_icp(src, tgt, CI.SLIDE_RADIUS)
    print("slide: point-to-plane leaves", geo.transformation[:3, 3] + CI.SLIDE_SHIFT)
    # (the restatement's point-to-plane run keeps 99.97 % of it; the CPU test's condition is 90 %)
    assert abs(geo.transformation[1, 3] + CI.SLIDE_SHIFT[1]) >= 0.9 * abs(CI.SLIDE_SHIFT[1])


# ------------------------------------------------------------------------------------------- API
def test_voxel_down_sample_carries_colours():
    f = CI.slide_pair()
    pc = PointCloud(f["tgt"], f["tn"], colors=f["tc"])
    down = pc.voxel_down_sample(0.1)
    pts, nrm = prep.voxel_down_sample(f["tgt"], 0.1, normals=f["tn"])
    np.testing.assert_array_equal(down.points, pts)
    np.testing.assert_array_equal(down.normals, nrm)
    assert down.has_colors() and 100 < len(pts) < len(f["tgt"])
    ref = CI.voxel_means(f["tgt"], f["tc"], 0.1)
    np.testing.assert_allclose(down.points, CI.voxel_means(f["tgt"], f["tgt"], 0.1), rtol=0, atol=1e-15)
    print("voxel colours: worst |diff|", np.abs(down.colors - ref).max())
    np.testing.assert_allclose(down.colors, ref, rtol=0, atol=1e-15)
    plain = PointCloud(f["tgt"]).voxel_down_sample(0.1)
    assert not plain.has_colors() and not plain.has_normals()
    np.testing.assert_array_equal(plain.points, pts)


def test_ply_carries_colours(tmp_path):
    from ply.ply import Ply

    f = CI.slide_pair()
    u8 = np.rint(f["tc"] * 255.0)
    p = tmp_path / "coloured.ply"
    plyio.write_ply(p, f["tgt"], colors=f["tc"], binary=True)
    ply = Ply(p, voxel_size=0.1)
    np.testing.assert_array_equal(ply.pcd.colors, u8 / 255.0)
    assert ply.pcd_down.has_colors() and ply.pcd_down.has_normals()
    np.testing.assert_allclose(ply.pcd_down.colors, CI.voxel_means(f["tgt"], u8 / 255.0, 0.1), rtol=0, atol=1e-15)
    q = tmp_path / "plain.ply"
    plyio.write_ply(q, f["tgt"], binary=True)
    plain = Ply(q, voxel_size=0.1)
    assert not plain.pcd.has_colors() and not plain.pcd_down.has_colors()
    # and the cluster / keypoint selections keep them
    kept = Ply(p, voxel_size=0.1, keypoints={})
    assert len(kept.pcd_down.colors) == len(kept.pcd_down.points) == len(kept.keypoint_indices)
