"""GPU parity of plane segmentation (m3d_segment_plane, m3d_plane_score through m3d.prep,
PointCloud and Ply) against the CPU restatement in tests/plane_restatement.py.

What is compared how.  Bit-equal or integer-equal, no tolerance: the per-hypothesis counts,
best_index, best_count, evaluated, iterations, ransac_plane and the inlier indices — both sides
round every operation of the sampler, the plane fits and dist = |((a·x + b·y) + c·z) + d| the same
way (fp64, no contraction).  err and best_rmse: rtol 1e-12 — the device adds the same non-negative
terms sequentially inside a chunk of PLANE_CHUNK points and the chunk sums in a fixed tree, the
restatement sequentially over the cloud (error ≤ n·2⁻⁵³ ≈ 2e-12 in the worst case and
~√n·2⁻⁵³ ≈ 2e-14 for rounding errors of mixed sign at n = 2e4; the argument of
tests/test_gpu_clean.py's header).  The refit plane: 100 × the restatement's own difference between
two summation orders for that input, floor 1e-13 on the normal and 1e-13·max(1, |d|) on d
(REFIT_MEASURED below lists the differences the tolerances come from).

Before a run is compared the restatement alone must show that no decision hangs on a last bit:
every rmse-decided tie has a relative gap ≥ 1e-9, every break_it argument is ≥ 1e-6 away from an
integer or is the num_iterations clamp.
"""
import ctypes as C

import numpy as np
import pytest

import plane_restatement as R
from m3d import _lib, prep
from m3d.core import Cloud, ptr, stream_handle
from m3d.types import PointCloud

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

CH = prep.PLANE_CHUNK
ERR_RTOL = 1e-12
# the restatement's two-order refit differences (normal, d) on the four scene runs, measured on the
# CPU: n3 (7.5e-16, 6.7e-17), n3_off (1.1e-15, 4.5e-13 at |d| = 771), n4 (4.4e-16, 0), n6
# (2.2e-16, 7.8e-18) — so every tolerance below is its floor: 1e-13 on the normal, 1e-13·max(1, |d|)
# on d (7.7e-11 for n3_off)
REFIT_MEASURED = {"n3": (7.5e-16, 6.7e-17), "n3_off": (1.1e-15, 4.5e-13), "n4": (4.4e-16, 0.0), "n6": (2.2e-16, 7.8e-18)}


def preconditions(r):
    assert all(g >= 1e-9 for g in r.rmse_gaps), r.rmse_gaps
    assert all(clamped or off >= 1e-6 for _, off, clamped in r.break_args), r.break_args


def assert_err(got, ref):
    reached = ref >= 0
    np.testing.assert_array_equal(got[~reached], -1.0)
    np.testing.assert_allclose(got[reached], ref[reached], rtol=ERR_RTOL, atol=0)


def assert_run(P, r, thr, rn, iters, prob, **kw):
    """One device call against the restatement's run r."""
    preconditions(r)
    plane, inl, out = prep.segment_plane(P, thr, rn, iters, prob, with_details=True, **kw)
    np.testing.assert_array_equal(out.counts, r.counts)
    assert (out.best_index, out.best_count, out.evaluated, out.iterations) == \
        (r.best_index, r.best_count, r.evaluated, r.iterations)
    assert out.ransac_plane.tobytes() == r.ransac_plane.tobytes()
    assert inl.dtype == np.int64
    np.testing.assert_array_equal(inl, r.inliers)
    assert_err(out.err, r.err)
    np.testing.assert_allclose(out.best_rmse, r.best_rmse, rtol=ERR_RTOL, atol=0)
    tol_n = max(100 * r.refit_diff[0], 1e-13)
    tol_d = max(100 * r.refit_diff[1], 1e-13 * max(1.0, abs(r.plane[3])))
    print(f"refit: |Δnormal| {np.abs(plane[:3] - r.plane[:3]).max():.3g} (tol {tol_n:.3g}), "
          f"|Δd| {abs(plane[3] - r.plane[3]):.3g} (tol {tol_d:.3g}); two-order {r.refit_diff}")
    assert np.abs(plane[:3] - r.plane[:3]).max() <= tol_n
    assert abs(plane[3] - r.plane[3]) <= tol_d
    return plane, inl, out


# ------------------------------------------------------------------------------- plane_score
SCORE_N = (3, 63, 64, 65, CH - 1, CH, CH + 1, 2 * CH + 7)
SCORE_H = (1, 63, 64, 65, 129)
SCORE_THR = 0.3
_score = {}


def score_inputs():
    """2C + 7 points and 129 planes through the cloud; the smaller cases are prefixes."""
    if not _score:
        rng = np.random.default_rng(21)
        P = rng.standard_normal((2 * CH + 7, 3))
        nrm = rng.standard_normal((129, 3))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        planes = np.column_stack([nrm, rng.uniform(-0.5, 0.5, 129)])
        P.setflags(write=False)
        planes.setflags(write=False)
        _score["in"] = (P, planes)
    return _score["in"]


@pytest.mark.parametrize("n", SCORE_N)
def test_plane_score_form_boundaries(n):
    """Every H of the lane-group boundaries at every n of the chunk boundaries: counts equal, err
    within rtol 1e-12 of the sequential sum, and hypothesis 0's err bits the same for every H."""
    P, planes = score_inputs()
    Pn = P[:n]
    ref = [R.score(pl, Pn, SCORE_THR) for pl in planes]
    rc = np.array([c for c, _ in ref], np.int32)
    re_ = np.array([e for _, e in ref])
    assert 0 < rc.max() and (n < 64 or rc.min() < n)
    cloud = Cloud(Pn)
    first = set()
    for H in SCORE_H:
        cnt, err = prep.plane_score(cloud, planes[:H], SCORE_THR)
        assert cnt.dtype == np.int32 and err.dtype == np.float64 and len(cnt) == len(err) == H
        np.testing.assert_array_equal(cnt, rc[:H])
        np.testing.assert_allclose(err, re_[:H], rtol=ERR_RTOL, atol=0)
        first.add(err[:1].tobytes())
    assert len(first) == 1


def test_plane_score_of_nothing_touches_nothing():
    import torch

    P, planes = score_inputs()
    cloud, empty = Cloud(P[:100]), Cloud(np.zeros((0, 3)))
    ctx = cloud.ctx
    cnt = torch.full((4,), 77, dtype=torch.int32, device="cuda")
    err = torch.full((4,), 77.0, dtype=torch.float64, device="cuda")
    pl = torch.from_numpy(planes[:4].copy()).cuda()
    assert ctx.lib.m3d_plane_score(ctx.h, cloud.h, None, 0, 0.1, ptr(cnt), ptr(err), stream_handle()) == _lib.M3D_OK
    assert ctx.lib.m3d_plane_score(ctx.h, empty.h, ptr(pl), 4, 0.1, ptr(cnt), ptr(err), stream_handle()) == _lib.M3D_OK
    torch.cuda.synchronize()
    assert (cnt.cpu().numpy() == 77).all() and (err.cpu().numpy() == 77.0).all()
    c0, e0 = prep.plane_score(cloud, np.zeros((0, 4)), 0.1)
    assert len(c0) == 0 and len(e0) == 0
    c1, e1 = prep.plane_score(empty, planes[:4], 0.1)
    assert (c1 == 0).all() and (e1 == 0).all()


# ------------------------------------------------------------------------------- segment_plane
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_segment_plane_matches_the_restatement(name):
    n, _, _, rn, iters, seed = R.CONFIGS[name]
    r = R.config_run(name)
    assert r.best_index > 0 and r.records >= 2  # the scan's update path, not only its first hit
    assert name in REFIT_MEASURED
    assert_run(R.config_points(name), r, R.THR, rn, iters, R.PROB, seed=seed)
    if name == "n3":
        assert r.iterations < iters  # the early stop fires here


def outcome_bytes(res):
    plane, inl, o = res
    return (plane.tobytes(), inl.tobytes(), o.ransac_plane.tobytes(), o.best_index, o.best_count,
            np.float64(o.best_rmse).tobytes(), o.evaluated, o.iterations, o.counts.tobytes(), o.err.tobytes())


def test_result_does_not_depend_on_the_batch_and_repeats_bit_for_bit():
    n, _, _, rn, iters, seed = R.CONFIGS["n4"]
    cloud = Cloud(R.config_points("n4"))

    def run(batch):
        return outcome_bytes(prep.segment_plane(cloud, R.THR, rn, iters, R.PROB, seed=seed, batch=batch,
                                                with_details=True))

    base = run(0)
    assert run(0) == base  # two identical calls: identical bytes everywhere
    for batch in (1, 7, 64, iters + 5):
        assert run(batch) == base, batch
    # and with the early stop inside a batch (n3 stops at 104 of 300)
    n, _, _, rn, iters, seed = R.CONFIGS["n3"]
    cloud = Cloud(R.config_points("n3"))
    res = {b: outcome_bytes(prep.segment_plane(cloud, R.THR, rn, iters, R.PROB, seed=seed, batch=b, with_details=True))
           for b in (0, 7, 64, 100, iters + 5)}
    assert len(set(res.values())) == 1


def grid_cloud(nx=8, ny=8):
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return np.column_stack([x.ravel(), y.ravel(), np.zeros(nx * ny)])


def replay(P, samples, thr, prob, rn=3):
    samples = np.asarray(samples)
    r = R.segment_plane(P, thr, rn, len(samples), prob, samples=samples)
    return r, assert_run(P, r, thr, rn, len(samples), prob, samples=samples)


def test_replay_degenerate_samples_are_skipped():
    P = np.vstack([R.scene(1500, 4), [[5.0, 5, 5], [6, 6, 6], [7, 7, 7]]])
    samples = np.array([R.native_sample(2, h, 1500, 3) for h in range(12)])
    samples[1] = [1500, 1501, 1502]  # collinear
    samples[4] = [9, 9, 700]         # a coincident pair
    r, (_, _, out) = replay(P, samples, R.THR, R.PROB)
    assert out.counts[1] == -1 and out.counts[4] == -1 and (np.delete(out.counts, [1, 4]) >= 0).all()
    assert out.evaluated == 10 and out.iterations == 12


def tie_cloud():
    """16 grid points on z = 0, three points a little off it, five far away: with thr 0.01 the
    plane of a grid triple and the plane of the three off points hold the same 19 inliers."""
    off = np.array([[0.5, 0.5, 0.002], [2.5, 0.5, -0.002], [1.5, 2.5, 0.003]])
    far = np.array([[0.0, 0, 5], [1, 1, 6], [2, 0, -5], [3, 3, 7], [1, 2, -6]])
    return np.vstack([grid_cloud(4, 4), off, far])


FLAT, TILTED = [0, 1, 4], [16, 17, 18]


@pytest.mark.parametrize("samples,winner", [([TILTED, FLAT], 1), ([FLAT, TILTED], 0)])
def test_replay_equal_counts_are_decided_by_rmse(samples, winner):
    """The flat plane's err is the off points' 4e-6 + 4e-6 + 9e-6, the tilted plane's is larger
    (it misses the 16 grid points): the flat one replaces the tilted one when it comes second and
    is not replaced when it comes first."""
    P = tie_cloud()
    r, (_, _, out) = replay(P, samples, 0.01, R.PROB)
    assert r.counts.tolist() == [19, 19] and len(r.rmse_gaps) == 1 and r.rmse_gaps[0] > 0.1
    assert out.best_index == winner == int(np.argmin(r.err))
    assert r.records == (2 if winner == 1 else 1)


def test_replay_all_on_plane_stops_by_the_break_rule():
    """f == 1 gives break_it = 0: the loop leaves at the next check, the rows behind read −1 (the
    expected values are the restatement's)."""
    P = grid_cloud()
    samples = np.array([[0, 1, 8], [1, 2, 9], [0, 8, 9], [3, 12, 20], [7, 9, 30]])
    r, (_, _, out) = replay(P, samples, 0.01, R.PROB)
    assert r.break_it == 0.0 and r.best_index == 0 and r.best_count == len(P)
    assert out.iterations == r.iterations < len(samples) and out.evaluated == r.evaluated
    assert (out.counts[r.iterations:] == -1).all() and (out.err[r.iterations:] == -1).all()


def test_low_probability_stops_after_a_handful():
    rng = np.random.default_rng(8)
    n = 3000
    n_pl = int(0.97 * n)
    P = np.vstack([np.column_stack([rng.uniform(-2, 2, n_pl), rng.uniform(-2, 2, n_pl), rng.normal(0, 0.004, n_pl)]),
                   rng.uniform(-3, 3, (n - n_pl, 3))])[rng.permutation(n)]
    r = R.segment_plane(P, R.THR, 3, 1000, 0.5, seed=5)
    assert 0 < r.iterations < 20
    _, _, out = assert_run(P, r, R.THR, 3, 1000, 0.5, seed=5)
    assert (out.counts[r.iterations:] == -1).all()


def test_replay_every_sample_degenerate():
    P = grid_cloud()
    r, (plane, inl, out) = replay(P, [[0, 1, 2], [3, 3, 4], [8, 16, 24]], 0.01, 0.9)
    assert out.best_index == -1 and out.evaluated == 0 and len(inl) == 0
    assert not plane.any() and not out.ransac_plane.any() and (out.counts == -1).all()


def test_three_inliers_and_none():
    P = np.array([[0.1, 0.2, 0.3], [1.3, 0.1, 0.2], [0.2, 1.1, 0.4], [0.5, 0.5, 3.0], [0.2, 0.9, -2.0], [1.0, 1.0, 4.0]])
    r, (plane, inl, _) = replay(P, [[0, 1, 2]], 1e-9, 0.9)
    assert inl.tolist() == [0, 1, 2] and plane.any()  # only the sample itself: the refit is defined
    r, (plane, inl, out) = replay(P, [[0, 1, 2]], 0.0, 0.9)
    assert len(inl) == 0 and not plane.any() and out.best_index == -1 and out.counts.tolist() == [0]


# ------------------------------------------------------------------------------- errors
def c_segment(cloud, thr=0.01, prob=0.9, rn=3, iters=4):
    """m3d_segment_plane called directly (m3d.prep checks the same arguments before it would)."""
    import torch

    ctx = cloud.ctx
    p = _lib.PlaneParams(thr, prob, 0, rn, iters, 0, 0)
    r = _lib.PlaneResult()
    inl = torch.empty((max(cloud.n, 1),), dtype=torch.int32, device="cuda")
    rc = ctx.lib.m3d_segment_plane(ctx.h, cloud.h, C.byref(p), None, C.byref(r), ptr(inl), None, None, stream_handle())
    ctx.check(rc, "segment_plane")
    return r


@pytest.mark.parametrize("kw", [dict(rn=2), dict(rn=33), dict(rn=5), dict(prob=0.0), dict(prob=1.5),
                                dict(thr=float("nan")), dict(thr=-1.0), dict(iters=-1)])
def test_c_entry_point_rejects_invalid_arguments(kw):
    cloud = Cloud(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]))  # rn = 5: n < ransac_n
    assert c_segment(cloud).best_index >= 0
    with pytest.raises(ValueError):
        c_segment(cloud, **kw)


@pytest.mark.parametrize("bad", [-1, 64, 1 << 30])
def test_replay_index_out_of_range_is_an_error_not_a_fault(bad):
    P = grid_cloud()  # n = 64
    samples = np.array([[0, 1, 8], [1, 2, 9], [0, 8, 9]])
    samples[2, 1] = bad
    with pytest.raises(ValueError, match="sample index"):
        prep.segment_plane(P, 0.01, 3, 3, 0.9, samples=samples)
    plane, inl = prep.segment_plane(P, 0.01, 3, 2, 0.9, samples=samples[:2])  # the context still works
    assert len(inl) == 64 and abs(plane[2]) == 1.0


# ------------------------------------------------------------------------------- API
def test_pointcloud_segment_plane_and_select():
    P = R.config_points("n4")
    pc = PointCloud(P)
    plane, inl = pc.segment_plane(R.THR, 3, 100)
    ref_plane, ref_inl = prep.segment_plane(P, R.THR, 3, 100, 0.99999999)
    assert plane.tobytes() == ref_plane.tobytes() and plane.shape == (4,)
    np.testing.assert_array_equal(inl, ref_inl)
    assert len(inl) > 0.5 * len(P)
    rest = pc.select_by_index(inl, invert=True)
    assert len(rest.points) == len(P) - len(inl)


def test_ply_remove_plane():
    from ply.ply import Ply

    P = R.config_points("n4")
    np.random.seed(0)
    a = Ply.from_arrays(P, preprocess=True)
    np.random.seed(0)
    b = Ply.from_arrays(P, preprocess=True, remove_plane=None)
    for x, y in ((a.pcd.points, b.pcd.points), (a.pcd.normals, b.pcd.normals), (a.pcd_down.points, b.pcd_down.points),
                 (a.pcd_down.normals, b.pcd_down.normals), (a.pcd_fpfh.data, b.pcd_fpfh.data)):
        assert x.tobytes() == y.tobytes()
    assert "remove_plane" not in b.stage_ms
    np.random.seed(0)
    c = Ply.from_arrays(P, preprocess=True, remove_plane={"distance_threshold": R.THR, "num_iterations": 200, "seed": 7})
    assert "remove_plane" in c.stage_ms and c.plane_model.shape == (4,)
    assert c.plane_removed == len(P) - len(c.pcd.points) > 0.5 * len(P)
    assert (R.dist(c.plane_ransac, c.pcd.points) >= R.THR).all()
    assert len(c.pcd.normals) == len(c.pcd.points)
