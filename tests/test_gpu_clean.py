"""GPU parity of the outlier-removal path (m3d_knn_search, m3d_remove_statistical_outlier,
m3d_remove_radius_outlier through m3d.prep, PointCloud and Ply) against the CPU restatement in
tests/clean_restatement.py.

What is compared how.  Lists: indices equal, d² bit-equal — both sides evaluate
(dx·dx + dy·dy) + dz·dz in fp64 without contraction and order by (d², index).  Mean distances:
rtol 1e-14; they are expected bit-equal (the same sequential sum of correctly rounded square roots
and one division), the tolerance only allows for a square root that is not correctly rounded in one
of the two libraries.  mean / std_dev / threshold: rtol 1e-12 — the device adds the same
non-negative terms in a fixed tree (error ≤ ~log₂n·2⁻⁵³), the restatement sequentially (≤ n·2⁻⁵³ in
the worst case, ~√n·2⁻⁵³ ≈ 4e-14 for rounding errors of mixed sign at n = 1.1e5).  Kept indices:
equal, after asserting on the restatement that no mean distance lies within the stated relative margin of the
threshold (so the two summation orders cannot disagree about any point).
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import clean_restatement as R
from m3d import prep
from m3d.core import Cloud, context
from m3d.types import PointCloud

# the shared inputs are read-only arrays; torch only notes that it will not write to them either
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

MARGIN = 6e-3      # the table cases (tests/test_clean_cpu.py asserts it for each)
MARGIN_MIN = 1e-9  # the exclusion band of the mask comparison; no point may lie inside it


def assert_lists(P, k, ref):
    idx, d2, cnt = prep.knn_search(P, k)
    ridx, rd2, rcnt = ref
    np.testing.assert_array_equal(cnt, rcnt)
    assert (cnt == min(k, len(P))).all()
    np.testing.assert_array_equal(idx, ridx)
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    assert d2.tobytes() == rd2.tobytes()


@pytest.mark.parametrize("k", [1, 20, 64, 65, 128, 200])
def test_knn_search_across_the_kernel_forms(k):
    """k ≤ 64, ≤ 128 and ≤ 256 are three instantiations of the search kernel."""
    idx, d2, cnt = R.knn_case("A", 200)  # sorted once: the lists for a smaller k are its prefixes
    assert_lists(R.points("A"), k, (idx[:, :k], np.ascontiguousarray(d2[:, :k]), cnt.clip(max=k)))


@pytest.mark.parametrize("name,k", [("F", 20), ("G", 2), ("L7_1", 7), ("L7_1", 10), ("M", 6), ("E", 20)])
def test_knn_search_edge_clouds(name, k):
    P = R.points(name)
    ref = R.knn_case(name, k)
    assert_lists(P, k, ref)
    if name == "F":  # n < k: −1 / inf padding past the 12 points
        assert (ref[0][:, 12:] == -1).all() and np.isinf(ref[1][:, 12:]).all()
    if name == "G":  # coincident twins: the lower index first, not necessarily the point itself
        assert (ref[0][:, 0] != np.arange(len(P))).any()


def check_stats(st, ref):
    assert (st.kept, st.valid) == (len(ref.indices), ref.valid)
    for got, want in ((st.mean, ref.mean), (st.std_dev, ref.std_dev), (st.threshold, ref.threshold)):
        if np.isnan(want):
            assert np.isnan(got)
        else:
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_statistical_filter(name):
    _, k, ratio, removed = R.CASES[name]
    P = R.points(name)
    avg, ref = R.stat_case(name)
    assert ref.margin >= MARGIN and len(P) - len(ref.indices) == removed
    ind, st = prep.remove_statistical_outlier(P, k, ratio, with_mean_distance=True)
    print(name, "avg max rel diff", np.max(np.abs(st.mean_distance - avg) / np.where(avg > 0, avg, 1.0)),
          "bit-equal", st.mean_distance.tobytes() == avg.tobytes(), st.mean, st.std_dev, st.threshold)
    np.testing.assert_allclose(st.mean_distance, avg, rtol=1e-14, atol=0.0)
    check_stats(st, ref)
    assert ind.dtype == np.int32
    np.testing.assert_array_equal(ind, ref.indices)
    ind2, st2 = prep.remove_statistical_outlier(P, k, ratio)  # no mean distances asked for
    np.testing.assert_array_equal(ind2, ind)
    assert st2.mean_distance is None and st2.threshold == st.threshold


def test_statistical_filter_small_clouds():
    one = np.array([[1.0, 2.0, 3.0]])
    ind, st = prep.remove_statistical_outlier(one, 5, 2.0, with_mean_distance=True)
    assert len(ind) == 0 and (st.kept, st.valid) == (0, 1)
    assert np.isnan(st.threshold) and np.isnan(st.std_dev) and st.mean == 0.0
    assert st.mean_distance.tolist() == [0.0]
    P = R.points("D")[:50]
    ind, st = prep.remove_statistical_outlier(P, 1, 2.0)  # one neighbour: the point itself
    assert len(ind) == 0 and st.threshold == 0.0 and st.valid == 50
    idx, d2, cnt = prep.knn_search(one, 3)
    assert idx.tolist() == [[0, -1, -1]] and d2[0, 0] == 0.0 and np.isinf(d2[0, 1:]).all() and cnt.tolist() == [1]


RADIUS_CASES = [("A", 0.08, 6), ("A", 0.15, 16), ("L7_1", 0.25, 1), ("L7_1", 0.25 * (1 + 2.0 ** -40), 5)]


@pytest.mark.parametrize("name,radius,nb", RADIUS_CASES)
def test_radius_filter(name, radius, nb):
    P = R.points(name)
    want = R.radius_counts(P, radius)
    keep = np.flatnonzero(want > nb).astype(np.int32)
    ind, cnt = prep.remove_radius_outlier(P, nb, radius, with_counts=True)
    np.testing.assert_array_equal(cnt, want)
    np.testing.assert_array_equal(ind, keep)
    early = prep.remove_radius_outlier(P, nb, radius)  # counts stop once they exceed nb
    assert early.dtype == np.int32
    np.testing.assert_array_equal(early, keep)
    if name == "L7_1" and radius == 0.25:
        assert (cnt == 1).all() and len(ind) == 0  # strict: d² == r² is outside
    assert 0 < len(keep) < len(P) or radius == 0.25


def _early_leave_cloud(name):
    """tests/test_gpu_dbscan.py's shapes of the same names."""
    rng = np.random.default_rng(21)
    if name == "n65":  # one wave of candidates plus one, all within the radius of each other
        return np.ascontiguousarray(np.array([7.0, 7.0, 7.0]) + rng.uniform(-0.01, 0.01, (65, 3)))
    P = np.concatenate([np.tile([[0.5, 0.5, 0.5]], (200, 1)), rng.uniform(0.0, 1.0, (40, 3))])
    return np.ascontiguousarray(P[rng.permutation(len(P))])  # a cell holding 200 coincident points


EARLY_CLOUDS = {name: _early_leave_cloud(name) for name in ("cell200", "n65")}
EARLY_COUNTS = {name: R.radius_counts(P, 0.1) for name, P in EARLY_CLOUDS.items()}


@pytest.mark.parametrize("nb", [0, 63, 64, 65, 127, 128, 199, 200])
@pytest.mark.parametrize("name", ["cell200", "n65"])
def test_radius_filter_early_leave_across_chunks(name, nb):
    """The count without with_counts stops once it exceeds nb: in the first, second, third and last
    64-candidate chunk of the dense cell's row, and never.  nb = 0 is no filter parameter (Open3D
    and the C ABI refuse nb_points < 1): the kernel meets it as DBSCAN's core pass at min_points = 1,
    so that case compares there — the full counts, and every point core with and without them."""
    P, want = EARLY_CLOUDS[name], EARLY_COUNTS[name]
    assert want.max() >= (200 if name == "cell200" else 65)
    keep = np.flatnonzero(want > nb).astype(np.int32)
    if nb == 0:
        with pytest.raises(ValueError):
            prep.remove_radius_outlier(P, 0, 0.1)
        labels, out = prep.cluster_dbscan(P, 0.1, 1, with_details=True)
        np.testing.assert_array_equal(out.counts, want)
        assert out.num_core == len(keep) == len(P) and out.num_noise == 0 and (labels >= 0).all()
        np.testing.assert_array_equal(prep.cluster_dbscan(P, 0.1, 1), labels)  # the count stops at 1
        return
    ind, cnt = prep.remove_radius_outlier(P, nb, 0.1, with_counts=True)
    np.testing.assert_array_equal(cnt, want)
    np.testing.assert_array_equal(ind, keep)
    np.testing.assert_array_equal(prep.remove_radius_outlier(P, nb, 0.1), keep)


def test_determinism_stale_scratch_and_cached_grids():
    P = R.points("A")
    c = Cloud(P)
    lib = context().lib

    def neighbours():
        idx, d2, cnt = prep.hybrid_search(c, 0.2, 30)
        return idx.tobytes(), d2.tobytes(), cnt.tobytes(), prep.estimate_normals(c, 0.2, 30).tobytes()

    def filters():
        ind, st = prep.remove_statistical_outlier(c, 20, 2.0, with_mean_distance=True)
        rind, rcnt = prep.remove_radius_outlier(c, 6, 0.08, with_counts=True)
        return (ind.tobytes(), st.mean_distance.tobytes(), np.array([st.mean, st.std_dev, st.threshold]).tobytes(),
                (st.kept, st.valid), rind.tobytes(), rcnt.tobytes(), prep.remove_radius_outlier(c, 6, 0.08).tobytes())

    before = neighbours()
    first = filters()
    assert filters() == first
    assert lib.m3d_debug_block_cache_fill(0xFF) >= 0  # stale bytes in every idle cached block
    assert filters() == first
    assert neighbours() == before  # the cloud's cached grids are still the ones the search needs
    fresh = Cloud(P)
    assert neighbours() == tuple(
        x.tobytes() for x in (*prep.hybrid_search(fresh, 0.2, 30), prep.estimate_normals(fresh, 0.2, 30)))


def against_kd_tree(P):
    dist, _ = cKDTree(P).query(P, k=20)
    acc = np.zeros(len(P))
    for s in range(20):
        acc = acc + dist[:, s]
    avg = acc / 20.0
    ref = R.statistics(avg, 2.0)
    print("margin", ref.margin, "removed", len(P) - len(ref.indices))
    assert ref.margin > MARGIN_MIN
    ind, st = prep.remove_statistical_outlier(P, 20, 2.0, with_mean_distance=True)
    np.testing.assert_allclose(st.mean_distance, avg, rtol=1e-12, atol=0.0)
    check_stats(st, ref)
    np.testing.assert_array_equal(ind, ref.indices)
    return ref


def test_mid_size_cloud_against_the_kd_tree():
    """More than one block and a ladder of several levels: 100k shell points and 500 strays."""
    against_kd_tree(R.shell(9, 100000, 500))


def test_far_strays_with_more_than_one_block():
    """Two points 10³ radii away stretch the bounds: the call's grids span a cut box instead, the
    far points share its edge cells, and the result is the k-d tree's."""
    P = R.shell(11, 20000, 100, far=1)
    ref = against_kd_tree(P)
    far = np.flatnonzero(np.abs(P).max(1) >= 1e3)
    assert len(far) == 2 and not np.isin(far, ref.indices).any()


def test_python_surface():
    from ply import Ply

    P = R.points("A")
    N = np.random.default_rng(3).normal(size=P.shape)
    _, ref = R.stat_case("A")
    pc = PointCloud(P, N)
    out, ind = pc.remove_statistical_outlier(20, 2.0)
    np.testing.assert_array_equal(ind, ref.indices)
    np.testing.assert_array_equal(out.points, P[ind])
    np.testing.assert_array_equal(out.normals, N[ind])
    keep = np.flatnonzero(R.radius_counts(P, 0.08) > 6)
    out, ind = pc.remove_radius_outlier(6, 0.08)
    np.testing.assert_array_equal(ind, keep)
    np.testing.assert_array_equal(out.points, P[keep])
    np.testing.assert_array_equal(out.normals, N[keep])
    assert len(pc.points) == len(P)  # the filters return a new cloud

    np.random.seed(11)
    cleaned = Ply.from_arrays(P, preprocess=True, remove_outliers={"nb_neighbors": 20, "std_ratio": 2.0})
    assert len(cleaned.pcd.points) == 3017 and cleaned.stage_ms["remove_outliers"] > 0
    np.testing.assert_array_equal(cleaned.pcd.points, P[ref.indices])
    by_radius = Ply.from_arrays(P, preprocess=True, remove_outliers={"nb_points": 6, "radius": 0.08})
    assert len(by_radius.pcd.points) == len(keep)
    with pytest.raises(ValueError):
        Ply.from_arrays(P, preprocess=True, remove_outliers={"nb_neighbors": 20})

    def plain():
        np.random.seed(11)
        p = Ply.from_arrays(P, preprocess=True)
        assert "remove_outliers" not in p.stage_ms
        return tuple(a.tobytes() for a in (p.pcd.points, p.pcd.normals, p.pcd_down.points, p.pcd_down.normals,
                                           p.pcd_fpfh.data))

    assert plain() == plain()
