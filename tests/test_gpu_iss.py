"""GPU parity of the ISS keypoints (m3d_compute_iss_keypoints through m3d.prep, m3d.keypoint and Ply)
against the CPU restatement in tests/iss_restatement.py.

Keypoint indices and neighbour counts are compared for equality: both sides decide a neighbour by
the same fp64 expression (dx·dx + dy·dy) + dz·dz < r·r without contraction, and the restatement
proves (``undecided`` empty, asserted here as a precondition and in test_iss_cpu.py) that no
saliency test and no non-maximum comparison of these inputs lies within 1e-12·λ2 of flipping —
ten times the bound of an fp64 implementation's error.  The third eigenvalues are compared within
that 1e-12·λ2.
"""
from functools import lru_cache

import numpy as np
import pytest

import clean_restatement as C
import iss_restatement as R
from m3d import keypoint, prep
from m3d.core import Cloud
from m3d.types import PointCloud

# the shared inputs are read-only arrays; torch only notes that it will not write to them either
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

ALL = [(name, row) for name, rows in R.USED.items() for row in rows]


def run(P, rs=0.0, rn=0.0, g21=0.975, g32=0.975, mn=5):
    return prep.compute_iss_keypoints(P, rs, rn, g21, g32, mn, with_details=True)


def same(a, b):
    (ia, oa), (ib, ob) = a, b
    fields = ("num_keypoints", "num_salient", "num_counted", "salient_radius", "non_max_radius", "resolution")
    return (ia.tobytes() == ib.tobytes() and oa.third_eigen_values.tobytes() == ob.third_eigen_values.tobytes()
            and oa.counts.tobytes() == ob.counts.tobytes()
            and all(getattr(oa, f) == getattr(ob, f) for f in fields))


def assert_outcome(got, ref):
    """(indices, IssOutcome) of the device against an iss_restatement.solve namespace computed with
    the radii the device used."""
    idx, out = got
    assert len(ref.undecided) == 0  # the precondition of comparing decisions for equality
    assert idx.dtype == np.int64
    assert (out.salient_radius, out.non_max_radius) == (ref.salient_radius, ref.non_max_radius)
    np.testing.assert_array_equal(out.counts, ref.counts)
    err = np.abs(out.third_eigen_values - ref.third)
    print("max |third - ref| / e1:", float((err[ref.e1 > 0] / ref.e1[ref.e1 > 0]).max(initial=0.0)))
    decided = ~ref.sal_undecided
    assert (err[decided] <= 1e-12 * ref.e1[decided]).all()
    np.testing.assert_array_equal(idx, ref.keypoints)
    assert (out.num_keypoints, out.num_salient, out.num_counted) == (len(ref.keypoints), ref.num_salient,
                                                                     ref.num_counted)


@lru_cache(maxsize=None)
def reference(name, row, rs, rn):
    """The restatement of a fixture × row; a default row is solved with the radii the device resolved
    (its fixed-order sum and the restatement's sequential one differ in the last bits)."""
    _, _, g21, g32, mn = R.ROWS[row]
    if (rs, rn) == R.ROWS[row][:2]:
        return R.case(name, row)
    return R.solve(R.points(name), rs, rn, g21, g32, mn)


@pytest.mark.parametrize("name,row", ALL)
def test_fixture_row(name, row):
    P = R.points(name)
    params = R.ROWS[row]
    cloud = Cloud(P)
    first = run(cloud, *params)
    out = first[1]
    ref = reference(name, row, out.salient_radius, out.non_max_radius)
    assert_outcome(first, ref)
    np.testing.assert_array_equal(out.counts, C.radius_counts(P, out.salient_radius))
    assert (out.resolution == 0.0) == (row != 0)
    assert same(run(cloud, *params), first)
    prep.remove_radius_outlier(cloud, 3, out.salient_radius)  # the same cell size: the cloud's cached grid
    assert same(run(cloud, *params), first)
    assert same(run(P, *params), first)  # another cloud object, its grids built again
    np.testing.assert_array_equal(prep.compute_iss_keypoints(P, *params), ref.keypoints)


@pytest.mark.parametrize("name", list(R.USED))
def test_default_radii(name):
    P = R.points(name)
    n = len(P)
    res = prep.model_resolution(P)
    seq = R.model_resolution(P)
    print("resolution: device", res, "sequential", seq, "relative difference", abs(res - seq) / seq)
    assert abs(res - seq) <= n * 2.0 ** -53 * seq  # two orders of summing n positive terms
    assert prep.model_resolution(P) == res  # no floating-point atomics: the same bits
    first = run(P)
    out = first[1]
    assert (out.resolution, out.salient_radius, out.non_max_radius) == (res, 6.0 * res, 4.0 * res)
    assert_outcome(first, reference(name, 0, out.salient_radius, out.non_max_radius))
    # one zero radius replaces both
    assert same(run(P, 0.3, 0.0), first)
    assert same(run(P, 0.0, 0.3), first)


@pytest.mark.parametrize("name,row", [("bumpy11", 3), ("A", 2)])
def test_permutation(name, row):
    ref = R.case(name, row)
    perm = np.random.default_rng(9).permutation(len(ref.points))
    idx, out = run(np.ascontiguousarray(ref.points[perm]), *R.ROWS[row])
    np.testing.assert_array_equal(np.sort(perm[idx]), ref.keypoints)
    np.testing.assert_array_equal(out.counts, ref.counts[perm])


def _small(name):
    """→ (points, parameters)."""
    rng = np.random.default_rng(21)
    if name == "one":
        return np.array([[4.0, -2.0, 9.0]]), (0.1, 0.1, 0.975, 0.975, 1)
    if name == "two_coincident":
        return np.tile([[1.25, 2.5, -3.75]], (2, 1)), (0.1, 0.1, 0.975, 0.975, 2)
    if name == "cell200":  # a cell holding 200 coincident points beside a few others
        P = np.concatenate([np.tile([[0.5, 0.5, 0.5]], (200, 1)), rng.uniform(0.0, 1.0, (40, 3))])
        return np.ascontiguousarray(P[rng.permutation(len(P))]), (0.1, 0.1, 0.975, 0.975, 5)
    if name == "n65":  # one wave of candidates plus one, all within the radius of each other
        return np.array([7.0, 7.0, 7.0]) + rng.uniform(-0.01, 0.01, (65, 3)), (0.1, 0.1, 0.975, 0.975, 5)
    if name == "min_neighbors_above":
        return R.points("bumpy11"), (0.1, 0.1, 0.975, 0.975, 1000)
    if name == "min_neighbors_zero":  # three isolated points: count 1, a zero covariance
        far = C.CENTRE + np.array([[30.0, 0.0, 0.0], [0.0, 40.0, 0.0], [0.0, 0.0, -50.0]])
        return np.concatenate([R.points("bumpy11"), far]), (0.15, 0.2, 0.8, 0.1, 0)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one", "two_coincident", "cell200", "n65", "min_neighbors_above",
                                  "min_neighbors_zero"])
def test_small_shapes(name):
    P, params = _small(name)
    P = np.ascontiguousarray(P)
    ref = R.solve(P, *params)
    got = run(P, *params)
    assert np.isfinite(got[1].third_eigen_values).all()
    assert_outcome(got, ref)
    assert same(run(P, *params), got)
    if name in ("one", "two_coincident", "min_neighbors_above"):
        assert len(got[0]) == 0 and (got[1].third_eigen_values == 0.0).all()
    if name in ("one", "two_coincident"):  # a zero resolution: no keypoints, no scan
        idx, out = run(P)
        assert len(idx) == 0 and (out.resolution, out.salient_radius, out.non_max_radius) == (0.0, 0.0, 0.0)
        assert (out.third_eigen_values == 0.0).all() and (out.counts == 0).all()
        assert prep.model_resolution(P) == 0.0
    if name == "cell200":  # the coincident points see only themselves: Eigen's isZero, not 0 / 0
        at = (P == 0.5).all(1)
        assert (ref.counts[at] == 200).all() and (got[1].third_eigen_values[at] == 0.0).all()
    if name == "n65":  # one common set: the same-set rule keeps all of them or none
        assert (ref.counts == 65).all() and len(ref.keypoints) == 65
    if name == "min_neighbors_zero":
        assert (ref.counts[-3:] == 1).all() and got[1].num_counted == len(P) and len(got[0]) > 0


def test_strict_radius_on_the_lattice():
    """Only the counts and the determinism: a lattice is full of true ties between different sets."""
    P = C.points("L7_1")
    for r in (0.25, 0.25 * (1.0 + 2.0 ** -52)):
        got = run(P, r, r)
        np.testing.assert_array_equal(got[1].counts, C.radius_counts(P, r))
        assert same(run(P, r, r), got)
    assert (run(P, 0.25, 0.25)[1].counts == 1).all()  # d² == r² is outside


def test_exact_plane():
    rng = np.random.default_rng(17)
    P = np.column_stack([rng.uniform(-1, 1, (1500, 2)), np.full(1500, 2.5)]) + np.array([3.0, -1.0, 0.0])
    got = run(P, 0.2, 0.15)
    idx, out = got
    assert np.isfinite(out.third_eigen_values).all()
    np.testing.assert_array_equal(out.counts, C.radius_counts(P, 0.2))
    assert (out.third_eigen_values[idx] > 0.0).all()
    # d_z is exactly 0, the covariance block-diagonal, its smallest eigenvalue exactly 0
    assert (out.third_eigen_values == 0.0).all() and len(idx) == 0
    assert same(run(P, 0.2, 0.15), got)


# ------------------------------------------------------------------------------- API
def test_keypoint_module_returns_a_point_cloud():
    ref = R.case("bumpy11", 3)
    rng = np.random.default_rng(2)
    nrm = rng.standard_normal(ref.points.shape)
    cov = rng.standard_normal((len(ref.points), 3, 3))
    pc = PointCloud(ref.points, nrm, cov)
    key = keypoint.compute_iss_keypoints(pc, *R.ROWS[3])
    want = pc.select_by_index(ref.keypoints)
    assert isinstance(key, PointCloud)
    assert key.points.tobytes() == want.points.tobytes() and key.normals.tobytes() == want.normals.tobytes()
    assert key.covariances.tobytes() == want.covariances.tobytes()
    key = keypoint.compute_iss_keypoints(pc, salient_radius=0.1, non_max_radius=0.1, min_neighbors=12)
    assert key.points.tobytes() == want.points.tobytes()


def test_ply_keypoints():
    from ply.ply import Ply

    P = R.points("bumpy11")
    v = 0.03
    np.random.seed(0)
    full = Ply.from_arrays(P, preprocess=True, voxel_size=v)
    np.random.seed(0)
    none = Ply.from_arrays(P, preprocess=True, voxel_size=v, keypoints=None)
    assert "keypoints" not in none.stage_ms and not hasattr(none, "keypoint_indices")
    assert none.pcd_down.points.tobytes() == full.pcd_down.points.tobytes()
    assert none.pcd_down.normals.tobytes() == full.pcd_down.normals.tobytes()
    assert none.pcd_fpfh.data.tobytes() == full.pcd_fpfh.data.tobytes()
    assert none.pcd.normals.tobytes() == full.pcd.normals.tobytes()
    np.random.seed(0)
    key = Ply.from_arrays(P, preprocess=True, voxel_size=v, keypoints={})
    assert "keypoints" in key.stage_ms
    down, _ = prep.voxel_down_sample(P, v)  # the rows before the noise
    idx, out = prep.compute_iss_keypoints(down, with_details=True)
    assert 0 < len(idx) < len(down)
    np.testing.assert_array_equal(key.keypoint_indices, idx)
    assert key.keypoint_radii == (out.salient_radius, out.non_max_radius)
    np.testing.assert_array_equal(key.pcd_fpfh.data, full.pcd_fpfh.data[:, idx])
    np.testing.assert_array_equal(key.pcd_down.normals, full.pcd_down.normals[idx])
    np.random.seed(0)
    noise = 0.05 * np.random.randn(len(idx), 3)
    np.testing.assert_array_equal(key.pcd_down.points, down[idx] + noise)
    assert key.pcd.normals.tobytes() == full.pcd.normals.tobytes()
    # a subset of the parameters
    np.random.seed(0)
    sub = Ply.from_arrays(P, preprocess=True, voxel_size=v, keypoints={"min_neighbors": 8, "gamma_21": 0.9})
    np.testing.assert_array_equal(sub.keypoint_indices,
                                  prep.compute_iss_keypoints(down, gamma_21=0.9, min_neighbors=8))
