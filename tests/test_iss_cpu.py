"""The ISS restatement (tests/iss_restatement.py) checked on the CPU: no decision of any fixture ×
parameter row the GPU tests use lies within rounding of flipping, the same-set rule is exercised,
the extended-precision covariance is the exact one, a far offset changes no keypoint; linalg.h's
``sym3_eigenvalues`` (through its host hook) against LAPACK; and the Python layers reject bad
arguments and answer an empty cloud without a device."""
import ctypes as C

import numpy as np
import pytest

import iss_restatement as R
from m3d import _lib, prep

ALL = [(name, row) for name, rows in R.USED.items() for row in rows]


@pytest.mark.parametrize("name,row", ALL)
def test_no_decision_within_rounding(name, row):
    r = R.case(name, row)
    assert len(r.undecided) == 0
    assert len(r.keypoints) > 0 and (np.diff(r.keypoints) > 0).all()
    assert (r.third[r.keypoints] > 0).all()


def test_default_rows_match_the_prototype_and_exercise_the_same_set_rule():
    got = {name: (len(R.case(name, 0).keypoints), R.case(name, 0).same_set_keypoints) for name in R.USED}
    assert got == {"A": (141, 6), "C": (93, 15), "bumpy11": (97, 3), "bumpy12_far": (69, 5)}
    assert all(same >= 1 for _, same in got.values())


def test_multi_chunk_row_has_counts_beyond_one_wave():
    assert R.case("bumpy11", 1).counts.max() > 64


def test_extended_covariance_is_the_exact_one():
    assert R.extended_ok(), "np.longdouble has no 64-bit mantissa here: the restatement runs on Fraction"
    P = R.points("bumpy11")
    d = P[np.random.default_rng(5).choice(len(P), 40, replace=False)] - P[17]
    ext, exact = R.cov_extended(d), R.cov_fraction(d)
    # 40 products of |d|² ≤ 12 summed with a 64-bit mantissa: each entry is off by at most
    # 40·2⁻⁶⁴·Σ|d|², far below half an fp64 ulp of an entry of that size; the one fp64 rounding of
    # either side then differs by at most one ulp of the largest entry
    assert np.abs(ext - exact).max() <= 2.0 ** -52 * np.abs(exact).max()
    np.testing.assert_array_equal(exact, exact.T)


def test_far_offset_changes_no_keypoint():
    near, far = R.bumpy(12, 2000), R.points("bumpy12_far")
    assert len(np.unique(far, axis=0)) == len(np.unique(near, axis=0)) == len(near)  # still distinct
    a, b = R.solve(near, *R.DEFAULT), R.case("bumpy12_far", 0)
    # the offset rounds the coordinates, so the radii differ in the last digits; the sets must not
    np.testing.assert_array_equal(R.in_radius(near, a.salient_radius), R.in_radius(far, b.salient_radius))
    np.testing.assert_array_equal(R.in_radius(near, a.non_max_radius), R.in_radius(far, b.non_max_radius))
    np.testing.assert_array_equal(a.keypoints, b.keypoints)


# ------------------------------------------------------------------------------- sym3_eigenvalues
def _eig(A):
    lib = _lib.load()
    s = np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]], np.float64)
    out = np.zeros(3)
    P = C.POINTER(C.c_double)
    assert lib.m3d_debug_sym3_eigenvalues_host(s.ctypes.data_as(P), out.ctypes.data_as(P)) == 0
    return out


def _sym3_cases():
    rng = np.random.default_rng(31)
    out = []
    for _ in range(200):  # PSD, eigenvalues spread over up to twelve decades
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = 10.0 ** rng.uniform(-12, 0, 3) * rng.uniform(0.5, 2.0)
        out.append(("psd", (Q * lam) @ Q.T))
    for _ in range(50):
        B = rng.standard_normal((3, 2))
        out.append(("rank2", B @ B.T))
        v = rng.standard_normal(3)
        out.append(("rank1", np.outer(v, v)))
        out.append(("diag", np.diag(rng.uniform(0.0, 3.0, 3))))
    out.append(("zero", np.zeros((3, 3))))
    return out


def test_sym3_eigenvalues_against_lapack():
    for kind, A in _sym3_cases():
        A = 0.5 * (A + A.T)
        ref = np.linalg.eigvalsh(A)
        got = _eig(A)
        assert (np.diff(got) >= 0).all(), kind
        assert np.abs(got - ref).max() <= 4 * 2.0 ** -52 * ref[2], (kind, got, ref)
        if kind == "diag":
            np.testing.assert_array_equal(got, np.sort(np.diag(A)))


def test_sym3_eigenvalues_exact_zero_of_a_block():
    """A neighbourhood exactly in the plane z = const has d_z = 0: the zero row gives λ0 = 0 exactly."""
    rng = np.random.default_rng(32)
    for _ in range(50):
        B = rng.standard_normal((2, 5))
        A = np.zeros((3, 3))
        A[:2, :2] = B @ B.T
        k = rng.integers(3)
        perm = np.roll(np.arange(3), k)
        got = _eig(A[np.ix_(perm, perm)])
        assert got[0] == 0.0 and got[1] > 0.0
        ref = np.linalg.eigvalsh(A)
        assert np.abs(got - ref).max() <= 4 * 2.0 ** -52 * ref[2]


# ------------------------------------------------------------------------------- Python layers
def test_argument_errors_need_no_device():
    P = np.zeros((4, 3))
    for kw in ({"salient_radius": -1.0}, {"non_max_radius": float("nan")}, {"salient_radius": float("inf")},
               {"gamma_21": float("nan")}, {"gamma_32": float("inf")}, {"min_neighbors": -1}):
        with pytest.raises(ValueError):
            prep.compute_iss_keypoints(P, **kw)
    with pytest.raises(ValueError):
        prep.model_resolution(np.zeros(3))


def test_empty_cloud_needs_no_device():
    idx = prep.compute_iss_keypoints(np.zeros((0, 3)))
    assert idx.dtype == np.int64 and idx.shape == (0,)
    idx, out = prep.compute_iss_keypoints(np.zeros((0, 3)), 0.1, 0.2, with_details=True)
    assert idx.shape == (0,) and (out.num_keypoints, out.num_salient, out.num_counted) == (0, 0, 0)
    assert (out.salient_radius, out.non_max_radius, out.resolution) == (0.1, 0.2, 0.0)
    assert out.third_eigen_values.shape == (0,) and out.counts.dtype == np.int32
    assert prep.model_resolution(np.zeros((0, 3))) == 0.0
    from m3d import keypoint
    from m3d.types import PointCloud

    assert len(keypoint.compute_iss_keypoints(PointCloud()).points) == 0


def test_ply_rejects_unknown_keypoint_keys(tmp_path):
    from m3d import plyio
    from ply.ply import Ply

    P = np.random.default_rng(0).uniform(0, 1, (20, 3))
    with pytest.raises(ValueError, match="keypoints"):
        Ply.from_arrays(P, preprocess=True, voxel_size=0.1, keypoints={"bogus": 1})
    path = tmp_path / "c.ply"
    plyio.write_ply(path, P, binary=True)
    with pytest.raises(ValueError, match="keypoints"):
        Ply(path, 0.1, keypoints={"bogus": 1})
