"""The plane-segmentation restatement (tests/plane_restatement.py) against closed forms, the ctypes
mirror of the new C-ABI section against include/m3d.h, and the argument errors m3d.prep raises
before any device call.  No GPU."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import plane_restatement as R
from m3d import _lib, prep

ROOT = Path(__file__).resolve().parents[1]


def grid_cloud(nx=8, ny=8):
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    return np.column_stack([x.ravel(), y.ravel(), np.zeros(nx * ny)])


def test_integer_grid_on_z0_is_exact_and_stops_at_the_next_check():
    """Every point on the plane: the first non-degenerate sample gives (0, 0, ±1, ∓0) exactly,
    count = n, rmse 0, f = 1 → break_it = 0; evaluated is then 1 > 0, so the check in front of the
    next hypothesis stops the loop (the contract's order: the check comes before the evaluation)."""
    P = grid_cloud()
    r = R.segment_plane(P, 0.01, 3, 50, 0.99999999, seed=3)
    assert r.best_index >= 0
    assert (r.counts[: r.best_index] == -1).all()  # only collinear samples before it
    a, b, c, d = r.ransac_plane
    assert a == 0.0 and b == 0.0 and abs(c) == 1.0 and d == 0.0
    assert r.best_count == len(P) and r.best_rmse == 0.0 and r.break_it == 0.0
    assert r.break_args == [(0.0, 0.0, True)]
    assert r.evaluated == 1 and r.iterations == r.best_index + 1
    assert (r.counts[r.iterations:] == -1).all()
    np.testing.assert_array_equal(r.inliers, np.arange(len(P)))
    assert abs(r.plane[2]) == 1.0 and (r.plane[[0, 1, 3]] == 0.0).all()


def test_collinear_and_coincident_triples_are_skipped_without_counting():
    P = grid_cloud()
    samples = np.array([[0, 1, 2], [5, 5, 9], [0, 1, 8]])  # collinear, coincident, a triangle
    assert not R.plane_of_sample(P, samples[0]).any() and not R.plane_of_sample(P, samples[1]).any()
    r = R.segment_plane(P, 0.01, 3, 3, 0.99999999, samples=samples)
    assert r.counts.tolist() == [-1, -1, len(P)]
    assert r.evaluated == 1 and r.best_index == 2 and r.iterations == 3


def test_every_sample_degenerate_gives_the_zero_plane():
    P = grid_cloud()
    r = R.segment_plane(P, 0.01, 3, 2, 0.5, samples=np.array([[0, 1, 2], [8, 16, 24]]))
    assert r.best_index == -1 and r.evaluated == 0 and len(r.inliers) == 0
    assert not r.plane.any() and not r.ransac_plane.any()


def test_plane_from_points_matches_the_smallest_singular_vector():
    """GetPlaneFromPoints is the regression plane along the dominant axis, not the total least
    squares one: on out-of-plane noise σ over an extent L the two normals differ by O(σ²/L²)
    (the other two eigenvector terms of the covariance's adjugate).  The tolerance asked for —
    100 × the fit's own two-order difference, floor 1e-12 — therefore fixes how noisy the patch
    may be: σ = 1e-7 on a 4 × 4 patch (σ²/L² ≈ 6e-16, eight orders above the coordinates'
    rounding), in a general orientation."""
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    for m in (4, 6, 32, 2000):
        flat = np.column_stack([rng.uniform(-2, 2, m), rng.uniform(-2, 2, m), rng.normal(0, 1e-7, m)])
        P = flat @ Q.T + np.array([0.3, -0.2, 0.5])
        seq, pw = R.plane_from_points(P, "seq"), R.plane_from_points(P, "pairwise")
        tol = max(100 * np.abs(seq - pw).max(), 1e-12)
        cen = P.mean(0)
        nrm = np.linalg.svd(P - cen)[2][-1]
        if nrm @ seq[:3] < 0:
            nrm = -nrm
        assert abs(np.linalg.norm(seq[:3]) - 1) < 1e-15
        assert np.abs(seq[:3] - nrm).max() <= tol, (m, np.abs(seq[:3] - nrm).max(), tol)
        assert abs(seq[3] + nrm @ cen) <= tol


def test_triangle_plane_closed_form():
    pl = R.plane_from_triangle([1, 0, 0], [0, 1, 0], [0, 0, 1])
    np.testing.assert_allclose(pl, np.array([1, 1, 1, -1]) / np.sqrt(3), rtol=0, atol=2e-16)
    assert not R.plane_from_points(np.zeros((2, 3))).any()  # fewer than three points


def test_sampler_indices_are_distinct_in_range_and_pinned():
    for n, m in ((3, 3), (7, 6), (32, 32), (1000, 6), (4097, 4)):
        for h in range(50):
            s = R.native_sample(7, h, n, m)
            assert len(s) == m == len(set(s)) and min(s) >= 0 and max(s) < n
    assert R.native_sample(7, 5, 1000, 6) == [160, 717, 204, 209, 879, 610]
    # ransac_n = 3 is the registration sampler (oracle/ransac_oracle.py restates ransac.hip's)
    import ransac_oracle as O

    tri = O.native_triples(9, 0, 40, 5000)
    assert [R.native_sample(9, h, 5000, 3) for h in range(40)] == np.asarray(tri).tolist()


def test_probability_one_never_stops_early():
    P = R.scene(600, 3)
    r = R.segment_plane(P, 0.012, 3, 40, 1.0, seed=1)
    assert r.iterations == 40 and r.break_it == 40.0
    assert all(clamped and arg == 40.0 for arg, _, clamped in r.break_args)
    assert r.evaluated == int((r.counts >= 0).sum()) > 30


def test_no_iterations():
    r = R.segment_plane(R.scene(100, 1), 0.012, 3, 0, 0.9)
    assert r.best_index == -1 and r.iterations == 0 and r.evaluated == 0
    assert len(r.inliers) == 0 and not r.plane.any() and len(r.counts) == 0


def test_scene_runs_meet_the_gpu_tests_preconditions():
    """What tests/test_gpu_plane.py requires of its inputs, on the restatement alone."""
    for name in R.CONFIGS:
        r = R.config_run(name)
        assert r.best_index > 0 and r.records >= 2, name
        assert all(g >= 1e-9 for g in r.rmse_gaps), (name, r.rmse_gaps)
        assert all(clamped or off >= 1e-6 for _, off, clamped in r.break_args), (name, r.break_args)
    r = R.config_run("n3")
    assert r.iterations == 104  # the early stop fires
    assert R.config_run("n3_off").refit_diff[1] < 1e-12


# ------------------------------------------------------------------------------- header ↔ ctypes
SIZES = {"double": 8, "uint64_t": 8, "int64_t": 8, "int32_t": 4}


def header_struct(name):
    """[(type, field, array length)] of `typedef struct { … } name;` in include/m3d.h."""
    text = (ROOT / "include" / "m3d.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        typ, rest = decl.split(None, 1)
        for f in rest.split(","):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", f.strip())
            out.append((typ, m.group(1), int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("cname,mirror", [("m3d_plane_params", _lib.PlaneParams), ("m3d_plane_result", _lib.PlaneResult)])
def test_struct_mirrors_match_the_header(cname, mirror):
    fields = header_struct(cname)
    assert [f for _, f, _ in fields] == [f for f, _ in mirror._fields_]
    off = 0
    for (typ, fname, count), (_, ctype) in zip(fields, mirror._fields_):
        size = SIZES[typ]
        off = (off + size - 1) // size * size
        assert getattr(mirror, fname).offset == off, fname
        assert C.sizeof(ctype) == size * count, fname
        off += size * count
    assert C.sizeof(mirror) == (off + 7) // 8 * 8


def test_new_symbols_are_declared_exported_and_bound():
    text = (ROOT / "include" / "m3d.h").read_text()
    lib = _lib.load()
    for s in ("m3d_segment_plane", "m3d_plane_score", "m3d_plane_chunk"):
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["m3d_segment_plane"][1]) == 9
    assert len(_lib.SIGNATURES["m3d_plane_score"][1]) == 8
    assert lib.m3d_plane_chunk() == _lib.PLANE_CHUNK == prep.PLANE_CHUNK
    assert lib.m3d_abi_version() == 13


# ------------------------------------------------------------------------------- Python errors
@pytest.mark.parametrize("kw,msg", [
    (dict(probability=0.0), "Probability must be > 0 and <= 1.0"),
    (dict(probability=1.5), "Probability must be > 0 and <= 1.0"),
    (dict(probability=float("nan")), "Probability must be > 0 and <= 1.0"),
    (dict(ransac_n=2), "ransac_n should be set to higher than or equal to 3"),
    (dict(ransac_n=33), "ransac_n <= 32"),
    (dict(num_iterations=-1), "num_iterations"),
    (dict(distance_threshold=float("nan")), "distance_threshold"),
    (dict(distance_threshold=float("inf")), "distance_threshold"),
    (dict(distance_threshold=-0.1), "distance_threshold"),
    (dict(ransac_n=5), "at least 'ransac_n' points"),  # four points
    (dict(samples=np.zeros((3, 3), int), num_iterations=4), "samples"),
])
def test_argument_errors_are_raised_before_any_device_call(kw, msg):
    P = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    args = dict(distance_threshold=0.01, ransac_n=3, num_iterations=10, probability=0.9)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        prep.segment_plane(P, **args)


def test_ply_remove_plane_rejects_unknown_keys():
    from ply.ply import Ply

    P = R.scene(50, 2)
    for bad in ({"threshold": 0.01}, {"distance_threshold": 0.01, "iterations": 5}, {}):
        with pytest.raises(ValueError, match="remove_plane"):
            Ply.from_arrays(P, preprocess=True, remove_plane=bad)
