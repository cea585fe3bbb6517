"""Colored ICP without a GPU: the numpy restatement (tests/colored_restatement.py) against closed
forms, the capability it stands for (the ridge-slide fixture), and the host side of the feature
(PLY colours, PointCloud colours).

Slide fixture.  The ridge surface z = 0.02·sin 2x runs along y, so no geometric residual sees the
source's y offset of −0.03.  Conditions: with λ = 0.968 the joint estimator ends within 1/50 of
that offset of the truth; with λ = 1 (geometry only; JᵀJ is singular along the slide, hence the
least-squares solve) at least 90 % of it remains.
"""
import numpy as np
import pytest

import colored_restatement as CI
import icp_oracle as I
from m3d import plyio
from m3d.plyio import read_point_cloud  # noqa: F401  (the feature's host side: absent before it)
from m3d.types import PointCloud


# ------------------------------------------------------------------------------------ gradients
def plane_cloud(n, seed):
    """Points on the exact plane through the origin spanned by two orthonormal fp64 vectors whose
    products are exact enough: u = (1, 0, 0), v = (0, 0.6, 0.8), normal (0, −0.8, 0.6)."""
    rng = np.random.default_rng(seed)
    ab = rng.uniform(-1, 1, (n, 2))
    u, v = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8])
    pts = ab[:, :1] * u + ab[:, 1:] * v
    return pts, np.tile([0.0, -0.8, 0.6], (n, 1))


def test_gradient_of_a_linear_field_on_a_plane():
    pts, nrm = plane_cloud(600, 2)
    a, c = np.array([0.21, -0.13, 0.17]), 0.4
    inten = pts @ a + c
    col = np.stack([inten + 0.05, inten - 0.05, inten], axis=1)  # r ≠ g ≠ b, mean = I up to rounding
    g = CI.color_gradients(pts, nrm, col, 0.3)
    n = nrm[0]
    tangential = a - (a @ n) * n
    lens = np.array([len(x) for x in CI.hybrid_lists(pts, 0.3)])
    assert (lens == CI.MAX_NN).mean() > 0.8 and lens.min() >= 4
    print("linear field: worst |g - tangential part|", np.abs(g - tangential).max())
    assert np.abs(g - tangential).max() <= 1e-12
    gl = CI.color_gradients(pts, nrm, col, 0.3, dtype=np.longdouble)
    assert gl.dtype == np.longdouble and np.abs(gl - tangential).max() <= 1e-12


def test_uniform_colours_give_exactly_zero():
    f = CI.gradient_case(257, uniform=True)
    assert max(len(x) for x in f["lists"]) == CI.MAX_NN
    np.testing.assert_array_equal(f["g64"], np.zeros((257, 3)))
    np.testing.assert_array_equal(f["gld"], np.zeros((257, 3)))


def test_fewer_than_four_neighbours_give_zero():
    for n in (1, 3):
        np.testing.assert_array_equal(CI.gradient_case(n)["g64"], np.zeros((n, 3)))
    f = CI.gradient_case(2000)
    lens = np.array([len(x) for x in f["lists"]])
    few = lens < 4
    assert few.sum() == 4 and (lens == CI.MAX_NN).sum() >= 1900  # the stragglers; most lists at the cap
    np.testing.assert_array_equal(f["g64"][few], np.zeros((4, 3)))
    assert np.all(np.abs(f["g64"][~few]).sum(axis=1) > 0)
    # the fp64 restatement against the longdouble one: rounding only
    assert np.abs(f["g64"] - f["gld"]).max() <= 1e-12 * np.abs(f["gld"]).max()


def test_hybrid_list_contract():
    """strict d² < r², the query included, ordered by (d², index), cut at max_nn."""
    pts = np.array([[0.0, 0, 0], [1.0, 0, 0], [0.0, 1.0, 0], [0.0, 0, 0], [2.0, 0, 0]])
    lists = CI.hybrid_lists(pts, 1.0, 30)
    np.testing.assert_array_equal(lists[0], [0, 3])      # d = 1 is outside; the duplicate by index
    np.testing.assert_array_equal(lists[3], [0, 3])      # … so a duplicate's entry 0 is not itself
    np.testing.assert_array_equal(CI.hybrid_lists(pts, 1.5, 2)[1], [1, 0])


# ------------------------------------------------------------------------------------ terms
def test_terms_reduce_to_point_to_plane_at_lambda_one():
    import robust_restatement as R

    f = CI.eval_case(257)
    sums, scale = CI.colored_terms(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], f["corr"], lam=1.0)
    ref, _ = R.robust_plane_sums(f["pcd"], f["tgt"], f["tn"], f["corr"])
    assert np.all(np.abs(sums - ref) <= 1e-13 * np.maximum(scale, 1e-300))
    assert sums[28] == len(f["corr"]) and np.all(scale >= np.abs(sums))


def test_photometric_row_is_the_derivative_of_its_residual():
    """J1 is ∂r1/∂ξ at ξ = 0 for the twist ξ = (ω, t) moving vs to vs + ω × vs + t."""
    f = CI.eval_case(257)
    corr = f["corr"][:40]
    r, J, _ = CI.colored_rows(f["pcd"], f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], corr)
    h = 1e-6
    for a in range(6):
        xi = np.zeros(6)
        xi[a] = h
        moved = f["pcd"] + np.cross(xi[:3], f["pcd"]) + xi[3:]
        rp = CI.colored_rows(moved, f["si"], f["tgt"], f["tn"], f["ti"], f["grad"], corr)[0]
        np.testing.assert_allclose((rp - r) / h, J[:, :, a], rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------ the slide
def test_slide_fixture_colour_locks_what_geometry_cannot():
    f = CI.slide_pair()
    out = CI.slide_run()
    err = out["transformation"][:3, 3] + CI.SLIDE_SHIFT
    geo = CI.slide_run(lam=1.0, solve="lstsq")
    left = geo["transformation"][:3, 3] + CI.SLIDE_SHIFT
    print(f"slide: lambda 0.968 ends {err} from the truth after {out['iterations']} iterations "
          f"(fitness {out['fitness']:.3f}); lambda 1 leaves {left}")
    assert abs(err[1]) <= abs(CI.SLIDE_SHIFT[1]) / 50
    assert abs(left[1]) >= 0.9 * abs(CI.SLIDE_SHIFT[1])
    assert out["fitness"] > 0.9
    lens = np.array([len(x) for x in CI.hybrid_lists(f["tgt"], 2 * CI.SLIDE_RADIUS)])
    assert (lens == CI.MAX_NN).mean() > 0.95


def test_loop_fixture_has_no_near_ties():
    """The GPU test compares correspondences at every evaluation: the loop fixture must not hold a
    source whose two nearest targets are closer in d² than rounding could swap."""
    from scipy.spatial import cKDTree

    case = CI.loop_case("perturbed")
    tree = cKDTree(case["tgt"])
    assert case["ref"]["converged"] and 2 <= case["ref"]["iterations"] < 30
    for pcd, j in case["evals"]:
        _, jj = tree.query(pcd, k=2)
        d0, d1 = I.sq_dist(pcd, case["tgt"][jj[:, 0]]), I.sq_dist(pcd, case["tgt"][jj[:, 1]])
        assert np.all(np.abs(d1 - d0) > 1e-12)
        assert 0 < (j >= 0).sum() < len(j)


# ------------------------------------------------------------------------------------ host side
@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_ply_uchar_colours_round_trip(tmp_path, binary, with_normals):
    rng = np.random.default_rng(3)
    pts = rng.standard_normal((50, 3))
    nrm = rng.standard_normal((50, 3)) if with_normals else None
    u8 = rng.integers(0, 256, (50, 3))
    u8[0], u8[1] = 0, 255
    p = tmp_path / "c.ply"
    plyio.write_ply(p, pts, nrm, binary=binary, colors=u8 / 255.0)
    pc = plyio.read_point_cloud(p)
    np.testing.assert_array_equal(pc.points, pts)
    np.testing.assert_array_equal(pc.colors, u8 / 255.0)
    assert pc.has_colors() and pc.has_normals() == with_normals
    if with_normals:
        np.testing.assert_array_equal(pc.normals, nrm)
    got = plyio.read_ply(p)
    assert len(got) == 2  # read_ply keeps its two-value return
    np.testing.assert_array_equal(got[0], pts)


def test_ply_colour_rounding_and_clipping(tmp_path):
    p = tmp_path / "r.ply"
    col = np.array([[-0.2, 0.5, 1.3], [0.499 / 255, 0.501 / 255, 254.6 / 255]])
    plyio.write_ply(p, np.zeros((2, 3)), colors=col)
    np.testing.assert_array_equal(plyio.read_point_cloud(p).colors * 255, [[0, 128, 255], [0, 1, 255]])


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
@pytest.mark.parametrize("ctype", ["uchar", "float", "double"])
def test_ply_colour_types_and_endianness(tmp_path, fmt, ctype):
    rng = np.random.default_rng(5)
    n = 20
    pts = rng.standard_normal((n, 3))
    if ctype == "uchar":
        raw = rng.integers(0, 256, (n, 3)).astype(np.uint8)
        want = raw / 255.0
    elif ctype == "float":
        raw = rng.uniform(0, 1, (n, 3)).astype(np.float32)
        want = raw.astype(np.float64)
    else:
        raw = rng.uniform(0, 1, (n, 3))
        want = raw
    head = ["ply", f"format {fmt} 1.0", f"element vertex {n}", "property double x", "property double y",
            "property double z"] + [f"property {ctype} {c}" for c in ("red", "green", "blue")] + ["end_header"]
    p = tmp_path / "t.ply"
    with open(p, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        if fmt == "ascii":
            for a, c in zip(pts.tolist(), raw.tolist()):
                f.write((" ".join(map(repr, a)) + " " + " ".join(map(repr, c)) + "\n").encode("ascii"))
        else:
            e = "<" if fmt == "binary_little_endian" else ">"
            np_t = {"uchar": "u1", "float": e + "f4", "double": e + "f8"}[ctype]
            rec = np.empty(n, np.dtype([(k, e + "f8") for k in "xyz"] + [(k, np_t) for k in "rgb"]))
            for k, name in enumerate("xyz"):
                rec[name] = pts[:, k]
            for k, name in enumerate("rgb"):
                rec[name] = raw[:, k]
            f.write(rec.tobytes())
    pc = plyio.read_point_cloud(p)
    np.testing.assert_array_equal(pc.points, pts)
    np.testing.assert_array_equal(pc.colors, want)  # uchar / 255 and double exact, float widened


def test_ply_without_colours_is_as_before(tmp_path):
    p = tmp_path / "n.ply"
    pts = np.random.default_rng(1).standard_normal((10, 3))
    plyio.write_ply(p, pts, binary=True)
    pc = plyio.read_point_cloud(p)
    assert not pc.has_colors() and pc.colors.shape == (0, 3) and not pc.has_normals()
    np.testing.assert_array_equal(pc.points, pts)
    got = plyio.read_ply(p)
    assert len(got) == 2 and got[1] is None


def test_point_cloud_carries_colours():
    rng = np.random.default_rng(2)
    pts, col = rng.standard_normal((30, 3)), rng.uniform(0, 1, (30, 3))
    pc = PointCloud(pts, colors=col)
    assert pc.has_colors() and not PointCloud(pts).has_colors() and not PointCloud().has_colors()
    sel = pc.select_by_index([3, 7, 9])
    np.testing.assert_array_equal(sel.colors, col[[3, 7, 9]])
    np.testing.assert_array_equal(pc.select_by_index([3, 7, 9], invert=True).colors, np.delete(col, [3, 7, 9], axis=0))
    assert not PointCloud(pts).select_by_index([1]).has_colors()
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    np.testing.assert_array_equal(PointCloud(pts.copy(), colors=col.copy()).transform(T).colors, col)


def test_voxel_means_restatement():
    pts = np.array([[0.0, 0, 0], [0.1, 0, 0], [1.0, 0, 0], [0.05, 0.02, 0.0]])
    col = np.array([[0.0, 0.3, 0.6], [0.3, 0.3, 0.0], [1.0, 1.0, 1.0], [0.6, 0.3, 0.3]])
    np.testing.assert_allclose(CI.voxel_means(pts, col, 0.5), [[0.3, 0.3, 0.3], [1.0, 1.0, 1.0]], rtol=0, atol=1e-16)
