"""GPU parity of the registration evaluation (m3d_evaluate_registration through m3d.core.evaluate
and the matcher drop-in layer) against the CPU oracle.

Reference of every case: ``icp_oracle.initial_points(T, src)`` (the source, transformed unless T
isIdentity()) and ``icp_oracle.registration_result`` of those points: fitness, the correspondence
set and the per-source d².  The information matrix is restated literally below (``info_ref``):
the three rows G₁ = (0, z, −y, 1, 0, 0), G₂ = (−z, 0, x, 0, 1, 0), G₃ = (y, −x, 0, 0, 0, 1) of
every matched TARGET point, every entry (a, b) the sum of the terms G_r[a]·G_r[b]; each term is
taken exactly (Dekker's product: value + error), so ``math.fsum`` gives the correctly rounded
entry, and S = Σ|term|.

Bounds (derived, not measured).  Summing n rounded fp64 terms in any order errs by at most
n·2⁻⁵³·Σ|term|; a diagonal entry of GᵀG is formed from two such sums, hence
    |information_dev − ref| ≤ n·2⁻⁵²·S   per entry, n = matched pairs
(S = 0, the structural zeros: exactly 0), and likewise |Σd²_dev − fsum(d²)| ≤ n·2⁻⁵²·Σd².  The
entry point returns inlier_rmse = sqrt(Σd²_dev / n), not the sum, so that bound is asserted on
the root it implies: a relative error a of the sum is a/2 of the root (n·2⁻⁵³), plus half a
rounding of the division and one of the root (1.5·2⁻⁵³); the reference sqrt(fsum(d²) / n) carries
its own three roundings (≤ 2·2⁻⁵³):  |rmse_dev − rmse_ref| ≤ (n + 4)·2⁻⁵³·rmse_ref.
Indices, d², the count and fitness are compared exactly; brute force and the grid, and two calls
of one method, must agree in every bit, sums included.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_oracle as I
import matcher
from m3d import synth
from m3d.core import Cloud, evaluate, nn1

pytestmark = pytest.mark.gpu

U52 = 2.0 ** -52
U53 = 2.0 ** -53


def two_prod(a, b):
    """a·b = p + e exactly (Dekker / Veltkamp; no overflow at these magnitudes)."""
    p = a * b
    c = 134217729.0  # 2^27 + 1

    def split(v):
        t = v * c
        hi = t - (t - v)
        return hi, v - hi

    ah, al = split(a)
    bh, bl = split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def info_ref(q):
    """GᵀG over the points q (n, 3), literally: (ref, S), both (6, 6); ref correctly rounded."""
    n = len(q)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    o, l = np.zeros(n), np.ones(n)
    G = np.stack([np.stack([o, z, -y, l, o, o], axis=1),
                  np.stack([-z, o, x, o, l, o], axis=1),
                  np.stack([y, -x, o, o, o, l], axis=1)], axis=1)  # (n, 3 rows, 6)
    ref, S = np.zeros((6, 6)), np.zeros((6, 6))
    for a in range(6):
        for b in range(a, 6):
            p, e = two_prod(G[:, :, a].ravel(), G[:, :, b].ravel())
            ref[a, b] = ref[b, a] = math.fsum(np.concatenate([p, e]))
            S[a, b] = S[b, a] = math.fsum(np.abs(p))
    return ref, S


def run(s, t, T, r, nn):
    out = evaluate(s, t, T, r, nn=nn, information=True, with_correspondences=True, with_distances=True)
    return out, out.d2.cpu().numpy(), out.corr_idx.cpu().numpy()


def check_case(src, tgt, T, r, against_nn1=False, expect_fitness=None):
    """Every assertion of the module docstring for one (src, tgt, T, r), both NN methods."""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    ns = len(src)
    pts = I.initial_points(T, src)
    if len(tgt) > 0:
        fit, _, pairs, d2_ref = I.registration_result(pts, tgt, r)
    else:
        fit, pairs, d2_ref = 0.0, np.zeros((0, 2), np.int64), np.full(ns, np.inf)
    n = len(pairs)
    if expect_fitness is not None:
        assert round(fit, 3) == expect_fitness
    ref, S = info_ref(tgt[pairs[:, 1]])
    sum_ref = math.fsum(d2_ref[pairs[:, 0]])
    rmse_ref = math.sqrt(sum_ref / n) if n else 0.0
    idx_ref = np.full(ns, -1, np.int64)
    idx_ref[pairs[:, 0]] = pairs[:, 1]
    s, t = Cloud(src), Cloud(tgt)
    got = {}
    for nn in ("brute", "grid"):
        out, d2, idx = run(s, t, T, r, nn)
        np.testing.assert_array_equal(out.correspondence_set, pairs)
        np.testing.assert_array_equal(idx, idx_ref)
        np.testing.assert_array_equal(d2, d2_ref)
        assert out.num_correspondences == n
        assert out.fitness == fit
        err_rmse, tol_rmse = abs(out.inlier_rmse - rmse_ref), (n + 4) * U53 * rmse_ref
        err = np.abs(out.information - ref)
        tol = n * U52 * S
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0)))
        print(f"{nn}: ns {ns} matched {n} fitness {out.fitness:.4f} rmse err {err_rmse:.3e} (tol {tol_rmse:.3e}) "
              f"information max err/tol {worst:.3e}")
        assert err_rmse <= tol_rmse
        assert (err <= tol).all(), (err, tol)
        got[nn] = (out, d2, idx)
    # brute force and the grid: every output bit, sums included; and a second call of each
    for nn in ("brute", "grid"):
        out, d2, idx = run(s, t, T, r, nn)
        for o, dd, ii in (got["brute"], got["grid"]):
            assert (o.fitness, o.num_correspondences) == (out.fitness, out.num_correspondences)
            assert np.float64(o.inlier_rmse).tobytes() == np.float64(out.inlier_rmse).tobytes()
            assert o.information.tobytes() == out.information.tobytes()
            assert dd.tobytes() == d2.tobytes() and np.array_equal(ii, idx)
    if against_nn1:  # T not isIdentity(): nn1 applies the same transform
        assert not I.is_identity(T)
        for nn in ("brute", "grid"):
            i1, d1 = nn1(s, t, T, r, nn=nn)
            np.testing.assert_array_equal(i1.cpu().numpy(), got[nn][2])
            assert d1.cpu().numpy().tobytes() == got[nn][1].tobytes()
    return got["grid"][0]


def near_truth(T_true):
    return I.matmul4(synth.random_rigid(11, rot_range=0.01, trans_range=0.05), T_true)


def shift_T(T, c):
    A, B = np.eye(4), np.eye(4)
    A[:3, 3], B[:3, 3] = c, -np.asarray(c)
    return I.matmul4(I.matmul4(A, T), B)


OFFSET = np.array([1e5, -2e5, 3e4])


def test_small_pair_half_unmatched():
    src, tgt, _, T_true = synth.icp_pair(257, 300, seed=7)
    check_case(src, tgt, near_truth(T_true), 0.5, against_nn1=True, expect_fitness=0.529)


def test_pair_3000_4000():
    src, tgt, _, T_true = synth.icp_pair(3000, 4000, seed=5)
    check_case(src, tgt, near_truth(T_true), 0.3, against_nn1=True, expect_fitness=0.976)


def test_partial_overlap_target_cut():
    src, tgt, _, T_true = synth.icp_pair(3000, 4000, seed=5)
    cut = tgt[tgt[:, 0] > tgt[:, 0].mean()]
    assert len(cut) == 1990
    check_case(src, cut, T_true, 0.3, against_nn1=True, expect_fitness=0.483)


@pytest.mark.parametrize("eps", [0.0, 1e-13, 1e-11])
def test_identity_rule(eps):
    """T = I and T within 1e-12 of it leave the points untouched (isIdentity()); 1e-11 off is
    applied — each against initial_points."""
    src, tgt, _, _ = synth.icp_pair(500, 600, seed=9)
    T = np.eye(4)
    T[1, 2] += eps
    assert I.is_identity(T) == (eps < 1e-12)
    check_case(src * 1.003, tgt, T, 0.4)


def test_large_absolute_coordinates():
    """Both clouds shifted by (1e5, −2e5, 3e4): information entries ≈ 1e13.  Centred or fp32
    target coordinates would miss the bound by many orders of magnitude."""
    src, tgt, _, T_true = synth.icp_pair(3000, 4000, seed=5)
    out = check_case(src + OFFSET, tgt + OFFSET, shift_T(near_truth(T_true), OFFSET), 0.3, against_nn1=True)
    assert out.information[0, 0] > 1e13 and out.fitness > 0.9


@pytest.mark.parametrize("ns", [1, 255, 256, 257, 513])
def test_block_edges(ns):
    src, tgt, _, T_true = synth.icp_pair(513, 300, seed=7)
    check_case(src[:ns], tgt, near_truth(T_true), 0.5)


def test_more_than_256_partial_blocks():
    src, tgt, _, T_true = synth.icp_pair(70_000, 5000, seed=3)
    out = check_case(src, tgt, near_truth(T_true), 0.3)
    assert out.num_correspondences > 256 * 256 // 2


@pytest.mark.parametrize("case", ["ns0", "nt0", "far"])
def test_nothing_matched(case):
    src, tgt, _, T_true = synth.icp_pair(257, 300, seed=7)
    if case == "ns0":
        src = np.zeros((0, 3))
    elif case == "nt0":
        tgt = np.zeros((0, 3))
    else:
        src = src + 1e3
    out = check_case(src, tgt, near_truth(T_true), 0.5)
    assert (out.fitness, out.inlier_rmse, out.num_correspondences) == (0.0, 0.0, 0)
    assert out.correspondence_set.shape == (0, 2)
    assert out.information.shape == (6, 6) and not out.information.any()


def test_duplicate_targets_lowest_index_wins():
    rng = np.random.default_rng(21)
    dup = np.repeat(rng.normal(size=(50, 3)), 40, axis=0)
    out = check_case(dup + 1e-3, dup, np.eye(4), 0.5)
    assert out.fitness == 1.0 and (out.correspondence_set[:, 1] % 40 == 0).all()


def test_dense_target_cell_defers_queries():
    """A vertex fan (3000 targets within 0.004 of one point: ≥ 256 in one cell at r) makes the grid
    loop defer the queries near it to its one-block-per-query kernel; the evaluation reads that
    list's header next to its sums and must report the same result as brute force."""
    rng = np.random.default_rng(21)
    sph, _ = synth.surface_points(30000, seed=3)
    fan = np.vstack([sph, sph[7] + rng.normal(scale=0.002, size=(3000, 3))])
    src = np.vstack([sph[::3] * 1.001, sph[7] + rng.normal(scale=0.03, size=(2000, 3))])
    out = check_case(src, fan, synth.random_rigid(17, rot_range=0.01, trans_range=0.01), 0.12, against_nn1=True)
    assert out.fitness > 0.9


@pytest.mark.parametrize("shifted", [False, True])
def test_compute_point_cloud_distance(shifted):
    if shifted:
        src, tgt, _, T_true = synth.icp_pair(3000, 4000, seed=5)
        src, tgt, T = src + OFFSET, tgt + OFFSET, shift_T(near_truth(T_true), OFFSET)
    else:
        src, tgt, _, T_true = synth.icp_pair(257, 300, seed=7)
        T = near_truth(T_true)
    pts = I.initial_points(T, src)
    j, d2_ref = I.nn_exact(cKDTree(tgt), tgt, pts, 1e7)  # unbounded: every source has a neighbour
    assert (j >= 0).all()
    np.testing.assert_array_equal(d2_ref, I.sq_dist(pts, tgt[j]))
    got = matcher.compute_point_cloud_distance(src, tgt, T)
    assert got.dtype == np.float64 and got.shape == (len(src),)
    np.testing.assert_array_equal(got, np.sqrt(d2_ref))
    # the squared distances themselves, bit for bit (same call the function makes)
    from matcher.evaluate import _reach

    out = evaluate(Cloud(src), Cloud(tgt), T, _reach(src, tgt, T), nn="brute", with_correspondences=True,
                   with_distances=True)
    assert out.d2.cpu().numpy().tobytes() == d2_ref.tobytes()
    np.testing.assert_array_equal(out.corr_idx.cpu().numpy(), j)
    assert out.fitness == 1.0
    if not shifted:
        np.testing.assert_array_equal(matcher.compute_point_cloud_distance(src, np.zeros((0, 3))), np.zeros(len(src)))
        assert matcher.compute_point_cloud_distance(np.zeros((0, 3)), tgt).shape == (0,)
        # no transformation: the cloud as it is
        np.testing.assert_array_equal(matcher.compute_point_cloud_distance(src, tgt),
                                      np.sqrt(I.nn_exact(cKDTree(tgt), tgt, src, 1e7)[1]))


def test_drop_in_layer():
    src, tgt, nrm, T_true = synth.icp_pair(3000, 4000, seed=5)
    T, r = near_truth(T_true), 0.3
    ref = evaluate(Cloud(src), Cloud(tgt), T, r, information=True)
    ply_s = SimpleNamespace(pcd=SimpleNamespace(points=src, normals=np.zeros((0, 3))))
    ply_t = SimpleNamespace(pcd=SimpleNamespace(points=tgt, normals=nrm))
    for a, b in ((ply_s, ply_t), (src, tgt), (ply_s.pcd, tgt)):
        res = matcher.evaluate_registration(a, b, r, T)
        assert (res.fitness, res.inlier_rmse) == (ref.fitness, ref.inlier_rmse)
        np.testing.assert_array_equal(res.correspondence_set, ref.correspondence_set)
        np.testing.assert_array_equal(res.transformation, T)
        G = matcher.get_information_matrix_from_point_clouds(a, b, r, T)
        assert G.shape == (6, 6) and G.dtype == np.float64
        assert G.tobytes() == ref.information.tobytes()
    np.testing.assert_array_equal(G, G.T)
    np.testing.assert_array_equal(G[3:, 3:], ref.num_correspondences * np.eye(3))
    assert ref.num_correspondences == len(ref.correspondence_set) > 0
    # the PointCloud method is the same call
    from m3d.types import PointCloud

    np.testing.assert_array_equal(PointCloud(src[:300]).compute_point_cloud_distance(PointCloud(tgt)),
                                  matcher.compute_point_cloud_distance(src[:300], tgt))
    # default transformation: identity
    e0 =matcher.evaluate_registration(src, tgt, r)
    o0 = evaluate(Cloud(src), Cloud(tgt), np.eye(4), r)
    assert (e0.fitness, e0.inlier_rmse) == (o0.fitness, o0.inlier_rmse)
