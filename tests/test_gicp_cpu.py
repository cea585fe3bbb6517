"""The Generalized-ICP restatement (tests/gicp_restatement.py) on the CPU: the forms it may use,
the rotation's branch, the covariance invariants, pose recovery, and the condition its loop
fixtures must meet for the GPU test's per-evaluation correspondence comparison."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import gicp_restatement as G
import icp_oracle as I
from m3d import synth


def one_evaluation(ns, nt=777, seed=3):
    src, sn, tgt, tn, T = G.bumpy_pair(ns, nt, seed)
    cs, ct = G.covariances_from_normals(sn, G.EPS), G.covariances_from_normals(tn, G.EPS)
    pcd = I.transform_points(T, src)
    cs = G.rotate_covariances(T[:3, :3], cs)
    _, _, corr, _ = I.registration_result(pcd, tgt, G.RADIUS)
    return pcd, cs, tgt, ct, corr


def test_inverse_form_equals_w_form():
    """Σ J₀ᵀ·M⁻¹·J₀ (closed-form inverse) against Open3D's rows W·d, W·J₀ with W = M^(−1/2) by eigh.
    Measured on this case: the largest |difference| / Σ|term| over the 30 slots is 9.9e-15 (both
    forms carry up to κ(M)·u ≈ 1e-13 of their own); asserted with a margin of 100 at 1e-12."""
    pcd, cs, tgt, ct, corr = one_evaluation(1000)
    assert 300 < len(corr) < 1000
    a, scale = G.gicp_terms(pcd, cs, tgt, ct, corr)
    b = G.gicp_terms_w(pcd, cs, tgt, ct, corr)
    rel = np.abs(a - b) / scale
    print("M^-1 form vs W form, worst |diff| / sum|term|:", rel.max())
    assert rel.max() < 1e-12
    assert a[28] == b[28] == len(corr) and a[29] == b[29]


@pytest.mark.parametrize("ns", [1, 257, 1000])
def test_float64_sums_sit_inside_the_device_bound(ns):
    """The bound the GPU test asserts, |sums − ref| ≤ 1e-11·Σ|term| per slot, holds between the
    restatement in float64 and in np.longdouble (x87 extended here: 64-bit significands) with
    margin: measured worst ratio 2.6e-14."""
    pcd, cs, tgt, ct, corr = one_evaluation(ns)
    a, scale = G.gicp_terms(pcd, cs, tgt, ct, corr)
    b, _ = G.gicp_terms(pcd, cs, tgt, ct, corr, dtype=np.longdouble)
    ok = scale > 0
    rel = np.abs(a - b.astype(np.float64))[ok] / scale[ok]
    print("float64 vs longdouble, worst |diff| / sum|term|:", rel.max() if ok.any() else 0.0)
    assert np.all(np.abs(a - b.astype(np.float64)) <= 1e-11 * scale)
    if np.finfo(np.longdouble).nmant > 52 and ok.any():
        assert rel.max() < 1e-12


def test_rotation_branches():
    e1 = np.array([1.0, 0.0, 0.0])
    np.testing.assert_array_equal(G.rotation_e1_to_x(e1), np.eye(3))
    np.testing.assert_array_equal(G.rotation_e1_to_x(-e1), np.eye(3))  # c = −1 < −0.99
    lo = np.array([-0.995, np.sqrt(1 - 0.995 ** 2), 0.0])  # c < −0.99: the identity, not a rotation
    np.testing.assert_array_equal(G.rotation_e1_to_x(lo), np.eye(3))
    c = -0.99 + 1e-9  # just above: the rotation, factor 1 / (1 + c) ≈ 100
    hi = np.array([c, 0.6 * np.sqrt(1 - c * c), 0.8 * np.sqrt(1 - c * c)])
    for n in (hi, np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, -0.8])):
        R = G.rotation_e1_to_x(n)
        np.testing.assert_allclose(R @ e1, n, atol=1e-13)
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-13)
    # the identity branch leaves C = diag(ε, 1, 1) whatever the normal
    np.testing.assert_array_equal(G.covariances_from_normals([lo, -e1], 1e-3), [np.diag([1e-3, 1, 1])] * 2)


def test_covariances_stay_symmetric_with_their_eigenvalues_after_30_rotations():
    """Tolerances: Rx is orthogonal up to (1 / (1 + c))·|‖n‖² − 1| plus a few roundings, at most
    100·4u ≈ 5e-14 for a normal normalised in fp64, so the eigenvalues start within 1e-13; each of
    the 30 rotations (orthogonal to a few u) moves them by at most ≈ 8u ≈ 1e-15: 2e-13 after."""
    rng = np.random.default_rng(5)
    n = rng.standard_normal((200, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    C = G.covariances_from_normals(n, 1e-3)
    np.testing.assert_array_equal(C, np.swapaxes(C, 1, 2))
    np.testing.assert_allclose(np.linalg.eigvalsh(C), [[1e-3, 1, 1]] * 200, rtol=0, atol=1e-13)
    rot = n[:, 0] >= -0.99  # (the identity branch keeps e1 as the ε axis whatever the normal)
    assert 190 <= rot.sum() < 200
    np.testing.assert_allclose(np.einsum("mij,mj->mi", C, n)[rot], 1e-3 * n[rot], rtol=0, atol=1e-13)  # ε axis
    for k in range(30):
        R = synth.random_rigid(100 + k, rot_range=0.05)[:3, :3]
        C = G.rotate_covariances(R, C)
        n = n @ R.T
    np.testing.assert_array_equal(C, np.swapaxes(C, 1, 2))
    np.testing.assert_allclose(np.linalg.eigvalsh(C), [[1e-3, 1, 1]] * 200, rtol=0, atol=2e-13)
    np.testing.assert_allclose(np.einsum("mij,mj->mi", C, n)[rot], 1e-3 * n[rot], rtol=0, atol=2e-13)


def test_recovers_a_known_pose_without_noise():
    """A noise-free pair whose source points ARE target points moved by T⁻¹: the pose comes back."""
    tgt, tn = synth.surface_points(1500, seed=9)
    T = synth.random_rigid(10, center=tgt.mean(axis=0), rot_range=np.pi / 90, trans_range=0.03)
    Ti = np.linalg.inv(T)
    src, sn = synth.apply(Ti, tgt[::2]), tn[::2] @ Ti[:3, :3].T
    out = G.registration_generalized_icp(src, tgt, 0.5, np.eye(4), G.covariances_from_normals(sn),
                                         G.covariances_from_normals(tn))
    assert out["fitness"] == 1.0 and out["converged"]
    np.testing.assert_allclose(out["transformation"], T, atol=1e-10)
    assert out["inlier_rmse"] < 1e-10


def test_empty_set_and_missing_target_give_the_identity_update():
    src, sn, tgt, tn, _ = G.bumpy_pair(50, 60, 2)
    cs, ct = G.covariances_from_normals(sn), G.covariances_from_normals(tn)
    out = G.registration_generalized_icp(src + 100.0, tgt, 0.5, np.eye(4), cs, ct)
    np.testing.assert_array_equal(out["transformation"], np.eye(4))
    assert (out["fitness"], out["inlier_rmse"], out["iterations"], out["converged"]) == (0.0, 0.0, 1, True)


@pytest.mark.parametrize("kind", ["identity", "perturbed"])
def test_loop_fixtures_have_no_near_ties(kind):
    """Fixture condition of tests/test_gpu_gicp.py: at every evaluation of the restatement, every
    source's best and second-best d² differ by more than 1e-9, and its best d² is farther than
    that from r² — so a device run whose points differ from the restatement's by rounding
    (≈1e-15) must pick the same correspondences."""
    case = G.loop_case(kind)
    tgt = case["tgt"]
    tree = cKDTree(tgt)
    assert 2 <= len(case["evals"]) <= 31 and case["ref"]["converged"]
    worst_gap, worst_edge = np.inf, np.inf
    for pcd, j in case["evals"]:
        _, jj = tree.query(pcd, k=2)
        d0, d1 = I.sq_dist(pcd, tgt[jj[:, 0]]), I.sq_dist(pcd, tgt[jj[:, 1]])
        worst_gap = min(worst_gap, np.abs(d1 - d0).min())
        worst_edge = min(worst_edge, np.abs(np.minimum(d0, d1) - G.LOOP_RADIUS ** 2).min())
        assert 0.5 < (j >= 0).mean() < 1.0  # some sources unmatched at this radius
    print("matched share", (case["evals"][-1][1] >= 0).mean(), "iterations", case["ref"]["iterations"])
    print(f"{kind}: evaluations {len(case['evals'])}, smallest d2 gap {worst_gap:.3e}, to r2 {worst_edge:.3e}")
    assert worst_gap > 1e-9 and worst_edge > 1e-9
    np.testing.assert_allclose(case["ref"]["transformation"], case["T_true"], atol=2e-2)
