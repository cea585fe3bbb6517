"""Constructed inputs of the ICP device solve (icp.hip solve_state), shared by tests/test_solve_cpu.py
(the host-compiled algebra against mpmath) and tests/test_gpu_solve.py (the gfx950 solve against
the host-compiled algebra and the restatement).  Everything is built once, from fixed seeds.

A point-to-plane system is (name, A, b): A the full symmetric 6×6 (mirrored from its upper triangle,
as solve_state builds it from slots 0..20), b the right-hand side the solve sees (slots 21..26 hold
−b).  A point-to-point case is (name, H, true_rank, ratio): the 3×3 cross-covariance H = Σ p qᵀ
rotation_from_cov sees, the rank it was built with and s0 / s(rank−1)."""
import ctypes as C
import math

import numpy as np

P = C.POINTER(C.c_double)


def host_ldlt(A, b):
    """m3d_debug_ldlt6_host: linalg.h's solve rule (unpivoted, pivoted fall-back) compiled for the host."""
    from m3d import _lib

    x = np.zeros(6)
    A = np.ascontiguousarray(A, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    assert _lib.load().m3d_debug_ldlt6_host(A.ctypes.data_as(P), b.ctypes.data_as(P), x.ctypes.data_as(P)) == 0
    return x


def host_rotation(H):
    """m3d_debug_rotation_from_cov_host → (R 3×3, the rank it used)."""
    from m3d import _lib

    H = np.ascontiguousarray(np.asarray(H, np.float64).reshape(9))
    R = np.zeros(9)
    rank = _lib.load().m3d_debug_rotation_from_cov_host(H.ctypes.data_as(P), R.ctypes.data_as(P))
    return R.reshape(3, 3), rank


def umeyama_rotation(H):
    """icp_oracle.umeyama's rotation for the cross-covariance H = Σ p qᵀ: six point pairs with zero
    means, p = ±e_k and q = ± row k of H, so that Σ p qᵀ = 2·H (umeyama is invariant to the
    factor)."""
    import icp_oracle as I

    H = np.asarray(H, np.float64)
    return I.umeyama(np.vstack([np.eye(3), -np.eye(3)]), np.vstack([H, -H]))[:3, :3]


ANGLE_SCALES = (1e-9, 1e-3, 0.49, 0.5, math.nextafter(0.5, 1.0), 1.0, 3.0)


def mirror(A):
    """The symmetric matrix of A's upper triangle."""
    U = np.triu(np.asarray(A, np.float64))
    return U + np.triu(U, 1).T


def rot(rng):
    Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = Q * np.sign(np.diag(R))
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    return Q


def plane_full_rank():
    """JᵀJ = Q·diag(λ)·Qᵀ with cond ≤ 1e4 and b = A·x★, max |x★[0..2]| at every scale of
    ANGLE_SCALES (the computed x sits within cond·u of it: whichever side of 0.5 it lands decides
    the branch, and the test reads the side from the host solution); 'one_big': one angle above 0.5
    and two tiny ones (the branch is on the maximum).  'exact_*': A diagonal with power-of-two
    entries, so that both factorisations are exact and x[0] IS the stated value: exactly 0.5 and
    its two neighbours."""
    rng = np.random.default_rng(20)
    out = []
    for k, sc in enumerate(ANGLE_SCALES):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = 10.0 ** rng.uniform(0.0, 4.0, 6)
        lam[0], lam[5] = 1.0, 1e4
        A = mirror((Q * lam) @ Q.T)
        ang = rng.uniform(-1.0, 1.0, 3)
        ang *= sc / np.abs(ang).max()
        xs = np.concatenate([ang, rng.uniform(-0.3, 0.3, 3)])
        out.append((f"scale_{sc!r}", A, A @ xs))
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    A = mirror((Q * np.array([1.0, 3.0, 20.0, 150.0, 900.0, 5e3])) @ Q.T)
    out.append(("one_big", A, A @ np.array([1e-7, 0.8, -2e-8, 0.1, -0.2, 0.05])))
    d = np.array([4.0, 1.0, 64.0, 4096.0, 2.0, 512.0])
    for name, a0 in (("exact_half", 0.5), ("exact_above_half", math.nextafter(0.5, 1.0)),
                     ("exact_below_half", math.nextafter(0.5, 0.0)), ("exact_minus_half", -0.5)):
        xs = np.array([a0, -0.25, 0.125, 0.75, -1.5, 0.375])
        out.append((name, np.diag(d), d * xs))
    return out


def plane_singular():
    """Rank-deficient JᵀJ: each single zero column of J (b[k] = 0), two zero columns, A = 0, and a
    pivot straddling ldlt6_solve_spd's fall-back.  Straddle: A = L·D·Lᵀ with D = (4, 1, d2, 1, 1, 1),
    unit lower L with entries 0 / ±0.25 / ±0.5 and row 2 of L zero left of the diagonal, so that
    A[2][2] = d2 and the unpivoted pivot 2 = d2 exactly; every diagonal entry of A but the first is
    below 4, so lo = 1e-9·dmax = 1e-9·4.  d2 = the double above lo (the unpivoted path keeps it:
    D > lo) and lo itself (not > lo: the pivoted fall-back)."""
    rng = np.random.default_rng(21)
    out = []
    for zero in ((0,), (1,), (2,), (3,), (4,), (5,), (1, 4)):
        J = rng.standard_normal((50, 6))
        J[:, list(zero)] = 0.0
        A = mirror(J.T @ J)
        b = rng.standard_normal(6)
        b[list(zero)] = 0.0
        out.append(("zero_" + "_".join(map(str, zero)), A, b, zero))
    out.append(("zero_matrix", np.zeros((6, 6)), rng.standard_normal(6), (0, 1, 2, 3, 4, 5)))
    L = np.eye(6)
    L[1, 0] = 0.5
    L[3, :3] = (0.25, -0.5, 0.5)
    L[4, :4] = (-0.5, 0.25, -0.25, 0.5)
    L[5, :5] = (0.25, 0.5, 0.5, -0.25, 0.25)
    lo = 1e-9 * 4.0
    for name, d2 in (("pivot_above", math.nextafter(lo, 1.0)), ("pivot_at", lo)):
        A = mirror((L * np.array([4.0, 1.0, d2, 1.0, 1.0, 1.0])) @ L.T)
        assert A[2, 2] == d2 and np.diag(A).max() == 4.0 == A[0, 0]
        out.append((name, A, np.array([0.01, -0.02, 1e-10, 0.3, -0.1, 0.2]), ()))
    return out


def cov_cases():
    """Cross-covariances for rotation_from_cov → (name, H, true rank, s0 / s_last-nonzero)."""
    rng = np.random.default_rng(22)
    Ra, Rb, Rc = rot(rng), rot(rng), rot(rng)
    full = Ra @ np.diag([3.0, 2.0, 1.0])
    out = [
        ("rot_321", full, 3, 3.0),
        ("equal_leading", 2.0 * Rb, 3, 1.0),
        ("equal_trailing", Ra @ np.diag([3.0, 1.0, 1.0]) @ Rb.T, 3, 3.0),
        ("reflection", Ra @ np.diag([3.0, 2.0, -1.0]) @ Rb.T, 3, 3.0),
        ("rank2", Rc @ np.diag([3.0, 2.0, 0.0]), 2, 1.5),
        ("ratio_1e3", Ra @ np.diag([1e3, 1.0, 0.5]) @ Rc.T, 3, 1e3),
        ("s1_above_1e-14", Ra @ np.diag([1.0, 2e-14, 0.0]) @ Rb.T, 2, 5e13),
        ("s1_below_1e-14", Ra @ np.diag([1.0, 0.5e-14, 0.0]) @ Rb.T, 1, 1.0),
        ("zero", np.zeros((3, 3)), 0, 1.0),
        ("scale_1e-140", 1e-140 * full, 3, 3.0),
        ("scale_1e-200", 1e-200 * full, 3, 3.0),
        ("scale_1e-320", 1e-320 * full, 3, 3.0),
        ("scale_1e160", 1e160 * full, 3, 3.0),
    ]
    nan = full.copy()
    nan[1, 2] = np.nan
    out.append(("nan_entry", nan, 3, 3.0))
    u = rng.standard_normal(3)
    v = rng.standard_normal(3)
    r1 = [("generic", u, v), ("axes", [0, 2.0, 0], [0, 0, -3.0]), ("axis_x_z", [1.5, 0, 0], [0, 0, 1.0]),
          ("tie_xy", [1.0, -1.0, 0.5], [2.0, 0.5, 0.5]), ("tie_yz", [3.0, 1.0, 1.0], [0.5, -2.0, 2.0]),
          ("tie_all", [1.0, 1.0, 1.0], [-1.0, 1.0, -1.0]), ("tie_xz_small", [0.25, 2.0, -0.25], [1.0, 0, 1.0])]
    for name, a, b in r1:
        out.append(("rank1_" + name, np.outer(np.asarray(a, np.float64), np.asarray(b, np.float64)), 1, 1.0))
    return out
