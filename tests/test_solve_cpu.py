"""The ICP solve's algebra without a GPU: the restatement of its device-only part
(tests/solve_restatement.py) against mpmath, and the host-compiled hooks of linalg.h (the code the
gfx950 solve compiles) against mpmath with the numpy oracle as the yardstick.
tests/test_gpu_solve.py then pins the device to these two, bit for bit."""
import math
import random

import numpy as np
import pytest

import icp_oracle as I
import solve_cases as SC
import solve_restatement as S
from solve_cases import host_ldlt, host_rotation, umeyama_rotation

mpmath = pytest.importorskip("mpmath")


def test_fma_is_one_rounding():
    """fma() rounds once: known cases where a·b + c in two roundings differs."""
    e = 2.0 ** -52
    assert S.fma(1.0 + e, 1.0 - e, -1.0) == -e * e and (1.0 + e) * (1.0 - e) - 1.0 == 0.0
    assert S.fma(3.0, 1.0 / 3.0, -1.0) == -2.0 ** -54
    # ties to even among subnormals: 1.5 units → 2 units, 0.5 unit → 0
    assert S.fma(5e-324, 0.5, 5e-324) == 1e-323 and S.fma(5e-324, 0.5, 0.0) == 0.0
    assert S.fma(2.0, 3.0, 4.0) == 10.0 and math.isnan(S.fma(math.nan, 1.0, 1.0))


def test_sincos_small_accuracy():
    """sincos_small against 200-bit sin / cos on 20,000 uniform arguments of [−0.5, 0.5] and the
    edges, in ulps of the exact value: < 1 ulp for both, DESIGN's bound (measured: sine 0.566,
    cosine 0.596)."""
    rnd = random.Random(1)
    args = [rnd.uniform(-0.5, 0.5) for _ in range(20000)]
    args += [0.5, -0.5, 0.0, 2.0 ** -27, 1e-300, 5e-324, math.nextafter(0.5, 0.0)]
    ws = wc = 0.0
    for a in args:
        sn, cs = S.sincos_small(a)
        rs, rc = S.mp_sincos(a)
        wc = max(wc, S.ulps(cs, rc))
        if a == 0.0:
            assert sn == 0.0 and cs == 1.0
        else:
            ws = max(ws, S.ulps(sn, rs))
    print(f"sincos_small worst error: sine {ws:.3f} ulp, cosine {wc:.3f} ulp")
    assert ws < 1.0 and wc < 1.0


def test_small_angle_update_is_a_rotation():
    """vec6_to_matrix_sc on sincos_small's values is a rotation to 4·2⁻⁵² in ‖RᵀR − I‖max over the
    small range (each entry of RᵀR is a sum of three products of entries good to about an ulp)."""
    rnd = random.Random(2)
    worst = 0.0
    cases = [[rnd.uniform(-0.5, 0.5) for _ in range(3)] for _ in range(2000)]
    cases += [[0.5, 0.5, 0.5], [-0.5, 0.5, -0.5], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [1e-9, -1e-9, 1e-12]]
    for ang in cases:
        R = S.update_small(ang + [0.1, 0.2, 0.3])[:3, :3]
        worst = max(worst, np.abs(R.T @ R - np.eye(3)).max())
        assert np.linalg.det(R) > 0.0
    print("small-angle update: worst |RtR - I|", worst)
    assert worst <= 4 * 2.0 ** -52


def test_host_ldlt_against_mp_with_the_oracle_as_yardstick():
    """m3d_debug_ldlt6_host (the device solve's rule) on the full-rank systems the device tests feed
    (cond ≤ 1e4; the rank-deficient and the straddling ones have no conditioning to compare under
    and are pinned bit for bit on the device instead): its error against the 200-bit solution is at
    most 8× that of icp_oracle.ldlt_solve (numpy, Eigen's pivoted order), with a floor of
    16·2⁻⁵³·‖x‖∞ — the hook factors without pivoting where the oracle pivots.

    The two errors compared are the maxima over the systems, each error relative to its ‖x‖∞
    (measured: hook 3.3e-13, oracle 3.0e-13).  System by system the ratio of two backward-stable
    solvers' errors is noise — either one can land within an ulp of x by luck: on 'scale_0.5' the
    oracle's error is 1.4e-15 and the hook's 4.4e-14, 31×, both far inside κ·u ≈ 1e-12 — so a
    per-system ratio would test the draw, not the factorisation.  Every per-system figure is
    printed."""
    wh = wo = 0.0
    for name, A, b in SC.plane_full_rank():
        x = S.mp_solve(A, b)
        xn = float(max(abs(v) for v in x))
        eh = float(max(abs(mpmath.mpf(float(g)) - v) for g, v in zip(host_ldlt(A, b), x)))
        eo = float(max(abs(mpmath.mpf(float(g)) - v) for g, v in zip(I.ldlt_solve(A, b), x)))
        print(f"{name}: hook error {eh:.3e}, oracle error {eo:.3e} (|x| {xn:.3g})")
        wh, wo = max(wh, eh / xn), max(wo, eo / xn)
    print(f"ldlt worst relative error: hook {wh:.3e}, oracle {wo:.3e}")
    assert wh <= max(8.0 * wo, 16.0 * S.U)


def test_host_ldlt_singular_systems():
    """Zero columns of J: the hook's zero components are exactly 0.0, as the oracle's; the rest
    agrees with the oracle to the conditioning of the excited block."""
    for name, A, b, zero in SC.plane_singular():
        x = host_ldlt(A, b)
        ref = I.ldlt_solve(A, b)
        for k in zero:
            assert x[k] == 0.0 and ref[k] == 0.0, name
        np.testing.assert_allclose(x, ref, rtol=1e-5 if name.startswith("pivot") else 1e-10, atol=1e-13, err_msg=name)


def test_host_ldlt_non_finite_systems():
    """A NaN anywhere in A or b reaches x (the device solve then writes the identity update) — on
    the diagonal too, where the pivot search cannot see it and the zero-pivot rule alone would
    return a finite x without that axis."""
    _, A, b = SC.plane_full_rank()[1]
    for i, j in ((0, 0), (1, 1), (5, 5), (0, 1), (2, 3)):
        An = A.copy()
        An[i, j] = An[j, i] = np.nan
        assert not np.isfinite(host_ldlt(An, b)).all(), (i, j)
    for k in (0, 3):
        bn = b.copy()
        bn[k] = np.inf
        assert not np.isfinite(host_ldlt(A, bn)).all(), k


def test_host_rotation_from_cov():
    """m3d_debug_rotation_from_cov_host: the rank it reports; for rank ≥ 2 and singular ratio ≤ 1e3
    its error against the 200-bit rotation is at most 4× that of icp_oracle.umeyama's SVD on the
    same H (floor 32·2⁻⁵³); for rank ≤ 1 R is proper orthogonal to 8·2⁻⁵² and (rank 1) maps u0 to
    v0; a non-finite or overflowing H gives the identity.

    Scale 1e-200 is NOT above the s0 > 1e-300 guard: the column norms are taken from squared
    entries, which underflow below about 1e-154, so such an H is H = 0 to rotation_from_cov (rank
    0, identity) — pinned here as it is, with 1e-140 as the small scale that does pass the guard."""
    wh = wo = 0.0
    for name, H, rank, ratio in SC.cov_cases():
        R, got = host_rotation(H)
        if name in ("nan_entry", "scale_1e160"):
            assert got == -1 and np.array_equal(R, np.eye(3)), name
            continue
        if name in ("zero", "scale_1e-200", "scale_1e-320"):
            assert got == 0 and np.array_equal(R, np.eye(3)), name
            continue
        assert got == min(rank, 2), name
        if rank >= 2 and ratio <= 1e3:
            ref = S.mp_rotation_from_cov(H)
            eh = S.mp_max_abs_diff(R, ref)
            eo = S.mp_max_abs_diff(umeyama_rotation(H), ref)
            print(f"{name}: hook error {eh:.3e}, umeyama error {eo:.3e}")
            wh, wo = max(wh, eh), max(wo, eo)
            assert eh <= max(4.0 * eo, 32.0 * S.U), name
        else:
            assert np.abs(R @ R.T - np.eye(3)).max() <= 8 * 2.0 ** -52, name
            assert abs(np.linalg.det(R) - 1.0) <= 8 * 2.0 ** -52, name
            if rank == 1 and name.startswith("rank1"):
                u0, v0 = rank1_directions(H)
                assert np.abs(R @ u0 - v0).max() <= 8 * 2.0 ** -52, name
    print(f"rotation_from_cov worst entry error: hook {wh:.3e}, umeyama {wo:.3e}")


def rank1_directions(H):
    """u0, v0 of H = s·u0·v0ᵀ (u0 source, v0 target), signs tied by H itself."""
    H = np.asarray(H, np.float64)
    i, j = np.unravel_index(np.abs(H).argmax(), H.shape)
    u0 = H[:, j] / np.linalg.norm(H[:, j])
    v0 = H[i, :] / np.linalg.norm(H[i, :])
    if u0 @ H @ v0 < 0:
        v0 = -v0
    return u0, v0


def test_solve_bookkeeping_rule():
    """The restated stop rule on hand cases: `<` is strict, the first evaluation never converges,
    max_iteration = k stops at evaluation k + 1 without an update, a finished loop is frozen."""
    sums = np.zeros(32)
    sums[28], sums[29] = 32.0, 2.0
    p = dict(relative_fitness=0.0, relative_rmse=0.0, max_iteration=30, ns=64)
    st = S.new_state()
    for k in range(5):
        st, upd = S.solve_bookkeeping(st, sums, p)
        assert upd and not st["done"] and st["iters"] == k + 1
    assert st["fitness"] == 0.5 and st["rmse"] == 0.25
    p = dict(relative_fitness=1e-300, relative_rmse=1e-300, max_iteration=30, ns=64)
    st, upd = S.solve_bookkeeping(S.new_state(), sums, p)
    assert upd and not st["converged"]
    st, upd = S.solve_bookkeeping(st, sums, p)
    assert not upd and st["converged"] and st["done"] and st["iters"] == 1 and st["evals"] == 2
    assert S.solve_bookkeeping(st, np.ones(32), p) == (st, False)
    for mi in (0, 1, 2):
        st = S.new_state()
        p = dict(relative_fitness=-1.0, relative_rmse=-1.0, max_iteration=mi, ns=64)
        for k in range(mi + 1):
            st, upd = S.solve_bookkeeping(st, sums, p)
            assert upd == (k < mi)
        assert st["done"] and not st["converged"] and st["iters"] == mi and st["evals"] == mi + 1
