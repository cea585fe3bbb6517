"""GPU parity of Fast Global Registration (m3d_fgr_* through m3d.prep and matcher.fgr) against the
CPU restatement in tests/fgr_restatement.py.

What is compared how.  Bit-equal or integer-equal, no tolerance: the 27 sums of one terms pass, the
means, the scale, the tuple test's rows, tuples and trials, par_final, and T_norm / par_final
between the two loop paths — both sides round every operation the same way (fp64, no contraction,
IEEE division and sqrt) and every sum has one order that depends on the count alone
(fgr_restatement.device_sum).  Against sequential summation a sum stays within
(n − 1)·2⁻⁵²·Σ|term|, the bound for two orders of one sum.

T_norm and T against the restatement: max(100 × the scene's two-order difference, 1e-12·max(1, |t|)).
Why not bits: vec6_to_matrix's sin / cos are the device's own on one side and libm's on the other
and may differ in the last bit; each Gauss–Newton step contracts towards the same fixed point, so
such a difference does not grow over the 64 iterations.  TWO_ORDER lists the restatement's own
differences between the device order and sequential sums, measured on the CPU by
tests/test_fgr_cpu.py (all ≤ 1e-15, so every tolerance below is its floor).

Before a run is compared, tests/test_fgr_cpu.py shows on the restatement alone that no decision
hangs on a last bit: every tuple comparison has a relative gap ≥ 1e-9 and the unpivoted solve
holds at every iteration of the well-posed scenes.
"""
import numpy as np
import pytest

import fgr_cases as K
import fgr_restatement as R
from m3d import prep
from m3d.core import Cloud
from m3d.types import FastGlobalRegistrationOption

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]

# rows → the restatement's largest |ΔT| between device-order and sequential sums over the loop cases
TWO_ORDER = {10: 8.9e-16, 11: 5e-16, 64: 3.3e-16, 65: 3.3e-16, 3000: 6.1e-16, 3072: 7.2e-16, "scene600": 4.4e-16}


def option(**fields):
    return FastGlobalRegistrationOption(**fields)


def assert_T(got, ref, two_order):
    tol = max(100 * two_order, 1e-12 * max(1.0, np.abs(ref[:3, 3]).max()))
    d = np.abs(got - ref).max()
    print(f"|ΔT| {d:.3g} (tol {tol:.3g})")
    assert d <= tol


# ------------------------------------------------------------------------------- fgr_terms
@pytest.mark.parametrize("n", K.TERMS_N)
def test_terms_are_the_restatements_bits(n):
    p, q = K.terms_rows()
    for par in K.TERMS_PAR:
        got = prep.fgr_terms(p[:n], q[:n], par)
        terms = R.row_terms(p[:n], q[:n], par)
        assert got.tobytes() == R.expand_sums(R.device_sum(terms)).tobytes()
        seq = R.expand_sums(R.sequential_sum(terms))
        bound = (n - 1) * 2.0 ** -52 * R.expand_sums(np.abs(terms).sum(0))
        assert (np.abs(got - seq) <= np.abs(bound)).all()


def test_terms_of_no_rows_are_zero():
    assert not prep.fgr_terms(np.zeros((0, 3)), np.zeros((0, 3)), 1.0).any()


# ------------------------------------------------------------------------------- normalise, tuple test
@pytest.mark.parametrize("name", list(K.tuple_cases()))
def test_normalise_and_tuple_test(name):
    S, G, rows, fields = K.tuple_cases()[name]
    ref = R.fgr(S, G, rows, R.Option(**fields))
    out = prep.fgr_on_correspondences(S, G, rows, option(**fields), with_details=True)
    assert len(S) != len(G)
    assert out.mean_src.tobytes() == ref.nz.mean_src.tobytes() and out.mean_tgt.tobytes() == ref.nz.mean_tgt.tobytes()
    assert out.scale_global == ref.nz.g and out.n_input == len(rows)
    assert (out.tuples, out.trials) == (ref.tuples, ref.trials)
    np.testing.assert_array_equal(out.rows, ref.rows)
    t_rows, t_trials = prep.fgr_tuple_test(S, G, rows, option(**fields))
    np.testing.assert_array_equal(t_rows, ref.rows)
    assert t_trials == ref.trials
    assert out.par_final == ref.par_final
    if len(ref.rows) < 10:  # too few rows (n3, n10's four tuples give 12; cap 1 / 0 give 3; none_pass 0): T_norm = I
        assert out.T_norm.tobytes() == np.eye(4).tobytes()
        assert out.transformation.tobytes() == ref.T.tobytes()
    else:
        assert_T(out.T_norm, ref.T_norm, TWO_ORDER["scene600"])
        assert_T(out.transformation, ref.T, TWO_ORDER["scene600"])


# ------------------------------------------------------------------------------- the loop
@pytest.mark.parametrize("n", K.LOOP_ROWS)
def test_loop_paths_agree_bitwise_and_with_the_restatement(n):
    S, G, rows, _ = K.big_scene()
    cs, cg = Cloud(S), Cloud(G)
    for fields in K.loop_options():
        one = prep.fgr_on_correspondences(cs, cg, rows[:n], option(**fields), path=1)
        multi = prep.fgr_on_correspondences(cs, cg, rows[:n], option(**fields), path=2)
        auto = prep.fgr_on_correspondences(cs, cg, rows[:n], option(**fields))
        assert one.T_norm.tobytes() == multi.T_norm.tobytes() == auto.T_norm.tobytes(), fields
        assert one.par_final == multi.par_final == auto.par_final
        assert one.transformation.tobytes() == multi.transformation.tobytes()
        ref = R.fgr(S, G, rows[:n], R.Option(**fields))
        assert one.par_final == ref.par_final, fields
        assert_T(one.T_norm, ref.T_norm, TWO_ORDER[n])
        assert_T(one.transformation, ref.T, TWO_ORDER[n])
        if fields["iteration_number"] == 0:
            assert one.T_norm.tobytes() == np.eye(4).tobytes()


def test_more_rows_than_one_workgroup_holds():
    """2·ONE_WG_ROWS + 7 rows (repeats of the scene's): the automatic path is the multi-block one,
    path 1 is refused."""
    S, G, rows, _ = K.big_scene()
    many = np.vstack([rows, rows, rows[:7]])
    o = dict(tuple_test=False, decrease_mu=True, maximum_correspondence_distance=K.LOOP_MAXCD)
    out = prep.fgr_on_correspondences(S, G, many, option(**o))
    forced = prep.fgr_on_correspondences(S, G, many, option(**o), path=2)
    assert out.T_norm.tobytes() == forced.T_norm.tobytes()
    ref = R.fgr(S, G, many, R.Option(**o))
    assert out.par_final == ref.par_final
    assert_T(out.T_norm, ref.T_norm, TWO_ORDER[3072])
    with pytest.raises(ValueError):
        prep.fgr_on_correspondences(S, G, many, option(**o), path=1)


# ------------------------------------------------------------------------------- degenerate inputs
def test_nine_rows_give_the_translation_between_the_means():
    S, G, rows, _ = K.scene600()
    out = prep.fgr_on_correspondences(S, G, rows[:9], option(tuple_test=False), with_details=True)
    assert out.T_norm.tobytes() == np.eye(4).tobytes()
    want = np.eye(4)
    want[:3, 3] = out.mean_tgt - out.mean_src
    assert out.transformation.tobytes() == want.tobytes()
    np.testing.assert_array_equal(out.rows, rows[:9])


@pytest.mark.parametrize("name", list(K.degenerate_cases()))
def test_rank_deficient_rows_follow_the_solve_rule(name):
    """All rows one pair (rank 3) and collinear rows (rank 5): the pivoted solve decides.  The
    components along the null space are rounding noise over rounding noise, so two summation
    orders give different trajectories (the restatement's own two orders differ by 0.02 … 1.8 here):
    what can be compared is one iteration — bit-equal sums, the same solve, then sin / cos within
    2 ulp of libm's on entries ≤ 1, so δ agrees to 1e-14 and the translation x[3:6] in every bit —
    and, over 64 iterations, the two device paths with each other (the same arithmetic) and no NaN."""
    S, G, rows = K.degenerate_cases()[name]
    ref = R.fgr(S, G, rows, R.Option(tuple_test=False, iteration_number=1))
    assert ref.lp.spd == [False]
    for path in (1, 2):
        out = prep.fgr_on_correspondences(S, G, rows, option(tuple_test=False, iteration_number=1), path=path)
        np.testing.assert_allclose(out.T_norm[:3, :3], ref.T_norm[:3, :3], atol=1e-14, rtol=0)
        assert out.T_norm[:, 3].tobytes() == ref.T_norm[:, 3].tobytes()
        np.testing.assert_allclose(out.transformation, ref.T, atol=1e-13 * max(1.0, np.abs(ref.T).max()), rtol=0)
    one = prep.fgr_on_correspondences(S, G, rows, option(tuple_test=False), path=1)
    multi = prep.fgr_on_correspondences(S, G, rows, option(tuple_test=False), path=2)
    assert np.isfinite(one.transformation).all() and np.isfinite(one.T_norm).all()
    assert one.T_norm.tobytes() == multi.T_norm.tobytes() and one.transformation.tobytes() == multi.transformation.tobytes()


def test_empty_rows_and_empty_clouds():
    from matcher import registration_fgr_based_on_feature_matching

    S, G, rows, _ = K.scene600()
    out = prep.fgr_on_correspondences(S, G, np.zeros((0, 2), np.int32), option(), with_details=True)
    assert out.T_norm.tobytes() == np.eye(4).tobytes() and len(out.rows) == 0 and out.tuples == 0
    np.testing.assert_array_equal(out.transformation[:3, 3], out.mean_tgt - out.mean_src)
    none = prep.fgr_on_correspondences(np.zeros((0, 3)), G, np.zeros((0, 2), np.int32), option())
    assert none.transformation.tobytes() == np.eye(4).tobytes() and none.fitness == 0.0
    assert len(none.correspondence_set) == 0
    res = registration_fgr_based_on_feature_matching(np.zeros((0, 3)), G, np.zeros((0, 33)), np.zeros((len(G), 33)))
    assert res.transformation.tobytes() == np.eye(4).tobytes() and res.fitness == 0.0
    with pytest.raises(ValueError):
        prep.fgr_on_correspondences(S, G, [[0, len(G)]], option())
    with pytest.raises(ValueError):
        registration_fgr_based_on_feature_matching(S, G, np.zeros((5, 33)), np.zeros((len(G), 33)))


# ------------------------------------------------------------------------------- full calls
_full = {}
FULL_VOXEL = 0.44


def full_pair():
    """A synthetic scan pair through Ply's preprocessing at voxel 0.44: about 2000 down-sampled
    points each.  Checked on the CPU first: the oracle's preprocessing and FPFH (oracle/prep_oracle.py:
    2119 / 2175 points, 898 mutual rows), the restatement (coarse max |ΔT| 3.5e-2, smallest tuple gap
    2e-7) and the oracle's point-to-plane ICP from there end at max |ΔT| 6.2e-5."""
    if not _full:
        from m3d import synth
        from ply import Ply

        T = synth.random_rigid(31, rot_range=0.5, trans_range=0.5)
        tgt_pts, tgt_n = synth.surface_points(20000, seed=2)
        src_pts, src_n = synth.surface_points(18000, seed=1)
        Ti = np.linalg.inv(T)
        np.random.seed(0)
        src = Ply.from_arrays(synth.apply(Ti, src_pts), src_n @ Ti[:3, :3].T, voxel_size=FULL_VOXEL, preprocess=True)
        tgt = Ply.from_arrays(tgt_pts, tgt_n, voxel_size=FULL_VOXEL, preprocess=True)
        _full["pair"] = (src, tgt, T)
    return _full["pair"]


def test_feature_matching_call():
    from matcher import evaluate_registration, registration_fgr_based_on_feature_matching

    src, tgt, T = full_pair()
    s_pts, t_pts = src.pcd_down.points, tgt.pcd_down.points
    assert 1500 <= len(s_pts) <= 2600 and 1500 <= len(t_pts) <= 2600
    o = option(maximum_correspondence_distance=0.5 * FULL_VOXEL)
    res = registration_fgr_based_on_feature_matching(src, tgt, src.pcd_fpfh, tgt.pcd_fpfh, o)
    again = registration_fgr_based_on_feature_matching(src, tgt, src.pcd_fpfh, tgt.pcd_fpfh, o)
    assert res.transformation.tobytes() == again.transformation.tobytes()
    assert (res.fitness, res.inlier_rmse) == (again.fitness, again.inlier_rmse)
    np.testing.assert_array_equal(res.correspondence_set, again.correspondence_set)
    # the rows: the restatement fed the device's own features' mutual pairs
    corres = prep.feature_correspondences(src.pcd_fpfh, tgt.pcd_fpfh, True, 0.0)
    assert (np.diff(corres[:, 0]) > 0).all()
    ref = R.fgr(s_pts, t_pts, corres, R.Option(maximum_correspondence_distance=0.5 * FULL_VOXEL))
    assert ref.tup.min_gap >= 1e-9
    det = prep.fgr_on_correspondences(s_pts, t_pts, corres, o, with_details=True)
    np.testing.assert_array_equal(det.rows, ref.rows)
    assert (det.tuples, det.trials) == (ref.tuples, ref.trials)
    assert det.transformation.tobytes() == res.transformation.tobytes()
    ev = evaluate_registration(s_pts, t_pts, 0.5 * FULL_VOXEL, res.transformation)
    assert (res.fitness, res.inlier_rmse) == (ev.fitness, ev.inlier_rmse)
    np.testing.assert_array_equal(res.correspondence_set, ev.correspondence_set)


def test_register_with_fgr_reaches_the_pose_and_the_default_is_unchanged():
    from matcher import global_registration, refine_registration, register

    src, tgt, T = full_pair()
    res = register(src, tgt, coarse="fgr")
    print("register(coarse='fgr') max |ΔT|", np.abs(res.transformation - T).max())
    np.testing.assert_allclose(res.transformation, T, atol=5e-3)
    # no `coarse`: exactly the two stages it ran before
    plain = register(src, tgt)
    before = refine_registration(src, tgt, global_registration(src, tgt, src.voxel_size, iteration=30).transformation,
                                 src.voxel_size)
    assert plain.transformation.tobytes() == before.transformation.tobytes()
    assert (plain.fitness, plain.inlier_rmse) == (before.fitness, before.inlier_rmse)
    assert register(src, tgt, coarse="ransac").transformation.tobytes() == plain.transformation.tobytes()
