"""The ICP device solve (icp.hip solve_state, compiled for gfx950) on constructed sums.

Every cloud ICP loop, Generalized ICP, the robust kernels, Colored ICP and mesh ICP end in this one
function.  IcpLoop.solve takes a caller-owned buffer of 32 doubles and IcpLoop.result() returns what
the solve made of it, so a test hands the device any normal equations or cross-covariance: no search
is ever run here (but for the anchor test, which shows that the constructed sums speak the terms
pass's language, and the points() test at the end).

The library is built with -ffp-contract=off and the algebra is + − × / sqrt fma, correctly rounded
on both sides, so the device result is pinned bit for bit
  * against the same header compiled for the host (m3d_debug_ldlt6_host,
    m3d_debug_rotation_from_cov_host), and
  * against the pure-Python restatement (tests/solve_restatement.py) of what exists only on the
    device: sincos_small, vec6_to_matrix_sc as the wave evaluates it, matmul4_affine, the stop rule;
tests/test_solve_cpu.py holds those two against mpmath.  Only the libm sincos branch (max |angle| >
0.5) is compared with a tolerance, derived below.

Scope: constructed sums reach solve_kernel only.  The fused tails (terms_solve_kernel,
reduce_solve_kernel, reduce_groups_kernel) call the same solve_state and the fused-against-unfused
tests (test_gpu_icp, test_gpu_sum_order, test_gpu_nn_terms_fused) pin them to solve_kernel bit for
bit; there are no probes into those kernels here.

Slot layout (include/m3d.h, icp.hip terms_add): point-to-plane JᵀJ's upper triangle row-major in
0..20, Jᵀr in 21..26 (the solve negates it), Σr² in 27; point-to-point Σ(p − c) in 0..2, Σ(q − c)
in 3..5, Σ(p − c)(q − c)ᵀ row-major in 6..14, p the loop's (transformed) source point, q its target
and c the SOURCE cloud's centre for both moments (terms_add subtracts a.c = src->center from p and
from q alike; the solve adds sp.c back to both means); both: count in 28, Σd² in 29."""
import math

import numpy as np
import pytest

import solve_cases as SC
import solve_restatement as S
from m3d import _lib, synth
from m3d.core import Cloud, IcpLoop
from solve_cases import host_ldlt, host_rotation, umeyama_rotation

pytestmark = pytest.mark.gpu

PLANE, POINT = _lib.EST_POINT_TO_PLANE, _lib.EST_POINT_TO_POINT
CENTRE = np.array([0.5, -0.25, 1.0])  # the 64-point source's centre: exactly representable
NS = 64
INIT = synth.random_rigid(5, rot_range=0.3, trans_range=0.2)
EYE = np.eye(4)


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(30)
    src = rng.uniform(-1.0, 1.0, (NS, 3)) + CENTRE
    tgt = rng.uniform(-1.0, 1.0, (NS, 3))
    nrm = rng.standard_normal((NS, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return Cloud(src, center=CENTRE), Cloud(tgt, nrm)


def make_loop(clouds, est, relative_fitness=-1.0, relative_rmse=-1.0, max_iteration=1000):
    return IcpLoop(clouds[0], clouds[1], 0.5, estimation=est, relative_fitness=relative_fitness,
                   relative_rmse=relative_rmse, max_iteration=max_iteration, nn="brute")


@pytest.fixture(scope="module")
def loops(clouds):
    return {est: make_loop(clouds, est) for est in (PLANE, POINT)}


def feed(lp, sums):
    import torch

    lp.solve(torch.from_numpy(np.ascontiguousarray(sums, np.float64)).cuda())
    return lp.result()


def solve_once(lp, sums, init=INIT):
    lp.reset(init)
    return feed(lp, sums)


def plane_sums(A, b, count=32.0, sd2=0.5):
    s = np.zeros(32)
    s[:21] = np.asarray(A)[np.triu_indices(6)]
    s[21:27] = -np.asarray(b)
    s[28], s[29] = count, sd2
    return s


def point_sums(H, count=64.0, sd2=0.5, sp=(0.0, 0.0, 0.0), sq=(0.0, 0.0, 0.0)):
    """count·H in the second-moment slots: with count a power of two and zero first moments the
    solve's H = S/n − mp·mqᵀ is the given matrix exactly."""
    s = np.zeros(32)
    s[0:3], s[3:6] = sp, sq
    s[6:15] = (np.asarray(H, np.float64) * count).reshape(9)
    s[28], s[29] = count, sd2
    return s


def same(a, b, what):
    """Equal values in every entry (==: a −0 equals a +0), no NaN."""
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(a, b), f"{what}: differs by {np.abs(a - b).max()}\n{a!r}\n{b!r}"


# ------------------------------------------------------------------------------- the anchor
@pytest.mark.parametrize("est", [PLANE, POINT])
def test_constructed_sums_speak_the_terms_language(est):
    """One real 512-point pair, a small non-identity init: the sums of shard_nn + shard_terms equal
    the slots recomputed in fp64 numpy from lp.points() and lp.correspondences() in the layout of
    the module docstring — per slot to 1e-12 of Σ|term| (the sums differ in order only).  The
    point-to-point moments are centred on the source's centre, both of them."""
    import torch

    src, tgt, nrm, _ = synth.icp_pair(512, seed=31)
    c = np.array([0.125, -0.5, 0.25])
    lp = IcpLoop(Cloud(src, center=c), Cloud(tgt, nrm), 0.3, estimation=est, nn="brute")
    lp.reset(synth.random_rigid(6, rot_range=0.02, trans_range=0.02))
    sums = torch.zeros(32, dtype=torch.float64, device="cuda")
    lp.shard_nn(0, None)
    lp.shard_terms(0, None, None, sums)
    got = sums.cpu().numpy()
    Q = lp.points().cpu().numpy()
    j = lp.correspondences().cpu().numpy()
    m = j >= 0
    assert 100 < m.sum() == got[28]
    Q, q, n = Q[m], tgt[j[m]], nrm[j[m]]
    terms = np.zeros((m.sum(), 30))
    terms[:, 28] = 1.0
    terms[:, 29] = ((Q - q) ** 2).sum(axis=1)
    if est == PLANE:
        r = ((Q - q) * n).sum(axis=1)
        J = np.concatenate([np.cross(Q, n), n], axis=1)
        iu = np.triu_indices(6)
        terms[:, :21] = J[:, iu[0]] * J[:, iu[1]]
        terms[:, 21:27] = J * r[:, None]
        terms[:, 27] = r * r
    else:
        pc, qc = Q - c, q - c
        terms[:, 0:3], terms[:, 3:6] = pc, qc
        terms[:, 6:15] = (pc[:, :, None] * qc[:, None, :]).reshape(-1, 9)
    ref, scale = terms.sum(axis=0), np.abs(terms).sum(axis=0)
    err = np.abs(got[:30] - ref)
    print("anchor: worst slot error / sum|term|", (err / np.maximum(scale, 1e-300)).max())
    assert (err <= 1e-12 * scale).all(), (err, scale)


# ------------------------------------------------------------------------------- point-to-plane
LIBM_WORST = []


@pytest.mark.parametrize("case", SC.plane_full_rank(), ids=lambda c: c[0])
def test_plane_update_from_constructed_system(loops, case):
    """A x = b of a chosen solution at every angle scale: the translation column of `update` is
    x[3..5] of the host-compiled hook on the same A and b, bit for bit; at max |angle| ≤ 0.5 the
    whole update is the restated vec6_to_matrix_sc(sincos_small(x)), bit for bit; above 0.5 (the
    libm sincos branch) every rotation entry is within 40·2⁻⁵³ of the 200-bit matrix of x — a device
    sine or cosine within 4 ulp (OpenCL's requirement for double, values ≤ 1: 4·2⁻⁵³ each), every
    entry a difference of two triple products: 2·3·4·2⁻⁵³ from the factors plus the entry's own
    seven roundings, 31·2⁻⁵³, rounded up.  `transformation` is the restated
    matmul4_affine(update, init), bit for bit."""
    name, A, b = case
    x = host_ldlt(A, b)
    big = np.abs(x[:3]).max()
    exact = {"exact_half": 0.5, "exact_above_half": math.nextafter(0.5, 1.0),
             "exact_below_half": math.nextafter(0.5, 0.0), "exact_minus_half": -0.5}
    if name in exact:
        assert x[0] == exact[name] and big == abs(exact[name])
    r = solve_once(loops[PLANE], plane_sums(A, b))
    same(r.update[:3, 3], x[3:6], f"{name}: translation against the host hook")
    same(r.update[3], [0, 0, 0, 1], name)
    if big <= 0.5:
        same(r.update, S.update_small(x), f"{name}: update against the restatement")
    else:
        err = S.mp_max_abs_diff(r.update[:3, :3], S.mp_vec6_rotation(x))
        LIBM_WORST.append(err)
        print(f"{name}: libm branch, worst rotation entry error {err / S.U:.2f} * 2^-53 "
              f"(worst so far {max(LIBM_WORST) / S.U:.2f})")
        assert err <= 40 * S.U, name
    same(r.transformation, S.matmul4_affine(r.update, INIT), f"{name}: transformation")
    assert r.iterations == 1 and r.fitness == 0.5 and r.inlier_rmse == 0.125


@pytest.mark.parametrize("case", SC.plane_singular(), ids=lambda c: c[0])
def test_plane_singular_systems(loops, case):
    """Zero columns of J, A = 0 with count > 0, and a pivot on either side of the unpivoted
    factorisation's fall-back: the solution is the host hook's (the same rule) in every bit, its
    zero components exactly 0.0, and the update the restated matrix of it (A = 0: the identity)."""
    name, A, b, zero = case
    x = host_ldlt(A, b)
    assert all(x[k] == 0.0 for k in zero) and np.abs(x[:3]).max() <= 0.5
    r = solve_once(loops[PLANE], plane_sums(A, b))
    same(r.update[:3, 3], x[3:6], f"{name}: translation against the host hook")
    for k in zero:
        if k >= 3:
            assert r.update[k - 3, 3] == 0.0
    same(r.update, S.update_small(x), f"{name}: update against the restatement")
    if name == "zero_matrix":
        same(r.update, EYE, name)
    same(r.transformation, S.matmul4_affine(r.update, INIT), f"{name}: transformation")
    assert r.iterations == 1


# ------------------------------------------------------------------------------- point-to-point
@pytest.mark.parametrize("case", SC.cov_cases(), ids=lambda c: c[0])
def test_point_rotation_from_constructed_covariance(loops, case):
    """count = 64 and zero first moments: rotation_from_cov sees exactly the chosen H and
    t = c − R·c.  The rotation block of `update` is the host hook's R bit for bit in every case and
    the translation solve_state's formula on it in its order; for rank ≥ 2 and a singular ratio ≤
    1e3 the rotation agrees with the 200-bit one within 4× icp_oracle.umeyama's own error on the
    same H (floor 32·2⁻⁵³); for rank ≤ 1 it is proper orthogonal to 8·2⁻⁵²; a NaN entry and an
    overflowing H leave the identity update and `transformation` unchanged.  (Scale 1e-200: the
    squared entries underflow, H is zero to rotation_from_cov — tests/test_solve_cpu.py.)"""
    name, H, rank, ratio = case
    R, got = host_rotation(H)
    r = solve_once(loops[POINT], point_sums(H))
    same(r.update[:3, :3], R, f"{name}: rotation against the host hook")
    same(r.update[:3, 3], S.p2p_translation(R, np.zeros(3), np.zeros(3), CENTRE), f"{name}: translation")
    same(r.transformation, S.matmul4_affine(r.update, INIT), f"{name}: transformation")
    assert r.iterations == 1
    if got <= 0:
        same(r.update, EYE, name)
        same(r.transformation, INIT, name)
        assert name in ("zero", "scale_1e-200", "scale_1e-320", "scale_1e160", "nan_entry")
    elif rank >= 2 and ratio <= 1e3:
        ref = S.mp_rotation_from_cov(H)
        ed = S.mp_max_abs_diff(r.update[:3, :3], ref)
        eo = S.mp_max_abs_diff(umeyama_rotation(H), ref)
        print(f"{name}: device error {ed:.3e}, umeyama error {eo:.3e}")
        assert ed <= max(4.0 * eo, 32.0 * S.U), name
    else:
        Rd = r.update[:3, :3]
        assert np.abs(Rd @ Rd.T - np.eye(3)).max() <= 8 * 2.0 ** -52 and abs(np.linalg.det(Rd) - 1) <= 8 * 2.0 ** -52


def test_point_translation_with_moments(loops):
    """Non-zero centre and non-zero first moments, a count that is no power of two: H and t follow
    solve_state's expressions in their order, from the host hook's rotation of that H."""
    rng = np.random.default_rng(33)
    n = 48.0
    sp, sq = rng.uniform(-20, 20, 3), rng.uniform(-20, 20, 3)
    M = rng.uniform(-30, 30, (3, 3)) + 40 * SC.rot(rng)
    s = point_sums(np.zeros((3, 3)), count=n, sp=sp, sq=sq)
    s[6:15] = M.reshape(9)
    mp, mq = [float(v) / n for v in sp], [float(v) / n for v in sq]
    H = np.array([[float(M[a, c]) / n - mp[a] * mq[c] for c in range(3)] for a in range(3)])
    R, rank = host_rotation(H)
    assert rank == 2
    r = solve_once(loops[POINT], s)
    same(r.update[:3, :3], R, "rotation")
    same(r.update[:3, 3], S.p2p_translation(R, mp, mq, CENTRE), "translation")
    same(r.transformation, S.matmul4_affine(r.update, INIT), "transformation")


# ------------------------------------------------------------------------------- bookkeeping
def small_system():
    name, A, b = SC.plane_full_rank()[1]
    return A, b, S.update_small(host_ldlt(A, b))


def follow(lp, seq, params, init=INIT):
    """Feed the sums of seq to the device loop and to solve_bookkeeping; after every solve each
    field of result() is the restatement's, and update / transformation follow from whether the
    evaluation applied an update (upds: the update each sums would give)."""
    lp.reset(init)
    st, T, last = S.new_state(), init.copy(), EYE
    for sums, upd in seq:
        st, applied = S.solve_bookkeeping(st, sums, params)
        if applied:
            last = upd
            T = S.matmul4_affine(upd, T)
        r = feed(lp, sums)
        assert (r.fitness, r.inlier_rmse, r.num_correspondences, r.iterations, r.converged) == (
            st["fitness"], st["rmse"], st["count"], st["iters"], bool(st["converged"])), (r, st)
        same(r.update, last, "update")
        same(r.transformation, T, "transformation")
    return st


def test_bookkeeping_fitness_rmse_and_strict_convergence(clouds):
    A, b, upd = small_system()
    s1 = plane_sums(A, b, count=37.0, sd2=3.0)
    # relative_* = 0: |Δ| < 0 never holds — the same sums again and again never converge
    p = dict(relative_fitness=0.0, relative_rmse=0.0, max_iteration=1000, ns=NS)
    st = follow(make_loop(clouds, PLANE, 0.0, 0.0), [(s1, upd)] * 4, p)
    assert st["iters"] == 4 and not st["done"] and st["fitness"] == 37.0 / 64.0 and st["rmse"] == math.sqrt(3.0 / 37.0)
    # a tiny positive threshold: never at the first evaluation, at the second; then frozen —
    # other sums change no field
    p = dict(relative_fitness=1e-300, relative_rmse=1e-300, max_iteration=1000, ns=NS)
    other = plane_sums(2 * A, 3 * b, count=11.0, sd2=7.0)
    st = follow(make_loop(clouds, PLANE, 1e-300, 1e-300), [(s1, upd), (s1, upd), (other, EYE), (s1, upd)], p)
    assert st["converged"] and st["iters"] == 1 and st["evals"] == 2
    # the fitness denominator after set_source_total
    lp = make_loop(clouds, PLANE)
    lp.set_source_total(100)
    st = follow(lp, [(s1, upd)], dict(relative_fitness=-1.0, relative_rmse=-1.0, max_iteration=1000, ns=100))
    assert st["fitness"] == 37.0 / 100.0


@pytest.mark.parametrize("max_iteration", [0, 1, 2])
def test_bookkeeping_max_iteration(clouds, max_iteration):
    """RegistrationICP's loop: max_iteration updates, then one more evaluation that applies none;
    later solves are no-ops."""
    A, b, upd = small_system()
    s1 = plane_sums(A, b)
    p = dict(relative_fitness=-1.0, relative_rmse=-1.0, max_iteration=max_iteration, ns=NS)
    other = plane_sums(2 * A, 3 * b, count=11.0, sd2=7.0)
    st = follow(make_loop(clouds, PLANE, max_iteration=max_iteration), [(s1, upd)] * (max_iteration + 1) + [(other, EYE)], p)
    assert st["done"] and not st["converged"] and st["iters"] == max_iteration and st["evals"] == max_iteration + 1


@pytest.mark.parametrize("est", [PLANE, POINT])
def test_bookkeeping_empty_and_non_finite(loops, est):
    """count = 0: fitness 0, rmse 0, the identity update, iterations advancing.  A NaN in slot 0 (or
    an infinite right-hand side) with a finite count: the identity update, fitness and rmse still
    from slots 28 and 29."""
    A, b, upd = small_system()
    p = dict(relative_fitness=-1.0, relative_rmse=-1.0, max_iteration=1000, ns=NS)
    good = plane_sums(A, b) if est == PLANE else point_sums(SC.cov_cases()[0][1])
    empty = good.copy()
    empty[28] = 0.0
    nan0 = good.copy()
    nan0[0] = np.nan
    inf = good.copy()
    inf[3 if est == POINT else 24] = np.inf
    st = follow(loops[est], [(empty, EYE), (nan0, EYE), (inf, EYE), (empty, EYE)], p)
    assert st["iters"] == 4 and st["fitness"] == 0.0 and st["rmse"] == 0.0 and st["count"] == 0


# ------------------------------------------------------------------------------- points() mid-step
def eigen_transform(T, p):
    """pcd.Transform(T) in Eigen's order (icp.hip q64_of): ((x·R0 + y·R1) + z·R2) + t, no fma."""
    R, t = T[:3, :3], T[:3, 3]
    return ((p[:, 0:1] * R[:, 0] + p[:, 1:2] * R[:, 1]) + p[:, 2:3] * R[:, 2]) + t


@pytest.fixture(scope="module")
def pair2k():
    src, tgt, nrm, _ = synth.icp_pair(2000, seed=34)
    return src, tgt, nrm, Cloud(src), Cloud(tgt, nrm)


@pytest.mark.parametrize("form", ["source_shard", "target_shard"])
@pytest.mark.parametrize("est", [PLANE, POINT])
@pytest.mark.parametrize("nn", ["brute", "grid"])
def test_points_between_terms_and_solve(pair2k, nn, est, form):
    """points() is 'the loop's fp64 points of the last evaluation' at every stage of the shard
    protocol (shard_nn → shard_terms → [all-reduce] → solve): after the first evaluation's terms
    pass, which has written init·source back while the solve has not yet counted the evaluation,
    it is init·source bit for bit (it was init·init·source: off by the init's motion, 0.11 here);
    the solve leaves it; after the second terms pass it is update₁·that.  With an identity init:
    the source itself, then update₁·source."""
    import torch

    src, tgt, nrm, s, t = pair2k
    lp = IcpLoop(s, t, 0.3, estimation=est, relative_fitness=-1, relative_rmse=-1, max_iteration=10, nn=nn)
    sums = torch.zeros(32, dtype=torch.float64, device="cuda")
    dk = torch.empty(len(src), dtype=torch.int64, device="cuda")
    cl = torch.empty(len(src), dtype=torch.int32, device="cuda")

    def evaluate():
        if form == "source_shard":
            lp.shard_nn(0, None)
            lp.shard_terms(0, None, None, sums)
        else:
            lp.shard_nn(0, dk)
            lp.shard_claim(dk, cl)
            lp.shard_terms(0, dk, cl, sums)

    for init in (synth.random_rigid(3, rot_range=0.02, trans_range=0.02), np.eye(4)):
        lp.reset(init)
        p0 = src if np.array_equal(init, np.eye(4)) else eigen_transform(init, src)
        same(lp.points().cpu().numpy(), p0, "before the first evaluation")
        evaluate()
        got = lp.points().cpu().numpy()
        print(f"{nn}/{est}/{form}: after the first terms pass, worst |points - init.source| = {np.abs(got - p0).max():.3e}")
        same(got, p0, "between the first terms pass and its solve")
        assert sums[28].item() > 500
        lp.solve(sums)
        same(lp.points().cpu().numpy(), p0, "after the first solve")
        upd = lp.result().update
        assert not np.array_equal(upd, np.eye(4))
        evaluate()
        same(lp.points().cpu().numpy(), eigen_transform(upd, p0), "after the second terms pass")
        lp.solve(sums)
        same(lp.points().cpu().numpy(), eigen_transform(upd, p0), "after the second solve")


def test_points_after_prepare_steps(pair2k):
    """Capturing a step graph enqueues nothing: points() after reset + prepare_steps is still
    init·source, and the captured steps then run from there as plain steps do."""
    src, tgt, nrm, s, t = pair2k
    init = synth.random_rigid(3, rot_range=0.02, trans_range=0.02)
    a = IcpLoop(s, t, 0.3, relative_fitness=-1, relative_rmse=-1, max_iteration=10, nn="brute")
    b = IcpLoop(s, t, 0.3, relative_fitness=-1, relative_rmse=-1, max_iteration=10, nn="brute")
    a.reset(init)
    a.prepare_steps(3)
    same(a.points().cpu().numpy(), eigen_transform(init, src), "after prepare_steps")
    a.steps(3)
    b.reset(init)
    for _ in range(3):
        b.step()
    same(a.points().cpu().numpy(), b.points().cpu().numpy(), "graph replay against plain steps")
    same(a.result().transformation, b.result().transformation, "transformation")
