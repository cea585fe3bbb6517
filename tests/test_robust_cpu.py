"""The robust-kernel restatement (tests/robust_restatement.py) and linalg.h's ``sym3_eigen``
(through its host hook) on the CPU: the weights against Open3D's losses, the L2 identities, the
eigendecomposition's bounds, W = M^(−1/2) against LAPACK, and the conditions the fixtures of
tests/test_gpu_robust.py must meet."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import gicp_restatement as G
import icp_oracle as I
import matcher
import robust_restatement as R
from m3d import _lib

U = 2.0 ** -52
P = C.POINTER(C.c_double)


# ------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("kind", sorted(R.KINDS.values()))
@pytest.mark.parametrize("k", [0.3, 2.0])
def test_weight_is_rho_prime_over_r(kind, k):
    """w(r) = ρ'(r) / r, ρ' by central differences with h = 1e-6·k: truncation ≈ h²·ρ'''/6 and
    rounding ≈ u·ρ/h are both below 1e-9 of ρ' here; asserted at 1e-7 relative.  r on both sides
    of k and of both signs, away from the kinks of ρ'' at |r| = k (and of L1 at 0)."""
    r = np.concatenate([f * k * np.array([0.05, 0.3, 0.7, 0.95, 1.05, 1.5, 3.0, 8.0]) for f in (1.0, -1.0)])
    h = 1e-6 * k
    ref = (R.rho(kind, r + h, k) - R.rho(kind, r - h, k)) / (2.0 * h) / r
    got = R.weight(kind, r, k)
    print(kind, k, "worst |w - rho'/r|:", np.abs(got - ref).max())
    np.testing.assert_allclose(got, ref, rtol=1e-7, atol=1e-7 * np.abs(ref).max())
    if kind == R.TUKEY:
        assert (got[np.abs(r) > k] == 0.0).all() and (got[np.abs(r) < k] > 0.0).all()
    if kind == R.HUBER:
        assert (got[np.abs(r) < k] == 1.0).all() and (got[np.abs(r) > k] < 1.0).all()


def test_public_classes_carry_the_same_weights():
    r = np.linspace(-3.0, 3.0, 61) + 1e-3
    cls = {R.L2: matcher.L2Loss(), R.L1: matcher.L1Loss(), R.HUBER: matcher.HuberLoss(0.7),
           R.CAUCHY: matcher.CauchyLoss(0.7), R.GM: matcher.GMLoss(0.7), R.TUKEY: matcher.TukeyLoss(0.7)}
    for kind, obj in cls.items():
        assert obj.kind == kind
        np.testing.assert_array_equal(obj.weight(r), R.weight(kind, r, 0.7))
        if kind in R.READS_K:
            assert obj.k == 0.7
    assert (_lib.ROBUST_L2, _lib.ROBUST_L1, _lib.ROBUST_HUBER, _lib.ROBUST_CAUCHY, _lib.ROBUST_GM,
            _lib.ROBUST_TUKEY) == (R.L2, R.L1, R.HUBER, R.CAUCHY, R.GM, R.TUKEY)
    assert np.isinf(matcher.L1Loss().weight(0.0))


def test_kernel_with_point_to_point_is_rejected_without_a_device():
    pts = np.zeros((4, 3))
    with pytest.raises(ValueError):
        matcher.registration_icp(pts, pts, 0.5, estimation="point_to_point", kernel=matcher.TukeyLoss(0.1))


# ------------------------------------------------------------------------------- L2 identities
@pytest.mark.parametrize("ns", [n for n in R.EVAL_NS if n > 1])
def test_l2_is_the_unweighted_estimator_bit_for_bit(ns):
    c = R.eval_case(ns)
    a = I.point_to_plane_terms(c["pcd"], c["tgt"], c["tn"], c["corr"])
    b = R.robust_plane_terms(c["pcd"], c["tgt"], c["tn"], c["corr"], R.L2)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    assert a[2] == b[2]
    g = G.gicp_terms_w(c["pcd"], c["cs"], c["tgt"], c["ct"], c["corr"])
    np.testing.assert_array_equal(g, R.robust_gicp_terms(c["pcd"], c["cs"], c["tgt"], c["ct"], c["corr"], R.L2))
    # and the 30-slot form the device is compared with is the same system
    s, scale = R.robust_plane_sums(c["pcd"], c["tgt"], c["tn"], c["corr"], R.L2)
    A, rhs = G.sums_to_system(s)
    assert np.all(np.abs(A - a[0]) <= 1e-13 * G.sums_to_system(scale)[0]) and np.all(np.abs(rhs - a[1]) <= 1e-13 * scale[21:27])
    s, scale = R.robust_gicp_sums(c["pcd"], c["cs"], c["tgt"], c["ct"], c["corr"], R.L2)
    assert np.all(np.abs(s - g) <= 1e-13 * scale)


# ---------------------------------------------------------------------------------- sym3_eigen
def _sym6(A):
    return np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]], np.float64)


def eigen(A):
    lam, V = np.zeros(3), np.zeros(9)
    assert _lib.load().m3d_debug_sym3_eigen_host(_sym6(A).ctypes.data_as(P), lam.ctypes.data_as(P),
                                                 V.ctypes.data_as(P)) == 0
    return lam, V.reshape(3, 3)


def eigenvalues(A):
    lam = np.zeros(3)
    assert _lib.load().m3d_debug_sym3_eigenvalues_host(_sym6(A).ctypes.data_as(P), lam.ctypes.data_as(P)) == 0
    return lam


SPD_KINDS = ("spd", "cov2", "repeated", "diag")


def sym3_cases():
    rng = np.random.default_rng(41)
    out = []
    for _ in range(300):  # SPD, condition up to 1e6
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = 10.0 ** rng.uniform(-6, 0, 3) * rng.uniform(0.5, 2.0)
        A = (Q * lam) @ Q.T
        out.append(("spd", 0.5 * (A + A.T)))
    n = rng.standard_normal((600, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    cov = G.covariances_from_normals(n, 1e-3)  # what Generalized ICP feeds: M = Ct + Cs
    out += [("cov2", cov[2 * i] + cov[2 * i + 1]) for i in range(299)]
    out.append(("cov2", cov[0] + cov[0]))  # equal normals: (2ε, 2, 2)
    N = np.array([[1.0, 2.0, 2.0], [2.0, 4.0, 4.0], [2.0, 4.0, 4.0]])  # 9·n·nᵀ, n = (1, 2, 2) / 3
    for b, m in ((1.0, 1.0), (7.0, -0.5), (0.25, 3.0), (3.0, 0.0)):
        out.append(("repeated", b * np.eye(3) + m * N))  # exactly (b, b, b + 9m), off the axes
    for d in ((2.0, 2.0, 5.0), (5.0, 2.0, 2.0), (2.0, 5.0, 2.0), (3.0, 3.0, 3.0), (1e-3, 1.0, 1.0)):
        out.append(("diag", np.diag(d)))
    out += [("diag", np.diag(rng.uniform(0.1, 3.0, 3))) for _ in range(20)]
    out.append(("zero", np.zeros((3, 3))))
    return out


def w_deviation(A):
    """‖W − W_ref‖ / ‖W_ref‖, W = V·diag(1/√λ)·Vᵀ from the hook's pairs, W_ref from eigh's."""
    lam, V = eigen(A)
    rl, RV = np.linalg.eigh(A)
    W, Wr = (V / np.sqrt(lam)) @ V.T, (RV / np.sqrt(rl)) @ RV.T
    return np.linalg.norm(W - Wr) / np.linalg.norm(Wr)


# V is a product of plane rotations, three per sweep and at most five sweeps in practice, each
# orthogonal to about one ulp: 16 u bounds both ‖VᵀV − I‖max and ‖V·diag(λ)·Vᵀ − A‖max / ‖A‖₂.
# Measured over sym3_cases(): 6.0 u and 4.6 u (tests/test_iss_cpu.py holds sym3_eigenvalues
# itself to 4 u against LAPACK; the eigenvalues here are those bits).
EIGEN_ULPS = 16
# Measured over the positive definite cases: the largest ‖W − W_ref‖ / ‖W_ref‖ is W_MEASURED, on a
# random SPD case of condition ≈ 1e6 — λmin carries an error of u·λmax from either method, so W
# moves by ≈ κ·u; the sums of two (ε, 1, 1) covariances (κ ≤ 1e3) reach 6.9e-14, the exactly
# repeated eigenvalues 1.0e-14.  Asserted at 16 times the measurement.
W_MEASURED = 6.6e-11
W_BOUND = 16 * W_MEASURED


def test_sym3_eigen_bounds():
    worst_o = worst_r = 0.0
    for kind, A in sym3_cases():
        lam, V = eigen(A)
        np.testing.assert_array_equal(lam, eigenvalues(A), err_msg=kind)  # the same rotations: the same bits
        assert (np.diff(lam) >= 0).all(), kind
        norm = np.linalg.norm(A, 2)
        o, r = np.abs(V.T @ V - np.eye(3)).max(), np.abs((V * lam) @ V.T - A).max()
        worst_o, worst_r = max(worst_o, o / U), max(worst_r, r / (U * norm) if norm else 0.0)
        assert o <= EIGEN_ULPS * U, (kind, A)
        assert r <= EIGEN_ULPS * U * norm, (kind, A)
        if kind in ("diag", "zero"):
            np.testing.assert_array_equal(lam, np.sort(np.diag(A)))
            assert sorted(np.abs(V).ravel()) == [0.0] * 6 + [1.0] * 3  # a permutation: no rotation ran
    print(f"sym3_eigen: worst |VtV - I| {worst_o:.2f} u, worst |V lam Vt - A| {worst_r:.2f} u |A|")


def test_inverse_square_root_against_lapack():
    worst = {}
    for kind, A in sym3_cases():
        if kind in SPD_KINDS:
            worst[kind] = max(worst.get(kind, 0.0), w_deviation(A))
    print("W = M^(-1/2): worst relative deviation per kind", worst)
    assert max(worst.values()) <= W_BOUND
    # the symmetric root is unique: repeated eigenvalues must not inflate the deviation
    assert worst["repeated"] <= max(worst["spd"], worst["cov2"])


# ------------------------------------------------------------------------- fixture conditions
@pytest.mark.parametrize("ns", R.EVAL_NS)
def test_one_evaluation_fixtures(ns):
    c = R.eval_case(ns)
    assert not I.is_identity(c["T"])
    assert len(c["corr"]) == (c["j"] >= 0).sum() >= 1
    if ns == 1000:
        assert len(c["corr"]) < ns  # some sources unmatched
    if ns == 1:  # one pair: k = |r| itself for point-to-plane, the Huber / Tukey boundary
        assert c["k_plane"] == abs(c["r_plane"][0])
        return
    for r, k in ((c["r_plane"], c["k_plane"]), (c["r_gicp"], c["k_gicp"])):
        above = (np.abs(r) > k).mean()
        assert 0.25 <= above <= 0.75  # Huber's and Tukey's two branches are both taken
        assert np.abs(r).min() > 0.0  # no L1 weight is infinite


LOOPS = [(est, kind, init) for est in ("plane", "gicp") for kind in (R.L2, R.TUKEY, R.HUBER)
         for init in ("identity", "perturbed")]


@pytest.mark.parametrize("est,kind,init", LOOPS)
def test_loop_fixture_has_no_near_ties(est, kind, init):
    """As tests/test_gicp_cpu.py for the Generalized ICP loop fixture: at every evaluation of the
    restatement every source's best and second-best d² differ by more than 1e-9, and its best d²
    is farther than that from r² — a device run whose points differ by rounding (≈1e-15) picks the
    same correspondences."""
    f, c = R.outlier_pair(), R.loop_case(est, kind, init)
    tree = cKDTree(f["tgt"])
    assert 2 <= len(c["evals"]) <= 31
    gap = edge = np.inf
    for pcd, j in c["evals"]:
        _, jj = tree.query(pcd, k=2)
        d0, d1 = I.sq_dist(pcd, f["tgt"][jj[:, 0]]), I.sq_dist(pcd, f["tgt"][jj[:, 1]])
        gap, edge = min(gap, np.abs(d1 - d0).min()), min(edge, np.abs(np.minimum(d0, d1) - G.LOOP_RADIUS ** 2).min())
        assert 0.5 < (j >= 0).mean() < 1.0
    print(f"{est} {kind} {init}: evaluations {len(c['evals'])}, converged {c['ref']['converged']}, "
          f"smallest d2 gap {gap:.3e}, to r2 {edge:.3e}")
    assert gap > 1e-9 and edge > 1e-9


@pytest.mark.parametrize("est", ["plane", "gicp"])
@pytest.mark.parametrize("init", ["identity", "perturbed"])
def test_loop_fixture_outliers_bias_l2_and_tukey_resists(est, init):
    f = R.outlier_pair()
    assert f["outlier"].sum() == round(R.OUTLIER_SHARE * len(f["src"]))
    # the pushed points still match at the true pose: the radius does not remove them
    _, _, corr, _ = I.registration_result(I.transform_points(f["T_true"], f["src"]), f["tgt"], G.LOOP_RADIUS)
    j = np.full(len(f["src"]), -1)
    j[corr[:, 0]] = corr[:, 1]
    assert (j[f["outlier"]] >= 0).mean() > 0.5 and f["outlier"][corr[:, 0]].mean() > 0.1
    clean = f["src"][~f["outlier"]]
    l2, tukey = R.loop_case(est, R.L2, init)["ref"], R.loop_case(est, R.TUKEY, init)["ref"]
    assert l2["converged"] and l2["iterations"] <= 30
    e_l2, e_tukey = (R.pose_error(x["transformation"], f["T_true"], clean) for x in (l2, tukey))
    print(f"{est} {init}: pose error L2 {e_l2:.4e}, Tukey {e_tukey:.4e}, ratio {e_tukey / e_l2:.3f}; "
          f"L2 iterations {l2['iterations']}, Tukey {tukey['iterations']}")
    assert e_tukey <= 0.5 * e_l2
