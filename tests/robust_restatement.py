"""Open3D's robust kernels inside point-to-plane and Generalized ICP, restated in numpy — TEST
INFRASTRUCTURE ONLY (tests/test_robust_cpu.py, tests/test_gpu_robust.py).

Open3D 0.19 ``RobustKernel.cpp``, ``Registration.cpp`` (ComputeJTJandJTr) and
``GeneralizedICP.cpp`` as the project defines them (include/m3d.h).  The loop, the
exact NN, the LDLT solve and the 6-vector → matrix step are ``icp_oracle``'s, the covariances and
the whitened rows ``gicp_restatement``'s; neither module is changed.

* ``weight(kind, r, k)`` — the six weights in the fp64 operation order the device uses, and
  ``rho(kind, r, k)`` — Open3D's losses ρ, whose ρ'(r)/r the weights are.
* ``robust_plane_terms`` — r = (vs − vt)·nt, J = [vs × nt | nt], JᵀJ = Σ w·J·Jᵀ, Jᵀr = Σ w·J·r,
  Σr² unweighted; ``icp_oracle.point_to_plane_terms`` when every weight is 1, bit for bit.
  ``robust_plane_sums``: the same as the 30 slots with Σ|term| per slot.
* ``robust_gicp_terms`` — ``gicp_restatement.gicp_terms_w`` with each whitened row weighted on its
  own; the same bits when every weight is 1.
* ``registration_icp_robust`` / ``registration_gicp_robust`` — RegistrationICP with those updates,
  ``on_eval`` per evaluation.
* fixtures: the one-evaluation cases with their median-|r| scales, and the outlier loop fixture.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
from scipy.spatial import cKDTree

import gicp_restatement as G
import icp_oracle as I

L2, L1, HUBER, CAUCHY, GM, TUKEY = range(6)  # include/m3d.h M3D_KERNEL_*
KINDS = {"l2": L2, "l1": L1, "huber": HUBER, "cauchy": CAUCHY, "gm": GM, "tukey": TUKEY}
READS_K = (HUBER, CAUCHY, GM, TUKEY)


def weight(kind, r, k=1.0):
    """w(r), elementwise, in exactly the device's fp64 operations (csrc/robust.hip)."""
    r = np.asarray(r, np.float64)
    if kind == L2:
        return np.ones_like(r)
    if kind == L1:
        with np.errstate(divide="ignore"):
            return 1.0 / np.abs(r)
    if kind == HUBER:
        return k / np.maximum(np.abs(r), k)
    if kind == CAUCHY:
        return 1.0 / (1.0 + (r / k) * (r / k))
    if kind == GM:
        return k / ((k + r * r) * (k + r * r))
    if kind == TUKEY:
        t = np.minimum(1.0, np.abs(r / k))
        u = 1.0 - t * t
        return u * u
    raise ValueError(f"unknown kernel kind {kind}")


def rho(kind, r, k=1.0):
    """Open3D's loss ρ(r) (RobustKernel.h): weight(r) = ρ'(r) / r."""
    r = np.asarray(r, np.float64)
    a = np.abs(r)
    if kind == L2:
        return r * r / 2.0
    if kind == L1:
        return a
    if kind == HUBER:
        return np.where(a <= k, r * r / 2.0, k * (a - k / 2.0))
    if kind == CAUCHY:
        return k * k / 2.0 * np.log1p((r / k) ** 2)
    if kind == GM:
        return (r * r / 2.0) / (k + r * r)
    if kind == TUKEY:
        return np.where(a <= k, k * k * (1.0 - (1.0 - (r / k) ** 2) ** 3) / 6.0, k * k / 6.0)
    raise ValueError(f"unknown kernel kind {kind}")


# ----------------------------------------------------------------------------------- point-to-plane
def plane_rows(src_t, tgt, tgt_n, corr):
    """→ (r (m,), J (m, 6)) of the matched pairs, as icp_oracle.point_to_plane_terms forms them."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    vs, vt, nt = src_t[corr[:, 0]], tgt[corr[:, 1]], tgt_n[corr[:, 1]]
    r = np.sum((vs - vt) * nt, axis=1)
    return r, np.concatenate([np.cross(vs, nt), nt], axis=1)


def robust_plane_terms(src_t, tgt, tgt_n, corr, kind=L2, k=1.0):
    """JᵀJ (6×6), Jᵀr (6), Σr² (unweighted) with the rows weighted by w(r)."""
    r, J = plane_rows(src_t, tgt, tgt_n, corr)
    Jw = J * weight(kind, r, k)[:, None]
    if np.array_equal(Jw, J):
        Jw = J  # unit weights: the same array, so numpy's matmul takes the path J.T @ J takes
    return Jw.T @ J, Jw.T @ r, float(r @ r)


def _pack_rows(J, r, w, d2, pairs):
    """Per-pair terms (pairs, 30) of rows J (m, 6), r, w (m,), m = pairs × rows-per-pair."""
    m = len(r)
    rows = m // pairs if pairs else 1
    t = np.zeros((m, 30))
    for s, (a, c) in enumerate(G.UPPER):
        t[:, s] = (w * J[:, a]) * J[:, c]
    for a in range(6):
        t[:, 21 + a] = (w * J[:, a]) * r
    t[:, 27] = r * r
    t = t.reshape(pairs, rows, 30).sum(axis=1)
    t[:, 28] = 1.0
    t[:, 29] = d2
    return t


def robust_plane_sums(src_t, tgt, tgt_n, corr, kind=L2, k=1.0):
    """→ (sums (30,), Σ|term| (30,)) in the device's slot layout."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    if len(corr) == 0:
        return np.zeros(30), np.zeros(30)
    r, J = plane_rows(src_t, tgt, tgt_n, corr)
    t = _pack_rows(J, r, weight(kind, r, k), I.sq_dist(src_t[corr[:, 0]], tgt[corr[:, 1]]), len(corr))
    return t.sum(axis=0), np.abs(t).sum(axis=0)


# ---------------------------------------------------------------------------------- Generalized ICP
def gicp_rows(vs, cov_s, vt, cov_t, corr):
    """Open3D's whitened rows: W = M^(−1/2) by eigh, r = W·d (m, 3), Jw = W·J₀ (m, 3, 6), d²."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    ps, d, M, d2 = G._pairs(vs, cov_s, vt, cov_t, corr, np.float64)
    lam, V = np.linalg.eigh(M)
    W = np.einsum("mik,mk,mjk->mij", V, 1.0 / np.sqrt(lam), V)
    r = np.einsum("mij,mj->mi", W, d)
    Jw = np.einsum("mij,mjc->mic", W, G.jacobian0(ps))
    return r, Jw, d2


def robust_gicp_terms(vs, cov_s, vt, cov_t, corr, kind=L2, k=1.0):
    """gicp_restatement.gicp_terms_w with the weight w(r_j) on each of the three rows → sums (30,)."""
    r, Jw, d2 = gicp_rows(vs, cov_s, vt, cov_t, corr)
    w = weight(kind, r, k)
    Jl = Jw * w[:, :, None]
    if np.array_equal(Jl, Jw):
        Jl = Jw
    t = G._pack(np.einsum("mia,mic->mac", Jl, Jw), np.einsum("mia,mi->ma", Jl, r), np.einsum("mi,mi->m", r, r), d2)
    return t.sum(axis=0)


def robust_gicp_sums(vs, cov_s, vt, cov_t, corr, kind=L2, k=1.0):
    """→ (sums (30,), Σ|term| (30,)): the scale of the device comparison, per weighted row."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    if len(corr) == 0:
        return np.zeros(30), np.zeros(30)
    r, Jw, d2 = gicp_rows(vs, cov_s, vt, cov_t, corr)
    rr = r.reshape(-1)
    t = _pack_rows(Jw.reshape(-1, 6), rr, weight(kind, rr, k), d2, len(corr))
    return robust_gicp_terms(vs, cov_s, vt, cov_t, corr, kind, k), np.abs(t).sum(axis=0)


# ------------------------------------------------------------------------------------------ loops
def _solve(sums_or_system):
    A, b = sums_or_system
    return I.vec6_to_matrix(I.ldlt_solve(np.asarray(A, np.float64), -np.asarray(b, np.float64)))


def _loop(src, tgt, max_dist, init, update, moved, relative_fitness, relative_rmse, max_iteration, on_eval):
    """RegistrationICP (icp_oracle.registration_icp's loop) around update(pcd, corr) → ΔT;
    moved(ΔT) is told of every transform the points take (the covariances follow it)."""
    if max_dist <= 0:
        raise ValueError("Invalid max_correspondence_distance.")
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    tree = cKDTree(tgt) if len(tgt) else None
    pcd = I.initial_points(T, src)
    if not I.is_identity(T):
        moved(T)

    def evaluate(k):
        if tree is None:
            fit, rmse, corr = 0.0, 0.0, np.zeros((0, 2), np.int64)
        else:
            fit, rmse, corr, _ = I.registration_result(pcd, tgt, max_dist, tree)
        if on_eval is not None:
            j = np.full(len(pcd), -1, np.int64)
            j[corr[:, 0]] = corr[:, 1]
            on_eval(k, pcd, j)
        return fit, rmse, corr

    fit, rmse, corr = evaluate(0)
    it, converged = 0, False
    while it < max_iteration:
        upd = np.eye(4) if len(corr) == 0 else update(pcd, corr)
        T = I.matmul4(upd, T)
        pcd = I.transform_points(upd, pcd)
        moved(upd)
        it += 1
        bfit, brmse = fit, rmse
        fit, rmse, corr = evaluate(it)
        if abs(bfit - fit) < relative_fitness and abs(brmse - rmse) < relative_rmse:
            converged = True
            break
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, correspondence_set=corr, iterations=it,
                converged=converged)


def registration_icp_robust(src, tgt, tgt_n, max_dist, init=None, kind=L2, k=1.0, relative_fitness=1e-6,
                            relative_rmse=1e-6, max_iteration=30, on_eval=None):
    """registration_icp with TransformationEstimationPointToPlane(kernel)."""
    def update(pcd, corr):
        JTJ, JTr, _ = robust_plane_terms(pcd, tgt, tgt_n, corr, kind, k)
        return _solve((JTJ, JTr))

    return _loop(src, tgt, max_dist, init, update, lambda upd: None, relative_fitness, relative_rmse,
                 max_iteration, on_eval)


def registration_gicp_robust(src, tgt, max_dist, init=None, src_cov=None, tgt_cov=None, kind=L2, k=1.0,
                             relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, on_eval=None):
    """registration_generalized_icp with TransformationEstimationForGeneralizedICP(ε, kernel)."""
    cov = [np.asarray(src_cov, np.float64).copy()]

    def moved(upd):
        cov[0] = G.rotate_covariances(upd[:3, :3], cov[0])

    def update(pcd, corr):
        return _solve(G.sums_to_system(robust_gicp_terms(pcd, cov[0], tgt, tgt_cov, corr, kind, k)))

    return _loop(src, tgt, max_dist, init, update, moved, relative_fitness, relative_rmse, max_iteration, on_eval)


# --------------------------------------------------------------------------------------- fixtures
EVAL_NS = (1, 255, 257, 1000)  # one lane, a block edge, a ragged second block, some sources unmatched
EVAL_NT, EVAL_SEED = 777, 3


@lru_cache(maxsize=None)
def eval_case(ns):
    """A one-evaluation case at a non-identity T_host (gicp_restatement.bumpy_pair's geometry,
    radius G.RADIUS): clouds, the moved points and covariances, the exact correspondences, and per
    estimator the scale k = the median |r| over the restatement's matched pairs (whitened rows for
    Generalized ICP) — so that both branches of Huber and Tukey are taken."""
    src, sn, tgt, tn, T = G.bumpy_pair(ns, EVAL_NT, EVAL_SEED)
    cs, ct = G.covariances_from_normals(sn, G.EPS), G.covariances_from_normals(tn, G.EPS)
    pcd = I.initial_points(T, src)
    csr = G.rotate_covariances(T[:3, :3], cs)
    _, _, corr, _ = I.registration_result(pcd, tgt, G.RADIUS)
    j = np.full(ns, -1, np.int64)
    j[corr[:, 0]] = corr[:, 1]
    r_plane = plane_rows(pcd, tgt, tn, corr)[0]
    r_gicp = gicp_rows(pcd, csr, tgt, ct, corr)[0].reshape(-1)
    for a in (src, sn, tgt, tn, pcd, csr, ct, corr, j):
        a.setflags(write=False)
    return dict(src=src, sn=sn, tgt=tgt, tn=tn, T=T, pcd=pcd, cs=csr, ct=ct, corr=corr, j=j, r_plane=r_plane,
                r_gicp=r_gicp, k_plane=float(np.median(np.abs(r_plane))), k_gicp=float(np.median(np.abs(r_gicp))))


LOOP_SEED = 45  # the first seed from 31 up at which all four L2 loops converge within 30 iterations
OUTLIER_SHARE = 0.15           # of the source, pushed off the surface along its normal
OUTLIER_PUSH = (0.10, 0.25)    # inside G.LOOP_RADIUS = 0.3: the pushed points still match
TUKEY_C, HUBER_C = 4.685, 1.345  # the usual tuning constants, times the clean points' σ


def pose_error(T, T_true, pts):
    """RMS distance between T·pts and T_true·pts."""
    d = I.transform_points(T, pts) - I.transform_points(T_true, pts)
    return float(np.sqrt(np.mean(np.sum(d * d, axis=1))))


@lru_cache(maxsize=None)
def outlier_pair():
    """gicp_restatement.bumpy_pair(2000, 2000) with OUTLIER_SHARE of the source pushed along its
    normal by OUTLIER_PUSH, and the kernels' scales from the clean points' residuals at T_true:
    σ = 1.4826·median|r|, k = TUKEY_C·σ or HUBER_C·σ, per estimator."""
    src, sn, tgt, tn, T = G.bumpy_pair(2000, 2000, LOOP_SEED)
    rng = np.random.default_rng(LOOP_SEED + 9)
    out = np.zeros(len(src), bool)
    out[rng.permutation(len(src))[: round(OUTLIER_SHARE * len(src))]] = True
    src = src + (out * rng.uniform(*OUTLIER_PUSH, len(src)))[:, None] * sn
    cs, ct = G.covariances_from_normals(sn, G.EPS), G.covariances_from_normals(tn, G.EPS)
    pcd = I.transform_points(T, src)
    _, _, corr, _ = I.registration_result(pcd, tgt, G.LOOP_RADIUS)
    clean = corr[~out[corr[:, 0]]]
    sig_p = 1.4826 * np.median(np.abs(plane_rows(pcd, tgt, tn, clean)[0]))
    sig_g = 1.4826 * np.median(np.abs(gicp_rows(pcd, G.rotate_covariances(T[:3, :3], cs), tgt, ct, clean)[0]))
    for a in (src, sn, tgt, tn, cs, ct, out):
        a.setflags(write=False)
    return dict(src=src, sn=sn, tgt=tgt, tn=tn, cs=cs, ct=ct, T_true=T, outlier=out,
                k={("plane", TUKEY): TUKEY_C * sig_p, ("plane", HUBER): HUBER_C * sig_p,
                   ("gicp", TUKEY): TUKEY_C * sig_g, ("gicp", HUBER): HUBER_C * sig_g})


@lru_cache(maxsize=None)
def loop_case(est, kind, init_kind):
    """The restatement's run of estimator ``est`` ("plane" / "gicp") with kernel ``kind`` (L2:
    no kernel) from init ``init_kind`` ("identity" / "perturbed", gicp_restatement.loop_init) on
    the outlier fixture, every evaluation recorded — computed once per session, never modified.
    → dict(init, k, ref, evals = [(pcd, j)])."""
    f = outlier_pair()
    init = G.loop_init(init_kind)
    k = f["k"].get((est, kind), 1.0)
    evals = []

    def on_eval(_, pcd, j):
        evals.append((pcd.copy(), j.copy()))

    if est == "plane":
        ref = registration_icp_robust(f["src"], f["tgt"], f["tn"], G.LOOP_RADIUS, init, kind, k, on_eval=on_eval)
    else:
        ref = registration_gicp_robust(f["src"], f["tgt"], G.LOOP_RADIUS, init, f["cs"], f["ct"], kind, k,
                                       on_eval=on_eval)
    return dict(init=init, k=k, ref=ref, evals=evals)
