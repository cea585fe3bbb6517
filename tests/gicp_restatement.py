"""Generalized ICP restated in numpy — TEST INFRASTRUCTURE ONLY (tests/test_gicp_cpu.py,
tests/test_gpu_gicp.py).

Open3D 0.19 ``pipelines/registration/GeneralizedICP.cpp`` as the project defines it
(include/m3d.h); the loop around the update is ``icp_oracle.registration_icp``'s,
whose pieces (exact NN, LDLT solve, 6-vector → matrix, Eigen-order products) are imported.

* ``rotation_e1_to_x(n)`` — GetRotationFromE1ToX: v = e1 × n, c = e1·n; I when c < −0.99, else
  I + [v]× + [v]×²·(1 / (1 + c)).
* ``covariances_from_normals`` — C = Rx·diag(ε, 1, 1)·Rxᵀ; the upper triangle is computed,
  ((ε·R_i0)·R_j0 + R_i1·R_j1) + R_i2·R_j2, and mirrored: exactly symmetric.
* ``rotate_covariances(R, C)`` — PointCloud::Transform on covariances, C ← R·C·Rᵀ: A = R·C, the
  upper triangle of A·Rᵀ, mirrored.
* ``gicp_terms`` — per correspondence d = vs − vt, M = Ct + Cs, B = M⁻¹ (cofactors over the
  determinant), J₀ = [−[vs]× | I]; the 30 sums Σ J₀ᵀ·B·J₀ (upper triangle, row-major), Σ J₀ᵀ·B·d,
  Σ dᵀ·B·d, count, Σd², and per slot Σ|term|.  ``gicp_terms_w`` is Open3D's own form: residual
  rows W·d and Jacobian rows W·J₀ with W = M^(−1/2) from ``eigh``.
* ``registration_generalized_icp`` — RegistrationICP with that update; every update moves the
  points and rotates the source covariances; ``on_eval(k, pcd, j, cov)`` per evaluation.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
from scipy.spatial import cKDTree

import icp_oracle as I

UPPER = [(a, c) for a in range(6) for c in range(a, 6)]  # slot → (row, column) of JᵀJ


def rotation_e1_to_x(n):
    n = np.asarray(n, np.float64)
    v = np.cross([1.0, 0.0, 0.0], n)
    c = n[0]
    if c < -0.99:
        return np.eye(3)
    K = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return np.eye(3) + K + (K @ K) * (1.0 / (1.0 + c))


def _mirror(up):
    """(n, 6) upper triangles (xx, xy, xz, yy, yz, zz) → (n, 3, 3) symmetric."""
    C = np.empty((len(up), 3, 3), up.dtype)
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        C[:, i, j] = C[:, j, i] = up[:, k]
    return C


def covariances_from_normals(normals, epsilon=1e-3):
    nrm = np.asarray(normals, np.float64).reshape(-1, 3)
    R = np.array([rotation_e1_to_x(v) for v in nrm]).reshape(-1, 3, 3)
    up = np.stack([((epsilon * R[:, i, 0]) * R[:, j, 0] + R[:, i, 1] * R[:, j, 1]) + R[:, i, 2] * R[:, j, 2]
                   for i in range(3) for j in range(i, 3)], axis=1).reshape(-1, 6)
    return _mirror(up)


def rotate_covariances(R, C):
    R = np.asarray(R, C.dtype)
    A = np.empty_like(C)
    for a in range(3):
        for b in range(3):
            A[:, a, b] = (R[a, 0] * C[:, 0, b] + R[a, 1] * C[:, 1, b]) + R[a, 2] * C[:, 2, b]
    up = np.stack([(A[:, a, 0] * R[b, 0] + A[:, a, 1] * R[b, 1]) + A[:, a, 2] * R[b, 2]
                   for a in range(3) for b in range(a, 3)], axis=1).reshape(-1, 6)
    return _mirror(up)


def inverse_sym3(M):
    """Closed-form inverse of (m, 3, 3) symmetric matrices: cofactors times 1 / det."""
    a, b, c = M[:, 0, 0], M[:, 0, 1], M[:, 0, 2]
    d, e, f = M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]
    co = np.stack([d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b], axis=1)
    rdet = 1.0 / ((a * co[:, 0] + b * co[:, 1]) + c * co[:, 2])
    return _mirror(co * rdet[:, None])


def jacobian0(vs):
    """J₀ = [−[vs]× | I], (m, 3, 6)."""
    m = len(vs)
    x, y, z = vs[:, 0], vs[:, 1], vs[:, 2]
    J = np.zeros((m, 3, 6), vs.dtype)
    J[:, 0, 1], J[:, 0, 2] = z, -y
    J[:, 1, 0], J[:, 1, 2] = -z, x
    J[:, 2, 0], J[:, 2, 1] = y, -x
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = 1.0
    return J


def _pack(JTJ, JTr, r2, d2):
    m = len(r2)
    t = np.empty((m, 30), JTJ.dtype)
    for k, (a, c) in enumerate(UPPER):
        t[:, k] = JTJ[:, a, c]
    t[:, 21:27] = JTr
    t[:, 27] = r2
    t[:, 28] = 1.0
    t[:, 29] = d2
    return t


def _pairs(vs, cov_s, vt, cov_t, corr, dtype):
    ci, cj = corr[:, 0], corr[:, 1]
    ps, pt = np.asarray(vs, dtype)[ci], np.asarray(vt, dtype)[cj]
    M = np.asarray(cov_t, dtype)[cj] + np.asarray(cov_s, dtype)[ci]
    d = ps - pt
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return ps, d, M, d2


def gicp_terms(vs, cov_s, vt, cov_t, corr, dtype=np.float64):
    """→ (sums (30,), abs_sums (30,) = Σ|term| per slot) in ``dtype``, the M⁻¹ form."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    if len(corr) == 0:
        return np.zeros(30, dtype), np.zeros(30, dtype)
    ps, d, M, d2 = _pairs(vs, cov_s, vt, cov_t, corr, dtype)
    B = inverse_sym3(M)
    J = jacobian0(ps)
    G = np.einsum("mrk,mkc->mrc", B, J)
    w = np.einsum("mrk,mk->mr", B, d)
    t = _pack(np.einsum("mra,mrc->mac", J, G), np.einsum("mra,mr->ma", J, w), np.einsum("mr,mr->m", d, w), d2)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def gicp_terms_w(vs, cov_s, vt, cov_t, corr):
    """Open3D's form: residual rows W·d, Jacobian rows W·J₀, W = M^(−1/2) by eigh → sums (30,)."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    ps, d, M, d2 = _pairs(vs, cov_s, vt, cov_t, corr, np.float64)
    lam, V = np.linalg.eigh(M)
    W = np.einsum("mik,mk,mjk->mij", V, 1.0 / np.sqrt(lam), V)
    r = np.einsum("mij,mj->mi", W, d)
    Jw = np.einsum("mij,mjc->mic", W, jacobian0(ps))
    t = _pack(np.einsum("mia,mic->mac", Jw, Jw), np.einsum("mia,mi->ma", Jw, r), np.einsum("mi,mi->m", r, r), d2)
    return t.sum(axis=0)


def sums_to_system(sums):
    A = np.zeros((6, 6))
    for k, (a, c) in enumerate(UPPER):
        A[a, c] = A[c, a] = sums[k]
    return A, np.asarray(sums[21:27], np.float64)


def gicp_update(pcd, cov_s, tgt, cov_t, corr):
    """ComputeTransformation: the identity for an empty set, else solve JᵀJ·x = −Jᵀr."""
    if len(corr) == 0:
        return np.eye(4)
    sums, _ = gicp_terms(pcd, cov_s, tgt, cov_t, corr)
    A, b = sums_to_system(sums)
    return I.vec6_to_matrix(I.ldlt_solve(A, -b))


def registration_generalized_icp(src, tgt, max_dist, init=None, src_cov=None, tgt_cov=None,
                                 relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30, on_eval=None):
    """RegistrationICP with the plane-to-plane update.  Returns dict(transformation, fitness,
    inlier_rmse, correspondence_set, iterations, converged, covariances)."""
    if max_dist <= 0:
        raise ValueError("Invalid max_correspondence_distance.")
    src = np.asarray(src, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    tree = cKDTree(tgt) if len(tgt) else None
    pcd = I.initial_points(T, src)
    cov = np.asarray(src_cov, np.float64).copy()
    if not I.is_identity(T):
        cov = rotate_covariances(T[:3, :3], cov)

    def evaluate(k):
        if tree is None:
            fit, rmse, corr = 0.0, 0.0, np.zeros((0, 2), np.int64)
        else:
            fit, rmse, corr, _ = I.registration_result(pcd, tgt, max_dist, tree)
        if on_eval is not None:
            j = np.full(len(pcd), -1, np.int64)
            j[corr[:, 0]] = corr[:, 1]
            on_eval(k, pcd, j, cov)
        return fit, rmse, corr

    fit, rmse, corr = evaluate(0)
    it, converged = 0, False
    while it < max_iteration:
        upd = gicp_update(pcd, cov, tgt, tgt_cov, corr)
        T = I.matmul4(upd, T)
        pcd = I.transform_points(upd, pcd)
        cov = rotate_covariances(upd[:3, :3], cov)
        it += 1
        bfit, brmse = fit, rmse
        fit, rmse, corr = evaluate(it)
        if abs(bfit - fit) < relative_fitness and abs(brmse - rmse) < relative_rmse:
            converged = True
            break
    return dict(transformation=T, fitness=fit, inlier_rmse=rmse, correspondence_set=corr, iterations=it,
                converged=converged, covariances=cov)


# ------------------------------------------------------------------------------------ fixtures
RADIUS = 0.8        # one-evaluation cases (nt = 777: some sources unmatched)
LOOP_RADIUS = 0.3   # loop cases (2,000 targets: some sources unmatched)
EPS = 1e-3


def bumpy_pair(ns, nt, seed, noise=0.01):
    """Two noisy samplings of the synthetic bumpy surface with unit normals and a known pose:
    → (src, src_normals, tgt, tgt_normals, T_true), T_true·src ≈ tgt's surface."""
    from m3d import synth

    tgt, tn = synth.surface_points(nt, seed)
    sw, sn = synth.surface_points(ns, seed + 100)
    rng = np.random.default_rng(seed + 5)
    tgt = tgt + noise * rng.standard_normal(tgt.shape)
    sw = sw + noise * rng.standard_normal(sw.shape)
    T = synth.random_rigid(seed + 1, center=tgt.mean(axis=0) if nt else None, rot_range=np.pi / 60, trans_range=0.05)
    Ti = np.linalg.inv(T)
    return (np.ascontiguousarray(synth.apply(Ti, sw)), np.ascontiguousarray(sn @ Ti[:3, :3].T), tgt, tn, T)


LOOP_SEED = 31


def loop_init(kind):
    from m3d import synth

    return np.eye(4) if kind == "identity" else synth.random_rigid(77, rot_range=0.01, trans_range=0.02)


@lru_cache(maxsize=None)
def loop_case(kind):
    """The 2,000 ↔ 2,000 loop fixture with init ``kind`` ("identity" / "perturbed"): its clouds,
    covariances and the restatement's run with every evaluation recorded — computed once per
    session and never modified.  → dict(src, sn, tgt, tn, T_true, init, cs, ct, ref, evals) with
    evals = [(pcd, j)] per evaluation."""
    src, sn, tgt, tn, T = bumpy_pair(2000, 2000, LOOP_SEED)
    cs, ct = covariances_from_normals(sn, EPS), covariances_from_normals(tn, EPS)
    init = loop_init(kind)
    evals = []
    ref = registration_generalized_icp(src, tgt, LOOP_RADIUS, init, cs, ct,
                                       on_eval=lambda k, pcd, j, cov: evals.append((pcd.copy(), j.copy())))
    for a in (src, sn, tgt, tn, cs, ct):
        a.setflags(write=False)
    return dict(src=src, sn=sn, tgt=tgt, tn=tn, T_true=T, init=init, cs=cs, ct=ct, ref=ref, evals=evals)
