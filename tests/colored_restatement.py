"""Colored ICP restated in numpy — TEST INFRASTRUCTURE ONLY (tests/test_colored_cpu.py,
tests/test_gpu_colored.py).

Open3D 0.19 ``pipelines/registration/ColoredICP.cpp`` as the project defines it (include/m3d.h,
DESIGN §3.19).  The loop, the exact NN, the LDLT solve and the 6-vector → matrix step are
``icp_oracle``'s through ``robust_restatement._loop``; the robust weights and the per-row slot
packing are ``robust_restatement``'s; none of those modules is changed.

* ``intensity(colors)`` — ((r + g) + b) / 3.
* ``hybrid_lists`` — per point the ``max_nn`` nearest with strict d² < r², itself included, ordered
  by (d², index), d² = ``icp_oracle.sq_dist``: the contract of the device's hybrid search.
* ``color_gradients`` — InitializePointCloudForColoredICP: nn < 4 gives 0; entry 0 is skipped
  whatever it is (Open3D's loop starts at 1; among exact duplicates FLANN's order is unpinned, here
  the lowest index leads); rows A = (p − ((p − vt)·nt)·nt) − vt, b = ip − it, one more row
  (nn − 1)·nt, b = 0; (AᵀA)·x = Aᵀb by an unpivoted LDLᵀ.  Departure from Eigen, as the device: a
  pivot that is not positive and finite, or a non-finite solution, gives 0.  ``dtype`` selects
  float64 or ``np.longdouble``.
* ``colored_rows`` / ``colored_terms`` — the geometric and the photometric row of every matched
  pair, the 30 sums in the device's slot layout and Σ|term| per slot.
* ``registration_colored_icp`` — RegistrationICP with that update; ``on_eval(k, pcd, j)`` per
  evaluation; ``solve="lstsq"`` replaces the LDLT by a least-squares solve (the λ = 1 case of the
  slide fixture, whose JᵀJ is singular along the slide).
* fixtures: ``colored_pair`` (gicp_restatement.bumpy_pair plus a colour field with r ≠ g ≠ b),
  ``gradient_case`` and ``slide_pair`` (the ridge surface z = 0.02·sin 2x whose y offset only the
  colours see).
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np
from scipy.spatial import cKDTree

import gicp_restatement as G
import icp_oracle as I
import robust_restatement as R

LAMBDA = 0.968
MAX_NN = 30


def intensity(colors, dtype=np.float64):
    c = np.asarray(colors, dtype).reshape(-1, 3)
    return ((c[:, 0] + c[:, 1]) + c[:, 2]) / dtype(3.0)


def hybrid_lists(pts, radius, max_nn=MAX_NN):
    """→ list of int64 index arrays, one per point."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    if len(pts) == 0:
        return []
    tree = cKDTree(pts)
    r2 = radius * radius
    out = []
    for k, js in enumerate(tree.query_ball_point(pts, radius * (1 + 1e-9))):
        js = np.asarray(js, np.int64)
        d2 = I.sq_dist(pts[js], pts[k][None, :])
        m = d2 < r2
        js, d2 = js[m], d2[m]
        out.append(js[np.lexsort((js, d2))][:max_nn])
    return out


def _ldlt3(a, b, dtype):
    """Unpivoted LDLᵀ solve of the symmetric 3×3 a; None when a pivot is not positive and finite or
    the solution is not finite."""
    with np.errstate(all="ignore"):
        e0 = a[0, 0]
        l10, l20 = a[0, 1] / e0, a[0, 2] / e0
        e1 = a[1, 1] - l10 * a[0, 1]
        m = a[1, 2] - l20 * a[0, 1]
        l21 = m / e1
        e2 = (a[2, 2] - l20 * a[0, 2]) - l21 * m
        y0 = b[0]
        y1 = b[1] - l10 * y0
        y2 = (b[2] - l20 * y0) - l21 * y1
        x2 = y2 / e2
        x1 = y1 / e1 - l21 * x2
        x0 = (y0 / e0 - l10 * x1) - l20 * x2
    x = np.array([x0, x1, x2], dtype)
    ok = all(np.isfinite(e) and e > 0 for e in (e0, e1, e2)) and np.all(np.isfinite(x))
    return x if ok else None


def color_gradients(pts, normals, colors, radius, max_nn=MAX_NN, dtype=np.float64, lists=None):
    P = np.asarray(pts, dtype).reshape(-1, 3)
    N = np.asarray(normals, dtype).reshape(-1, 3)
    it = intensity(colors, dtype)
    lists = hybrid_lists(pts, radius, max_nn) if lists is None else lists
    g = np.zeros((len(P), 3), dtype)
    for k, idx in enumerate(lists):
        nn = len(idx)
        if nn < 4:
            continue
        adj = idx[1:]
        vt, nt = P[k], N[k]
        d = P[adj] - vt
        s = (d[:, 0] * nt[0] + d[:, 1] * nt[1]) + d[:, 2] * nt[2]
        A = np.vstack([(P[adj] - s[:, None] * nt) - vt, dtype(nn - 1) * nt])
        b = np.concatenate([it[adj] - it[k], np.zeros(1, dtype)])
        x = _ldlt3(A.T @ A, A.T @ b, dtype)
        if x is not None:
            g[k] = x
    return g


def colored_rows(src_t, src_i, tgt, tgt_n, tgt_i, tgt_g, corr, lam=LAMBDA):
    """→ (r (m, 2), J (m, 2, 6), d² (m,)) of the matched pairs: row 0 geometric, row 1 photometric."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    vs, vt, nt = src_t[corr[:, 0]], tgt[corr[:, 1]], tgt_n[corr[:, 1]]
    is_, it, dit = src_i[corr[:, 0]], tgt_i[corr[:, 1]], tgt_g[corr[:, 1]]
    sg, sp = np.sqrt(lam), np.sqrt(1.0 - lam)
    d = vs - vt
    s = (d[:, 0] * nt[:, 0] + d[:, 1] * nt[:, 1]) + d[:, 2] * nt[:, 2]
    r0 = sg * s
    J0 = sg * np.concatenate([np.cross(vs, nt), nt], axis=1)
    e = (vs - s[:, None] * nt) - vt
    is0 = ((dit[:, 0] * e[:, 0] + dit[:, 1] * e[:, 1]) + dit[:, 2] * e[:, 2]) + it
    M = np.eye(3)[None, :, :] - nt[:, :, None] * nt[:, None, :]
    ditM = -np.einsum("ma,mac->mc", dit, M)
    r1 = sp * (is_ - is0)
    J1 = sp * np.concatenate([np.cross(vs, ditM), ditM], axis=1)
    return np.stack([r0, r1], axis=1), np.stack([J0, J1], axis=1), I.sq_dist(vs, vt)


def colored_terms(src_t, src_i, tgt, tgt_n, tgt_i, tgt_g, corr, lam=LAMBDA, kind=R.L2, k=1.0):
    """→ (sums (30,), Σ|term| (30,)) in the device's slot layout, each row weighted on its own."""
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    if len(corr) == 0:
        return np.zeros(30), np.zeros(30)
    r, J, d2 = colored_rows(src_t, src_i, tgt, tgt_n, tgt_i, tgt_g, corr, lam)
    rr = r.reshape(-1)
    t = R._pack_rows(J.reshape(-1, 6), rr, R.weight(kind, rr, k), d2, len(corr))
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def registration_colored_icp(src, src_colors, tgt, tgt_n, tgt_colors, max_dist, init=None, lam=LAMBDA,
                             kind=R.L2, k=1.0, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30,
                             on_eval=None, tgt_gradient=None, solve="ldlt"):
    """registration_colored_icp.  Returns robust_restatement._loop's dict plus ``gradient``."""
    if max_dist <= 0:
        raise ValueError("Invalid max_correspondence_distance.")
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    tgt_n = np.asarray(tgt_n, np.float64).reshape(-1, 3)
    src_i, tgt_i = intensity(src_colors), intensity(tgt_colors)
    grad = (color_gradients(tgt, tgt_n, tgt_colors, 2.0 * max_dist, MAX_NN) if tgt_gradient is None
            else np.asarray(tgt_gradient, np.float64))

    def update(pcd, corr):
        sums, _ = colored_terms(pcd, src_i, tgt, tgt_n, tgt_i, grad, corr, lam, kind, k)
        A, b = G.sums_to_system(sums)
        if solve == "lstsq":
            return I.vec6_to_matrix(np.linalg.lstsq(A, -b, rcond=1e-12)[0])
        return R._solve((A, b))

    out = R._loop(src, tgt, max_dist, init, update, lambda upd: None, relative_fitness, relative_rmse,
                  max_iteration, on_eval)
    out["gradient"] = grad
    return out


# ------------------------------------------------------------------------------------ fixtures
def color_field(p, seed, noise=0.01):
    """A smooth colour field of position with r ≠ g ≠ b plus small noise, inside [0, 1]."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    c = np.stack([0.5 + 0.3 * np.sin(1.3 * x + 0.4 * y) * np.cos(0.7 * z),
                  0.45 + 0.25 * np.cos(0.9 * y - 0.5 * x),
                  0.55 + 0.2 * np.sin(1.1 * z + 0.8 * x + 0.3 * y)], axis=1)
    c = c + noise * np.random.default_rng(seed).standard_normal(c.shape)
    return np.ascontiguousarray(np.clip(c, 0.0, 1.0))


@lru_cache(maxsize=None)
def colored_pair(ns, nt, seed):
    """gicp_restatement.bumpy_pair with colours: the field is a function of the position in the
    target's frame, so the source is coloured where T_true puts it.  → dict(src, sn, sc, tgt, tn,
    tc, T_true), read-only."""
    from m3d import synth

    src, sn, tgt, tn, T = G.bumpy_pair(ns, nt, seed)
    sc = color_field(synth.apply(T, src), seed + 7)
    tc = color_field(tgt, seed + 8)
    out = dict(src=src, sn=sn, sc=sc, tgt=tgt, tn=tn, tc=tc, T_true=T)
    for a in out.values():
        a.setflags(write=False)
    return out


def slide_intensity(p):
    return (0.5 + 0.25 * np.sin(3 * p[:, 0]) * np.cos(2 * p[:, 1])) + 0.15 * np.sin(1.7 * p[:, 0] + 2.3 * p[:, 1])


def slide_surface(n, seed):
    """n points of the ridge surface z = 0.02·sin 2x over [−1, 1]², its unit normals, and colours
    with r ≠ g ≠ b whose mean is the smooth texture ``slide_intensity``."""
    xy = np.random.default_rng(seed).uniform(-1, 1, (n, 2))
    p = np.column_stack([xy, 0.02 * np.sin(2 * xy[:, 0])])
    nrm = np.column_stack([-0.04 * np.cos(2 * xy[:, 0]), np.zeros(n), np.ones(n)])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    i0 = slide_intensity(p)
    w = 0.1 * np.sin(2.0 * p[:, 0] + p[:, 1])
    return np.ascontiguousarray(p), np.ascontiguousarray(nrm), np.ascontiguousarray(np.stack([i0 + w, i0 - w, i0], axis=1))


SLIDE_RADIUS = 0.12
SLIDE_SHIFT = np.array([0.05, -0.03, 0.0])


@lru_cache(maxsize=None)
def slide_pair(n=2000):
    """The ridge-slide fixture: target and source are two samplings of the same coloured ridge
    surface, the source shifted by SLIDE_SHIFT, so the true transform is the translation
    −SLIDE_SHIFT.  The ridge runs along y: geometry does not see the y offset.  Read-only."""
    tgt, tn, tc = slide_surface(n, 1)
    s, sn, sc = slide_surface(n, 2)
    src = np.ascontiguousarray(s + SLIDE_SHIFT)
    out = dict(src=src, sn=sn, sc=sc, tgt=tgt, tn=tn, tc=tc)
    for a in out.values():
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def slide_run(lam=LAMBDA, solve="ldlt"):
    f = slide_pair()
    return registration_colored_icp(f["src"], f["sc"], f["tgt"], f["tn"], f["tc"], SLIDE_RADIUS, lam=lam, solve=solve)


GRADIENT_NS = (0, 1, 3, 257, 2000)


@lru_cache(maxsize=None)
def gradient_case(n, uniform=False):
    """n points: the ridge surface plus a few far stragglers (fewer than 4 neighbours each), and a
    radius at which a point away from the border has about 60 neighbours, so most lists hit the
    cap of 30.  → dict(pts, nrm, col, radius, lists, g64, gld), computed once, read-only."""
    stragglers = min(4, n // 64)
    m = n - stragglers
    pts, nrm, col = slide_surface(m, 11 + n)
    far = np.array([[5.0, 5.0, 0.0], [5.05, 5.0, 0.0], [9.0, -4.0, 1.0], [-7.0, 3.0, 2.0]])[:stragglers]
    pts = np.ascontiguousarray(np.vstack([pts, far]))
    nrm = np.ascontiguousarray(np.vstack([nrm, np.tile([0.0, 0.0, 1.0], (stragglers, 1))]))
    col = np.ascontiguousarray(np.vstack([col, color_field(far, 5)]))
    if uniform:
        col = np.full_like(col, 0.3)
    radius = float(np.sqrt(60.0 * 4.0 / (np.pi * max(m, 1))))
    lists = hybrid_lists(pts, radius)
    g64 = color_gradients(pts, nrm, col, radius, lists=lists)
    gld = color_gradients(pts, nrm, col, radius, dtype=np.longdouble, lists=lists)
    for a in (pts, nrm, col, g64, gld):
        a.setflags(write=False)
    return dict(pts=pts, nrm=nrm, col=col, radius=radius, lists=lists, g64=g64, gld=gld)


EVAL_NS = (1, 257, 1000, 8453)  # tests/test_gpu_gicp.py's shapes: 8453 = 34 block partials
EVAL_NT, EVAL_SEED = 777, 3


@lru_cache(maxsize=None)
def eval_case(ns, identity=False):
    """A one-evaluation case (gicp_restatement's geometry, radius G.RADIUS) with the restatement's
    gradients (radius 2·G.RADIUS, 30), the moved points, the exact correspondences and, for the
    robust kernels, the scale k = the median |r| over both rows of the matched pairs."""
    from m3d import synth

    f = colored_pair(ns, EVAL_NT, EVAL_SEED)
    src, sn, T = f["src"], f["sn"], f["T_true"]
    if identity:
        src, sn, T = np.ascontiguousarray(synth.apply(T, src)), sn @ T[:3, :3].T, np.eye(4)
    grad = color_gradients(f["tgt"], f["tn"], f["tc"], 2.0 * G.RADIUS)
    pcd = I.initial_points(T, src)
    _, _, corr, _ = I.registration_result(pcd, f["tgt"], G.RADIUS)
    j = np.full(ns, -1, np.int64)
    j[corr[:, 0]] = corr[:, 1]
    si, ti = intensity(f["sc"]), intensity(f["tc"])
    r = colored_rows(pcd, si, f["tgt"], f["tn"], ti, grad, corr)[0]
    out = dict(src=src, sn=sn, sc=f["sc"], tgt=f["tgt"], tn=f["tn"], tc=f["tc"], T=T, grad=grad, pcd=pcd, corr=corr,
               j=j, si=si, ti=ti)
    for a in out.values():
        a.setflags(write=False)
    out["k"] = float(np.median(np.abs(r))) if r.size else 1.0
    return out


LOOP_SEED = 31


@lru_cache(maxsize=None)
def loop_case(kind):
    """The 2,000 ↔ 2,000 loop fixture with init ``kind`` ("identity" / "perturbed",
    gicp_restatement.loop_init): the restatement's run with every evaluation recorded — computed
    once per session, never modified.  → dict(fixture…, init, ref, evals = [(pcd, j)])."""
    f = colored_pair(2000, 2000, LOOP_SEED)
    init = G.loop_init(kind)
    evals = []
    ref = registration_colored_icp(f["src"], f["sc"], f["tgt"], f["tn"], f["tc"], G.LOOP_RADIUS, init,
                                   on_eval=lambda k, pcd, j: evals.append((pcd.copy(), j.copy())))
    return dict(f, init=init, ref=ref, evals=evals)


def voxel_means(points, values, voxel):
    """Per-voxel plain means of ``values`` in ascending (ix, iy, iz) order, voxels as
    prep_oracle / Open3D place them: index = floor((p − (min − voxel/2)) / voxel)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = np.asarray(values, np.float64).reshape(len(p), -1)
    vmin = p.min(axis=0) - voxel * 0.5
    ijk = np.floor((p - vmin) / voxel).astype(np.int64)
    order = np.lexsort((ijk[:, 2], ijk[:, 1], ijk[:, 0]))
    ijk, v = ijk[order], v[order]
    first = np.flatnonzero(np.r_[True, np.any(np.diff(ijk, axis=0) != 0, axis=1)])
    return np.add.reduceat(v, first, axis=0) / np.diff(np.r_[first, len(p)])[:, None]
