"""ICP of a point cloud against a triangle mesh's surface (csrc/mesh_icp.hip) restated in numpy —
TEST INFRASTRUCTURE ONLY (tests/test_mesh_icp_cpu.py, tests/test_gpu_mesh_icp.py).

fp64, one operation at a time.  The winner of a point is ``mesh_restatement.closest_points``'; the
loop, the LDLT solve and the 6-vector → matrix step are ``icp_oracle``'s; the weights are
``robust_restatement.weight``.  None of those modules is changed, and nothing is copied from them.

One evaluation of the loop's points P:
* winner: the smallest (d², triangle index) over every usable triangle, q its closest point;
* match: d² < max_dist·max_dist, strictly (a NaN point never matches); unmatched: triangle −1, d² inf;
* row of a matched p with winner (a, b, c): (cx, cy, cz) the cross product of the usable test,
  len = sqrt((cx·cx + cy·cy) + cz·cz), n = (cx, cy, cz) / len, r = ((px−qx)·nx + (py−qy)·ny) + (pz−qz)·nz,
  J = [p × n | n], weight w(r); the 30 slots as ``robust_restatement._pack_rows`` lays them out;
* fitness = count / ns, rmse = sqrt(Σd² / count), both 0 without a match.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

import icp_oracle as I
import mesh_restatement as M
import robust_restatement as RB

L2, L1, HUBER, CAUCHY, GM, TUKEY = RB.L2, RB.L1, RB.HUBER, RB.CAUCHY, RB.GM, RB.TUKEY


def face_normals(vertices, triangles):
    """(F, 3) unit face normals in the device's operations (NaN rows for zero-area triangles)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    ab, ac = b - a, c - a
    cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    with np.errstate(all="ignore"):
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        return np.stack([cx / ln, cy / ln, cz / ln], axis=1)


def evaluate(pcd, vertices, triangles, max_dist):
    """One evaluation's matches → dict(triangle (n,) int32, −1 none; d2 (n,), inf none; point (n, 3);
    fitness; rmse)."""
    pcd = np.asarray(pcd, np.float64).reshape(-1, 3)
    n = len(pcd)
    if n == 0:
        return dict(triangle=np.zeros(0, np.int32), d2=np.zeros(0), point=np.zeros((0, 3)), fitness=0.0, rmse=0.0)
    cp = M.closest_points(vertices, triangles, pcd)
    hit = (cp["triangle"] >= 0) & (cp["d2"] < max_dist * max_dist)
    tri = np.where(hit, cp["triangle"], -1).astype(np.int32)
    d2 = np.where(hit, cp["d2"], np.inf)
    m = int(hit.sum())
    fit = m / n if m else 0.0
    rmse = float(np.sqrt(np.sum(d2[hit]) / m)) if m else 0.0
    return dict(triangle=tri, d2=d2, point=cp["point"], fitness=fit, rmse=rmse)


def rows(pcd, vertices, triangles, ev):
    """→ (r (m,), J (m, 6), d2 (m,), index (m,)) of the matched points, in increasing point index."""
    pcd = np.asarray(pcd, np.float64).reshape(-1, 3)
    idx = np.nonzero(ev["triangle"] >= 0)[0]
    p, q = pcd[idx], ev["point"][idx]
    nn = face_normals(vertices, triangles)[ev["triangle"][idx]]
    d = p - q
    r = (d[:, 0] * nn[:, 0] + d[:, 1] * nn[:, 1]) + d[:, 2] * nn[:, 2]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    nx, ny, nz = nn[:, 0], nn[:, 1], nn[:, 2]
    J = np.stack([y * nz - z * ny, z * nx - x * nz, x * ny - y * nx, nx, ny, nz], axis=1)
    return r, J, ev["d2"][idx], idx


def row_terms(pcd, vertices, triangles, ev, kind=L2, k=1.0):
    """(m, 30): every matched point's contribution to the 30 slots."""
    r, J, d2, idx = rows(pcd, vertices, triangles, ev)
    if len(idx) == 0:
        return np.zeros((0, 30))
    return RB._pack_rows(J, r, RB.weight(kind, r, k), d2, len(idx))


def sums(pcd, vertices, triangles, ev, kind=L2, k=1.0):
    """→ (sums (30,), Σ|term| (30,)) in the device's slot layout."""
    t = row_terms(pcd, vertices, triangles, ev, kind, k)
    return t.sum(axis=0), np.abs(t).sum(axis=0)


def system(pcd, vertices, triangles, ev, kind=L2, k=1.0):
    """JᵀJ (6×6), Jᵀr (6) with the rows weighted by w(r)."""
    r, J, _, _ = rows(pcd, vertices, triangles, ev)
    Jw = J * RB.weight(kind, r, k)[:, None]
    return Jw.T @ J, Jw.T @ r


def update(pcd, vertices, triangles, ev, kind=L2, k=1.0):
    """ΔT of one evaluation (identity without a match)."""
    if not (ev["triangle"] >= 0).any():
        return np.eye(4)
    JTJ, JTr = system(pcd, vertices, triangles, ev, kind, k)
    return I.vec6_to_matrix(I.ldlt_solve(JTJ, -JTr))


def pairs_of(tri):
    idx = np.nonzero(tri >= 0)[0]
    return np.stack([idx, tri[idx]], axis=1).astype(np.int64).reshape(-1, 2)


def registration_icp_to_mesh(src, vertices, triangles, max_dist, init=None, kind=L2, k=1.0, relative_fitness=1e-6,
                             relative_rmse=1e-6, max_iteration=30, on_eval=None):
    """RegistrationICP (icp_oracle.registration_icp's loop) against the mesh's surface.
    on_eval(k, pcd, triangle) at every evaluation."""
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError("Invalid max_correspondence_distance.")
    if not M.usable(vertices, triangles).any():
        raise ValueError("the mesh has no usable triangle")
    src = np.asarray(src, np.float64).reshape(-1, 3)
    T = np.eye(4) if init is None else np.asarray(init, np.float64).copy()
    pcd = I.initial_points(T, src)

    def ev_of(kk):
        ev = evaluate(pcd, vertices, triangles, max_dist)
        if on_eval is not None:
            on_eval(kk, pcd.copy(), ev["triangle"].copy())
        return ev

    ev = ev_of(0)
    it, converged = 0, False
    while it < max_iteration:
        upd = update(pcd, vertices, triangles, ev, kind, k)
        if not np.isfinite(upd).all():
            upd = np.eye(4)
        T = I.matmul4(upd, T)
        pcd = I.transform_points(upd, pcd)
        it += 1
        before = ev
        ev = ev_of(it)
        if abs(before["fitness"] - ev["fitness"]) < relative_fitness and abs(before["rmse"] - ev["rmse"]) < relative_rmse:
            converged = True
            break
    return dict(transformation=T, fitness=ev["fitness"], inlier_rmse=ev["rmse"],
                correspondence_set=pairs_of(ev["triangle"]), iterations=it, converged=converged, points=pcd)


# --------------------------------------------------------------------------------------- fixtures
def sample_surface(vertices, triangles, n, seed):
    """n area-weighted samples of the mesh's surface → (points (n, 3), triangle (n,))."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    rng = np.random.default_rng(seed)
    f = rng.choice(len(t), n, p=area / area.sum())
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return w[:, :1] * a[f] + w[:, 1:2] * b[f] + w[:, 2:] * c[f], f


def vertex_normals(vertices, triangles):
    """Area-weighted vertex normals (the sum of the incident faces' cross products, normalised)."""
    v = np.asarray(vertices, np.float64)
    t = np.asarray(triangles)
    cr = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])
    n = np.zeros_like(v)
    for k in range(3):
        np.add.at(n, t[:, k], cr)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def worst_error(T, T_true, pts):
    """max |T·p − T_true·p| over pts."""
    d = I.transform_points(T, pts) - I.transform_points(T_true, pts)
    return float(np.sqrt((d * d).sum(axis=1)).max())


NS, MESH_SEED, POSE_SEED = 600, 4, 5


@lru_cache(maxsize=None)
def clean_pair(n_lat=12, n_lon=16):
    """The pair of the feature's motivating table: ``synth.surface_mesh(n_lat, n_lon, seed=4)``, 600
    area-weighted surface samples moved by the inverse of a small rigid motion; radius 0.1·extent."""
    from m3d import synth

    v, f = synth.surface_mesh(n_lat, n_lon, seed=MESH_SEED)
    ext = float((v.max(axis=0) - v.min(axis=0)).max())
    on, _ = sample_surface(v, f, NS, seed=1)
    T_true = synth.random_rigid(POSE_SEED, v.mean(axis=0), rot_range=0.08, trans_range=0.02 * ext)
    src = I.transform_points(np.linalg.inv(T_true), on)
    for a in (v, f, on, src, T_true):
        a.setflags(write=False)
    return dict(v=v, f=f, ext=ext, on=on, src=src, T_true=T_true, radius=0.1 * ext)


@lru_cache(maxsize=None)
def outlier_pair():
    """The same mesh and pose: noise of 0.001·extent on every sample, 15 % of them pushed 0.03·extent
    off the surface in a random direction; radius 0.02·extent, Tukey / Huber scale 0.005·extent."""
    c = clean_pair()
    v, f, ext = c["v"], c["f"], c["ext"]
    on = c["on"]
    rng = np.random.default_rng(18)
    out = np.zeros(NS, bool)
    out[rng.permutation(NS)[: round(0.15 * NS)]] = True
    d = rng.standard_normal((NS, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    pts = on + rng.normal(0.0, 0.001 * ext, (NS, 3)) + (out * 0.03 * ext)[:, None] * d
    src = I.transform_points(np.linalg.inv(c["T_true"]), pts)
    for a in (src, out):
        a.setflags(write=False)
    return dict(v=v, f=f, ext=ext, on=on, src=src, T_true=c["T_true"], outlier=out, radius=0.02 * ext, k=0.005 * ext)


def loop_init(init_kind):
    """"identity", or a small non-identity start (a twentieth of the pair's motion's scale)."""
    if init_kind == "identity":
        return np.eye(4)
    from m3d import synth

    c = clean_pair()
    return synth.random_rigid(23, c["v"].mean(axis=0), rot_range=0.01, trans_range=0.002 * c["ext"])


def trajectory(src, init, updates):
    """The loop's points at every evaluation of a run whose updates are given: P₀ = the source, moved
    by init unless isIdentity(); P_{k+1} = updates[k] applied to P_k in q64_of's operation order —
    the points of a loop that applied exactly those updates, bit for bit."""
    pts = [I.initial_points(np.eye(4) if init is None else np.asarray(init, np.float64), src)]
    for upd in updates:
        pts.append(I.transform_points(upd, pts[-1]))
    return pts


def stop_rule(history, relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):
    """RegistrationICP's stop decision on the (fitness, rmse) of evaluations 0, 1, … → (iterations,
    converged), or None when the history ends before the loop would."""
    for k in range(1, len(history)):
        if abs(history[k - 1][0] - history[k][0]) < relative_fitness and abs(history[k - 1][1] - history[k][1]) < relative_rmse:
            return k, True
        if k >= max_iteration:
            return k, False
    return (0, False) if max_iteration == 0 else None
