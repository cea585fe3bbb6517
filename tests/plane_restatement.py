"""CPU restatement of the plane-segmentation contract (include/m3d.h "plane segmentation", Open3D
0.19 PointCloud::SegmentPlane), line by line in numpy: the counter sampler, both plane fits, the
sequential best / break loop, the inliers and the refit.  Products and sums are written so that
numpy rounds each operation on its own (no fused multiply-add, ``np.cumsum(...)[-1]`` for a
sequential sum); one hypothesis is vectorised over the points.

Besides the result a run reports what a comparison with another implementation depends on:
  ``rmse_gaps``    for every decision taken on rmse at equal counts, |rmse − best_rmse| / max
  ``break_args``   for every break_it update, (the min(...) argument, its distance from the nearest
                   integer, whether it is exact: the num_iterations clamp, or the f = 1 branch,
                   which takes no logarithm)
  ``plane_pairwise`` / ``refit_diff``  the refit under numpy's pairwise summation, and its largest
                   difference from the sequential one (normal, d)
"""
from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

M64 = (1 << 64) - 1


def splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def native_sample(seed: int, h: int, n: int, m: int) -> list[int]:
    """ransac.hip native_triple for m distinct indices of [0, n)."""
    base = splitmix64((seed ^ ((h * 0x9E3779B97F4A7C15) & M64)) & M64)
    out: list[int] = []
    k = 0
    while len(out) < m and k < (1 << 20):
        v = splitmix64((base + k) & M64)
        idx = ((v >> 32) * n) >> 32
        if idx not in out:
            out.append(idx)
        k += 1
    return out


ZERO = np.zeros(4)


def plane_from_triangle(p0, p1, p2) -> np.ndarray:
    p0, p1, p2 = (np.asarray(p, np.float64) for p in (p0, p1, p2))
    e0, e1 = p1 - p0, p2 - p0
    a = e0[1] * e1[2] - e0[2] * e1[1]
    b = e0[2] * e1[0] - e0[0] * e1[2]
    c = e0[0] * e1[1] - e0[1] * e1[0]
    norm = np.sqrt((a * a + b * b) + c * c)
    if norm == 0.0:
        return ZERO.copy()
    a, b, c = a / norm, b / norm, c / norm
    return np.array([a, b, c, -((a * p0[0] + b * p0[1]) + c * p0[2])])


def _colsum(A, order):
    """Column sums of an m×k array: 'seq' in row order, 'pairwise' numpy's own ``sum``."""
    if order == "seq":
        return np.cumsum(A, axis=0)[-1]
    return np.array([np.sum(np.ascontiguousarray(A[:, k])) for k in range(A.shape[1])])


def plane_from_points(P, order: str = "seq") -> np.ndarray:
    """Open3D GetPlaneFromPoints."""
    P = np.asarray(P, np.float64).reshape(-1, 3)
    m = len(P)
    if m < 3:
        return ZERO.copy()
    cen = _colsum(P, order) / np.float64(m)
    r = P - cen
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    xx, xy, xz, yy, yz, zz = _colsum(np.stack([x * x, x * y, x * z, y * y, y * z, z * z], axis=1), order)
    det_x = yy * zz - yz * yz
    det_y = xx * zz - xz * xz
    det_z = xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        a, b, c = det_x, xz * yz - xy * zz, xy * yz - xz * yy
    elif det_y > det_z:
        a, b, c = xz * yz - xy * zz, det_y, xy * xz - yz * xx
    else:
        a, b, c = xy * yz - xz * yy, xy * xz - yz * xx, det_z
    norm = np.sqrt((a * a + b * b) + c * c)
    if norm == 0.0:
        return ZERO.copy()
    a, b, c = a / norm, b / norm, c / norm
    return np.array([a, b, c, -((a * cen[0] + b * cen[1]) + c * cen[2])])


def plane_of_sample(P, idx) -> np.ndarray:
    idx = list(idx)
    if len(idx) == 3:
        return plane_from_triangle(P[idx[0]], P[idx[1]], P[idx[2]])
    return plane_from_points(P[idx], "seq")


def dist(plane, P) -> np.ndarray:
    a, b, c, d = (np.float64(v) for v in plane)
    return np.abs(((a * P[:, 0] + b * P[:, 1]) + c * P[:, 2]) + d)


def score(plane, P, thr):
    """(count, err): err the sequential sum of dist² over the inliers in index order."""
    dd = dist(plane, P)
    sel = dd[dd < thr]
    if len(sel) == 0:
        return 0, np.float64(0.0)
    return len(sel), np.cumsum(sel * sel)[-1]


def break_argument(count, n, ransac_n, probability, num_iterations):
    """(break_it, the min(...) argument, its distance from the nearest integer, exact: the clamp
    or the f = 1 branch)."""
    f = np.float64(count) / np.float64(n)
    if not f < 1.0:
        return 0.0, 0.0, 0.0, True
    with np.errstate(all="ignore"):
        x = np.log(np.float64(1.0) - np.float64(probability)) / np.log(np.float64(1.0) - np.float64(f) ** ransac_n)
    arg = min(x, np.float64(num_iterations))
    clamped = not (x < num_iterations)
    off = 0.0 if not np.isfinite(arg) else abs(arg - np.round(arg))
    return float(np.trunc(arg)), float(arg), float(off), clamped


@dataclass
class Run:
    plane: np.ndarray
    plane_pairwise: np.ndarray
    ransac_plane: np.ndarray
    inliers: np.ndarray
    best_index: int
    best_count: int
    best_rmse: float
    evaluated: int
    iterations: int
    break_it: float
    counts: np.ndarray
    err: np.ndarray
    records: int = 0
    rmse_gaps: list = field(default_factory=list)
    break_args: list = field(default_factory=list)
    refit_diff: tuple = (0.0, 0.0)


def segment_plane(P, distance_threshold=0.01, ransac_n=3, num_iterations=100, probability=0.99999999,
                  seed=0, samples=None) -> Run:
    P = np.ascontiguousarray(P, np.float64).reshape(-1, 3)
    n = len(P)
    thr = np.float64(distance_threshold)
    best_count, best_rmse, best_plane, best_index = 0, np.float64(0.0), ZERO.copy(), -1
    break_it, evaluated = np.inf, 0
    counts = np.full(num_iterations, -1, np.int32)
    err = np.full(num_iterations, -1.0)
    records, gaps, bargs = 0, [], []
    iterations = num_iterations
    for h in range(num_iterations):
        if evaluated > break_it:
            iterations = h
            break
        idx = native_sample(seed, h, n, ransac_n) if samples is None else [int(v) for v in samples[h]]
        pi = plane_of_sample(P, idx)
        if not pi.any():
            continue
        count, e = score(pi, P, thr)
        rmse = e / np.sqrt(np.float64(count)) if count else np.float64(0.0)
        counts[h], err[h] = count, e
        if count == best_count and count > 0:  # (count 0: both rmse are the literal 0, no sum behind them)
            big = max(abs(rmse), abs(best_rmse))
            gaps.append(abs(rmse - best_rmse) / big if big > 0 else 0.0)
        if count > best_count or (count == best_count and rmse < best_rmse):
            best_count, best_rmse, best_plane, best_index = count, rmse, pi, h
            records += 1
            break_it, arg, off, clamped = break_argument(count, n, ransac_n, probability, num_iterations)
            bargs.append((arg, off, clamped))
        evaluated += 1
    inliers = np.nonzero(dist(best_plane, P) < thr)[0].astype(np.int64) if best_index >= 0 else np.zeros(0, np.int64)
    plane = plane_from_points(P[inliers], "seq")
    plane_pw = plane_from_points(P[inliers], "pairwise")
    diff = (float(np.abs(plane[:3] - plane_pw[:3]).max()), float(abs(plane[3] - plane_pw[3])))
    return Run(plane, plane_pw, best_plane, inliers, best_index, best_count, float(best_rmse), evaluated,
               iterations, break_it, counts, err, records, gaps, bargs, diff)


def scene(n: int, seed: int, offset: float = 0.0) -> np.ndarray:
    """A scan of a part on a table: 55 % on a 4 × 4 patch with N(0, 0.004) out-of-plane noise, 35 %
    in a 1.0 × 0.6 × 0.4 box above it, 10 % uniform strays in ±3; rotated by a random orthogonal
    matrix, shifted by ``offset`` on every axis, shuffled."""
    rng = np.random.default_rng(seed)
    n_pl = int(0.55 * n)
    n_ob = int(0.35 * n)
    n_st = n - n_pl - n_ob
    pl = np.column_stack([rng.uniform(-2, 2, n_pl), rng.uniform(-2, 2, n_pl), rng.normal(0.0, 0.004, n_pl)])
    ob = np.column_stack([rng.uniform(-0.5, 0.5, n_ob), rng.uniform(-0.3, 0.3, n_ob), rng.uniform(0.02, 0.42, n_ob)])
    st = rng.uniform(-3, 3, (n_st, 3))
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    P = np.vstack([pl, ob, st]) @ Q.T + np.float64(offset)
    P = P[rng.permutation(n)]
    P.setflags(write=False)
    return P


# the segment_plane configurations of the GPU test: name -> (n, scene seed, offset, ransac_n,
# iterations, sampler seed); thr 0.012, probability 0.99999999
THR = 0.012
PROB = 0.99999999
CONFIGS = {
    "n3": (20000, 11, 0.0, 3, 300, 7),
    "n3_off": (20000, 11, 1e3, 3, 300, 7),
    "n4": (4097, 12, 0.0, 4, 200, 7),
    "n6": (20000, 13, 0.0, 6, 200, 7),
}


@lru_cache(maxsize=None)
def config_points(name: str) -> np.ndarray:
    n, sseed, off, *_ = CONFIGS[name]
    return scene(n, sseed, off)


@lru_cache(maxsize=None)
def config_run(name: str) -> Run:
    """Computed once per session and shared; treat as read-only."""
    n, sseed, off, rn, iters, seed = CONFIGS[name]
    return segment_plane(config_points(name), THR, rn, iters, PROB, seed=seed)
