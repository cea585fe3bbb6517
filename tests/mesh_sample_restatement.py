"""The contracts of csrc/mesh_sample.hip (uniform surface sampling) and csrc/thin.hip
(minimum-distance thinning) restated in numpy, bit for bit: integer arithmetic in uint64, every
floating-point operation a single fp64 numpy operation in the order the headers state.  scipy's
cKDTree only proposes the candidate pairs of the thinning; membership is the exact d² test.
"""
import numpy as np
from scipy.spatial import cKDTree

U64 = np.uint64
_M32 = U64(0xFFFFFFFF)


# --------------------------------------------------------------------------------- sampler.h
def splitmix64(x):
    with np.errstate(over="ignore"):
        z = np.asarray(x, U64) + U64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
        return z ^ (z >> U64(31))


def sample_base(seed: int, k):
    with np.errstate(over="ignore"):
        return splitmix64(U64(seed & 0xFFFFFFFFFFFFFFFF) ^ (np.asarray(k, U64) * U64(0x9E3779B97F4A7C15)))


def umul64hi(x, w: int):
    """The high 64 bits of x·w (x uint64 array, w an int below 2^64), in 32-bit pieces."""
    x = np.asarray(x, U64)
    a, b = x >> U64(32), x & _M32
    c, d = U64(w >> 32), U64(w & 0xFFFFFFFF)
    ad, bc, bd = a * d, b * c, b * d
    carry = ((ad & _M32) + (bc & _M32) + (bd >> U64(32))) >> U64(32)
    return a * c + (ad >> U64(32)) + (bc >> U64(32)) + carry


# --------------------------------------------------------------------------------- weights
def _cross(v, f):
    a, b, c = (v[f[:, k]] for k in range(3))
    ab, ac = b - a, c - a
    cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
    cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
    cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    return a, ab, ac, cx, cy, cz


def lengths(v, f):
    """len_f of the contract: 0 for an unusable triangle or a length that is not finite."""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a, ab, ac, cx, cy, cz = _cross(v, f)
        fin = np.isfinite(v[f].reshape(len(f), 9)).all(axis=1)
        usable = fin & ~((cx == 0.0) & (cy == 0.0) & (cz == 0.0))
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
    return np.where(usable & np.isfinite(ln), ln, 0.0), usable


def weights(v, f):
    """→ (w uint64 (F,), cum uint64 (F,), W int).  ValueError without a usable triangle, or without
    one of finite non-zero length."""
    ln, usable = lengths(v, f)
    if not usable.any():
        raise ValueError("the mesh has no usable triangle")
    L = float(ln.max())
    if not L > 0.0:
        raise ValueError("the mesh has no triangle with a finite non-zero area")
    _, e = np.frexp(L)
    w = np.trunc(np.ldexp(ln, 32 - int(e))).astype(U64)
    cum = np.cumsum(w, dtype=U64)
    return w, cum, int(cum[-1])


def triangle_of_x0(cum, x0):
    """The triangle of a draw whose first stream value is x0: the smallest f with cum_f > t,
    t = the high 64 bits of x0·W."""
    t = umul64hi(x0, int(cum[-1]))
    return np.searchsorted(cum, t, side="right").astype(np.int32)


def triangle_of_t(cum, t):
    return np.searchsorted(cum, np.asarray(t, U64), side="right").astype(np.int32)


def fold(u, v):
    s = u + v
    over = s > 1.0
    return np.where(over, 1.0 - u, u), np.where(over, 1.0 - v, v)


def sample(v, f, n: int, seed: int = 0) -> dict:
    """m3d_mesh_sample: → point (n, 3), triangle (n,) int32, uv (n, 2), normal (n, 3)."""
    v = np.asarray(v, np.float64)
    f = np.asarray(f, np.int64).reshape(-1, 3)
    _, cum, _ = weights(v, f)
    base = sample_base(seed, np.arange(n, dtype=U64))
    with np.errstate(over="ignore"):
        x0, x1, x2 = splitmix64(base), splitmix64(base + U64(1)), splitmix64(base + U64(2))
    tri = triangle_of_x0(cum, x0)
    u = (x1 >> U64(11)).astype(np.float64) * 2.0 ** -53
    w = (x2 >> U64(11)).astype(np.float64) * 2.0 ** -53
    u, w = fold(u, w)
    with np.errstate(all="ignore"):
        a, ab, ac, cx, cy, cz = _cross(v, f[tri])
        point = (a + ab * u[:, None]) + ac * w[:, None]
        ln = np.sqrt((cx * cx + cy * cy) + cz * cz)
        normal = np.stack([cx / ln, cy / ln, cz / ln], axis=1)
    return {"point": point.reshape(n, 3), "triangle": tri, "uv": np.stack([u, w], axis=1).reshape(n, 2),
            "normal": normal.reshape(n, 3)}


# --------------------------------------------------------------------------------- thinning
def keys(seed: int, n: int):
    return sample_base(seed, np.arange(n, dtype=U64))


def rank_order(seed: int, n: int):
    """The point indices in ascending (key, index) order."""
    return np.lexsort((np.arange(n), keys(seed, n)))


def _pairs(points, radius):
    """Every pair i < j with d²(i, j) < radius², d² the contract's expression.  A point with a
    coordinate that is not finite is in no pair."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    fin = np.isfinite(p).all(axis=1)
    idx = np.flatnonzero(fin)
    if len(idx) < 2:
        return np.zeros((0, 2), np.int64)
    span = float(np.abs(p[idx]).max())
    cand = cKDTree(p[idx]).query_pairs(radius * (1.0 + 1e-9) + span * 1e-12, output_type="ndarray")
    i, j = idx[cand[:, 0]], idx[cand[:, 1]]
    d = p[j] - p[i]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    keep = d2 < radius * radius
    return np.stack([i[keep], j[keep]], axis=1)


def _ranked_pairs(points, radius, seed):
    """→ (lo, hi): for every pair inside the radius the lower- and the higher-ranked index."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    pr = _pairs(p, radius)
    k = keys(seed, len(p))
    i, j = pr[:, 0], pr[:, 1]  # i < j
    i_lower = (k[i] < k[j]) | ((k[i] == k[j]) & (i < j))
    return np.where(i_lower, i, j), np.where(i_lower, j, i)


def _check_radius(radius):
    if not (np.isfinite(radius) and radius > 0.0):
        raise ValueError("thin_min_distance: radius must be finite and > 0")


def thin_greedy(points, radius: float, seed: int = 0):
    """The definition: through the points by rank, a point is kept unless a kept point lies strictly
    inside its radius → kept mask (n,) bool."""
    _check_radius(radius)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    lo, hi = _ranked_pairs(p, radius, seed)
    order = np.argsort(hi, kind="stable")
    lo, hi = lo[order], hi[order]
    start = np.searchsorted(hi, np.arange(n + 1))
    kept = np.zeros(n, bool)
    fin = np.isfinite(p).all(axis=1)
    for i in rank_order(seed, n):
        kept[i] = fin[i] and not kept[lo[start[i]:start[i + 1]]].any()
    return kept


def thin_rounds(points, radius: float, seed: int = 0):
    """The device form's synchronous rounds → (decided (n,) int32: +k kept / −k dropped in round k,
    rounds).  Round R decides from the state after round R − 1 alone."""
    _check_radius(radius)
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(p)
    lo, hi = _ranked_pairs(p, radius, seed)
    fin = np.isfinite(p).all(axis=1)
    decided = np.zeros(n, np.int32)
    R = 0
    while (decided == 0).any():
        R += 1
        if R > 256:
            raise RuntimeError("thin_rounds: round bound reached")
        und = decided == 0
        kept_lower = np.bincount(hi, weights=(decided[lo] > 0), minlength=n) > 0
        und_lower = np.bincount(hi, weights=und[lo], minlength=n) > 0
        new = decided.copy()
        new[und & ~fin] = -R
        new[und & fin & kept_lower] = -R
        new[und & fin & ~kept_lower & ~und_lower] = R
        decided = new
    return decided, R


def thin_min_distance(points, radius: float, seed: int = 0):
    """prep.thin_min_distance: the kept indices, ascending int64."""
    return np.flatnonzero(thin_rounds(points, radius, seed)[0] > 0).astype(np.int64)
