"""CPU restatement of the outlier-removal path (numpy only) and the seeded inputs its tests share.

* lists: brute force, d² = (dx·dx + dy·dy) + dz·dz in fp64, each row ordered by
  ``np.lexsort((index, d2))`` — KDTreeFlann::SearchKNN with ties broken by the lower index;
* ``avg``: Σ ``np.sqrt(d²)`` over the list, accumulated sequentially from 0.0 in list order, / count;
* statistics: Open3D 0.19 RemoveStatisticalOutliers, sums accumulated sequentially in index order
  with its ``> 0`` rules; kept iff ``avg > 0 and avg < threshold``;
* radius counts: #{j : d² < r·r}, the point itself included; kept iff count > nb_points.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

CENTRE = np.array([10.0, -4.0, 2.5])


def shell(seed, n, strays, far=0, dup=0, box=0.6):
    """A noisy unit sphere shell around CENTRE, `strays` uniform points in the box ±(1 + box)
    around it, optionally two far points and the first `dup` rows again; all permuted."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    rad = 1.0 + 0.002 * rng.standard_normal(n)
    parts = [CENTRE + u * rad[:, None]]
    parts.append(CENTRE + rng.uniform(-(1.0 + box), 1.0 + box, size=(strays, 3)))
    if far:
        parts.append(np.array([[1e3, 1e3, 1e3], [-2e3, 5.0, 7.0]]))
    P = np.concatenate(parts)
    if dup:
        P = np.concatenate([P, P[:dup]])
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def lattice():
    """8×8×8 lattice, spacing 0.25, offset (3, −1, 0.5): every coordinate exact in fp64 and fp32."""
    g = np.arange(8) * 0.25
    P = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) + np.array([3.0, -1.0, 0.5])
    return np.ascontiguousarray(P[np.random.default_rng(8).permutation(len(P))])


def line():
    """500 points on a line: a grid one cell thick."""
    P = np.empty((500, 3))
    P[:, 0] = 5.0 + 0.01 * np.arange(500)
    P[:, 1] = 1.0
    P[:, 2] = -2.0
    return P


# name → (points factory, nb_neighbors, std_ratio, removed by the restatement)
CASES = {
    "A": (lambda: shell(1, 3000, 60), 20, 2.0, 43),
    "B": (lambda: shell(2, 3000, 60), 20, 1.0, 53),
    "C": (lambda: shell(3, 1500, 30, dup=40), 8, 2.0, 23),
    "D": (lambda: shell(4, 700, 10), 50, 2.0, 7),
    "E": (lambda: shell(5, 2000, 40, far=1), 20, 2.0, 2),
    "F": (lambda: shell(6, 12, 0), 20, 2.0, 1),
    "G": (lambda: shell(7, 300, 0, dup=300), 2, 2.0, 600),
    "L7_1": (lattice, 7, 1.0, 512 - 432),
    "L7_2": (lattice, 7, 2.0, 512 - 504),
    "L10_1": (lattice, 10, 1.0, 512 - 432),
    "M": (line, 6, 1.0, 500 - 496),
}


@lru_cache(maxsize=None)
def points(name):
    P = CASES[name][0]()
    P.setflags(write=False)
    return P


def d2_rows(P, rows):
    d = P[None, :, :] - P[rows, None, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn(P, k):
    """→ (idx n×k int32, −1 pad; d2 n×k, inf pad; count n int32)."""
    n = len(P)
    kk = min(k, n)
    idx = np.full((n, k), -1, np.int32)
    d2 = np.full((n, k), np.inf)
    ar = np.arange(n)
    for i0 in range(0, n, 512):
        D = d2_rows(P, np.arange(i0, min(i0 + 512, n)))
        for r in range(D.shape[0]):
            o = np.lexsort((ar, D[r]))[:kk]
            idx[i0 + r, :kk] = o
            d2[i0 + r, :kk] = D[r, o]
    return idx, d2, np.full(n, kk, np.int32)


def mean_distance(d2, count):
    """Σ sqrt(d²) in list order from 0.0, / count (rows of one cloud share their count)."""
    n = len(d2)
    acc = np.zeros(n)
    kk = int(count[0]) if n else 0
    for s in range(kk):
        acc = acc + np.sqrt(d2[:, s])
    return acc / float(kk) if n else acc


def statistics(avg, std_ratio):
    """RemoveStatisticalOutliers from the mean distances → namespace(valid, mean, std_dev,
    threshold, keep mask, indices, margin = the smallest |avg − threshold| / threshold over the
    points with avg > 0)."""
    n = len(avg)
    valid = n
    if n == 0:
        return SimpleNamespace(valid=0, mean=0.0, std_dev=0.0, threshold=0.0, keep=np.zeros(0, bool),
                               indices=np.zeros(0, np.int32), margin=np.inf)
    s = 0.0
    for a in avg:
        if a > 0:
            s += float(a)
    mean = s / valid
    q = 0.0
    for a in avg:
        if a > 0:
            q += (float(a) - mean) * (float(a) - mean)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.sqrt(np.float64(q) / np.float64(valid - 1)))
    thr = mean + std_ratio * std
    keep = (avg > 0) & (avg < thr)
    pos = avg[avg > 0]
    margin = float(np.min(np.abs(pos - thr) / thr)) if len(pos) and thr > 0 else np.inf
    return SimpleNamespace(valid=valid, mean=mean, std_dev=std, threshold=thr, keep=keep,
                           indices=np.flatnonzero(keep).astype(np.int32), margin=margin)


@lru_cache(maxsize=None)
def knn_case(name, k):
    """The lists of a named cloud (computed once per session, never modified)."""
    out = knn(points(name), k)
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def stat_case(name):
    """→ (avg, statistics) of a CASES entry with its own parameters."""
    _, k, ratio, _ = CASES[name]
    cloud = name if not name.startswith("L") else "L7_1"  # one lattice, three parameter sets
    _, d2, cnt = knn_case(cloud, k)
    avg = mean_distance(d2, cnt)
    avg.setflags(write=False)
    return avg, statistics(avg, ratio)


def radius_counts(P, radius):
    r2 = radius * radius
    out = np.empty(len(P), np.int32)
    for i0 in range(0, len(P), 512):
        out[i0:i0 + 512] = (d2_rows(P, np.arange(i0, min(i0 + 512, len(P)))) < r2).sum(1)
    return out
