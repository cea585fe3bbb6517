"""CPU restatement of DBSCAN as Open3D 0.19 ``PointCloud::ClusterDBSCAN`` computes it, and the
seeded inputs its tests share (numpy; scipy's cKDTree only proposes candidates).

* ``neighbours``: nbs[i] = {j : d² < eps·eps}, strict, the point itself included,
  d² = (dx·dx + dy·dy) + dz·dz in fp64 — the project's order; each list ascending;
* ``literal``: a port of Open3D's loop, the pop order of its ``unordered_set`` selectable (first in
  first out, or drawn from an rng);
* ``closed_form``: what the loop computes whatever the order — a core point takes the rank of its
  component in the core graph (components ranked by their smallest member), a non-core point the
  smallest label among its core neighbours, every other point −1.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
from scipy.sparse import csr_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

import clean_restatement as C


def d2_pairs(P, i, j):
    d = P[j] - P[i]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbours(P, eps):
    """→ list of n ascending int64 arrays.  The tree search runs at a radius a little beyond eps
    (its own arithmetic is not the project's); the exact test decides."""
    P = np.asarray(P, np.float64)
    n = len(P)
    if n == 0:
        return []
    slack = eps * 1e-6 + 1e-9 * (float(np.abs(P).max()) + 1.0)
    cand = cKDTree(P).query_ball_point(P, eps + slack, return_sorted=True)
    r2 = eps * eps
    out = []
    for i in range(n):
        c = np.asarray(cand[i], np.int64)
        out.append(c[d2_pairs(P, i, c) < r2])
    return out


def tie_margin(P, eps):
    """The smallest |d² − eps²| / eps² over all pairs near the radius (inf without any)."""
    P = np.asarray(P, np.float64)
    pairs = cKDTree(P).query_pairs(eps * 1.5, output_type="ndarray")
    if len(pairs) == 0:
        return np.inf
    r2 = eps * eps
    return float(np.min(np.abs(d2_pairs(P, pairs[:, 0], pairs[:, 1]) - r2) / r2))


def literal(nbs, min_points, rng=None):
    """Open3D's loop.  rng None: the pending set pops first in first out; otherwise a random member."""
    n = len(nbs)
    labels = np.full(n, -2, np.int32)
    cluster = 0
    for idx in range(n):
        if labels[idx] != -2:
            continue
        if len(nbs[idx]) < min_points:
            labels[idx] = -1
            continue
        pending = [int(j) for j in nbs[idx] if j != idx]
        visited = set(int(j) for j in nbs[idx])
        visited.add(idx)
        labels[idx] = cluster
        head = 0
        while head < len(pending):
            if rng is not None:
                k = int(rng.integers(head, len(pending)))
                pending[head], pending[k] = pending[k], pending[head]
            nb = pending[head]
            head += 1
            if labels[nb] == -1:
                labels[nb] = cluster
            if labels[nb] != -2:
                continue
            labels[nb] = cluster
            if len(nbs[nb]) >= min_points:
                for q in nbs[nb]:
                    q = int(q)
                    if q not in visited:
                        visited.add(q)
                        pending.append(q)
        cluster += 1
    return labels


def closed_form(nbs, min_points):
    """→ namespace(labels int32, core mask, border mask, multi = border points whose core neighbours
    carry more than one label, num_clusters)."""
    n = len(nbs)
    core = np.array([len(b) >= min_points for b in nbs], bool) if n else np.zeros(0, bool)
    labels = np.full(n, -1, np.int32)
    border = np.zeros(n, bool)
    multi = np.zeros(n, bool)
    if not core.any():
        return SimpleNamespace(labels=labels, core=core, border=border, multi=multi, num_clusters=0)
    rows = np.concatenate([np.full(len(nbs[i]), i, np.int64) for i in range(n) if core[i]])
    cols = np.concatenate([nbs[i] for i in range(n) if core[i]])
    keep = core[cols]
    g = csr_matrix((np.ones(keep.sum(), np.int8), (rows[keep], cols[keep])), shape=(n, n))
    _, comp = connected_components(g, directed=False)
    ci = np.flatnonzero(core)
    first = {}
    for i in ci:  # ascending: a component's first appearance is its smallest member
        first.setdefault(int(comp[i]), len(first))
    labels[ci] = [first[int(comp[i])] for i in ci]
    for i in np.flatnonzero(~core):
        cn = nbs[i][core[nbs[i]]]
        if len(cn):
            ls = labels[cn]
            labels[i] = ls.min()
            border[i] = True
            multi[i] = ls.min() != ls.max()
    return SimpleNamespace(labels=labels, core=core, border=border, multi=multi, num_clusters=len(first))


# name → (clean_restatement cloud, eps, min_points, clusters, noise, border, border points touching
# more than one cluster)
CASES = {
    "A_008_6": ("A", 0.08, 6, 96, 592, 899, 77),
    "A_012_10": ("A", 0.12, 10, 7, 133, 700, 34),
    "C_01_5": ("C", 0.1, 5, 93, 319, 430, 41),
    "E_01_8": ("E", 0.1, 8, 77, 996, 616, 32),      # two far strays
    "G_005_3": ("G", 0.05, 3, 28, 480, 0, 0),       # every point doubled
    "L_026_7": ("L7_1", 0.26, 7, 1, 80, 216, 0),
    "L_025_1": ("L7_1", 0.25, 1, 512, 0, 0, 0),     # every pair at exactly eps or beyond
    "M_00101_3": ("M", 0.0101, 3, 1, 0, 2, 0),      # a line
}
TIE_CASE = "L_025_1"


def solve(P, eps, min_points):
    """→ namespace(points, eps, min_points, nbs, counts, + closed_form's fields); arrays read-only."""
    nbs = neighbours(P, eps)
    r = closed_form(nbs, min_points)
    r.points, r.eps, r.min_points, r.nbs = P, eps, min_points, nbs
    r.counts = np.array([len(b) for b in nbs], np.int32)
    r.sizes = np.bincount(r.labels[r.labels >= 0], minlength=r.num_clusters).astype(np.int32)
    for a in (r.labels, r.core, r.border, r.multi, r.counts, r.sizes):
        a.setflags(write=False)
    return r


@lru_cache(maxsize=None)
def case(name):
    """A CASES row solved once per session."""
    cloud, eps, mp = CASES[name][:3]
    return solve(C.points(cloud), eps, mp)


def chain():
    """4120 points along a boustrophedon: 40 rows of 100 steps of 0.9·eps, 3 connecting steps
    between rows, z = 0.3·sin(0.05·k), eps = 0.05, offset (100, −50, 7), indices permuted."""
    eps = 0.05
    s = 0.9 * eps
    pts = []
    x = y = 0.0
    for r in range(40):
        d = 1.0 if r % 2 == 0 else -1.0
        for _ in range(100):
            pts.append((x, y))
            x += d * s
        for _ in range(3):
            pts.append((x, y))
            y += s
    xy = np.array(pts)
    assert len(xy) == 4120
    k = np.arange(len(xy))
    P = np.c_[xy, 0.3 * np.sin(0.05 * k)] + np.array([100.0, -50.0, 7.0])
    P = np.ascontiguousarray(P[np.random.default_rng(5).permutation(len(P))])
    P.setflags(write=False)
    return P, eps


def bridge():
    """Two blobs X and Y (jittered 6×6×6 lattices of spacing 0.03, 0.15 wide: three times eps = 0.05)
    whose facing sides are 0.09 apart, and ONE point between them, 0.045 from one point of each
    side and farther than eps from every other point: with min_points = 5 it is not core and
    touches a core point of each blob.  Index 0 is the bridge (Open3D first marks it noise, then
    relabels it), index 1 a point of X, 2 … 217 all of Y, 218 … 432 the rest of X with the point
    the bridge touches last: X is cluster 0 through index 1, although the bridge's neighbour in X
    has a higher index than its neighbour in Y.  → (points, eps, min_points, index of the bridge's
    neighbour in X, in Y)."""
    rng = np.random.default_rng(11)
    eps, mp = 0.05, 5
    g = np.arange(6) * 0.03
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    X = lat + rng.uniform(-0.001, 0.001, lat.shape)
    Y = lat + rng.uniform(-0.001, 0.001, lat.shape) + np.array([0.15 + 0.09, 0.0, 0.0])
    tx = int(np.flatnonzero((lat == [0.15, 0.06, 0.06]).all(1))[0])  # X's side facing Y
    ty = int(np.flatnonzero((lat == [0.0, 0.06, 0.06]).all(1))[0])   # Y's side facing X
    mid = np.array([0.15 + 0.045, 0.06, 0.06])
    X[tx] = lat[tx]
    Y[ty] = lat[ty] + np.array([0.15 + 0.09, 0.0, 0.0])
    X = np.concatenate([np.delete(X, tx, axis=0), X[tx][None, :]])  # the touched point last
    P = np.ascontiguousarray(np.concatenate([mid[None, :], X[:1], Y, X[1:]]) + np.array([-3.0, 8.0, 1.0]))
    P.setflags(write=False)
    return P, eps, mp, len(P) - 1, 2 + ty
