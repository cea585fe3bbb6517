"""Edge-case inputs for the preprocessing and feature-matching kernels (prep.hip, feat.hip) and a
census, on the CPU oracle alone, of which code paths those inputs reach.

* ``zoo()``: small named clouds with their (radius, max_nn) and, for some, given normals:
  exact planes (axis-aligned and tilted), lines, duplicated and coinciding points, isolated
  points, pairs and triples, a cloud far from the origin, points stacked along the normal, and
  clusters whose FPFH swap tests are near ties;
* ``eigen_path``: which return of FastEigen3x3 the oracle takes for a covariance;
* ``normal_stable_mask``: the rows whose oracle normal does not depend on the last bit of the
  solver's ``acos`` / ``cos`` (the one thing a second correct implementation may do differently);
* ``feature_split``: feat.hip's host arithmetic restated (what a (queries, references) shape
  reaches: slices, tiles per slice, the last slice and tile);
* ``tied_features`` / ``random_features``: feature rows with and without exact ties.

tests/test_prep_zoo_cpu.py asserts the census; tests/test_gpu_prep_edges.py runs the device on
the same inputs.
"""
import itertools
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import prep_oracle as P
from m3d import synth

EIGEN_PATHS = ("zero", "diag-x", "diag-y", "diag-z", "pos-v2", "pos-v1", "pos-cross", "neg-v0", "neg-v1",
               "neg-cross")
LIBM_FREE_PATHS = ("zero", "diag-x", "diag-y", "diag-z")  # returns that involve no acos / cos
STABLE_TOL = 1e-12
FPFH_MAX_NN = 60  # FPFH runs at radius 2·r, max_nn 60 on every cloud

# feat.hip: kFnnBlock, kFnnTile, the block target and the grid.y limit of feature_nn
FNN_BLOCK, FNN_TILE, FNN_TARGET, FNN_MAX_SLICES = 128, 64, 2048, 65535


def _lattice2(n, spacing):
    g = np.arange(n) * spacing
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def tilt():
    """The rotation of ``tilted_plane``."""
    return synth.random_rigid(5, rot_range=1.0, trans_range=0)[:3, :3]


def line_direction():
    return np.array([1.0, 2.0, 3.0]) / math.sqrt(14.0)


def _sparse():
    """40 points 10 apart on x; points 0-9 have a companion 0.05 along x, 5-9 another along y,
    10-14 one along z: neighbour counts 1 (25 points), 2 (20) and 3 (15)."""
    base = np.zeros((40, 3))
    base[:, 0] = 10.0 * np.arange(40)
    return np.concatenate([base, base[0:10] + [0.05, 0, 0], base[5:10] + [0, 0.05, 0],
                           base[10:15] + [0, 0, 0.05]])


def _build():
    rng = np.random.default_rng(20)
    z = {}
    lat = _lattice2(20, 0.1)
    zero = np.zeros(len(lat))
    z["lattice_plane"] = (np.c_[lat, zero], 0.25, 30, None)
    z["plane_x"] = (np.c_[zero, lat], 0.25, 30, None)
    z["plane_y"] = (np.c_[lat[:, 0], zero, lat[:, 1]], 0.25, 30, None)
    flat = np.c_[rng.uniform(-1, 1, (500, 2)), np.zeros(500)]
    z["tilted_plane"] = (flat @ tilt().T + np.array([3.0, -7.0, 11.0]), 0.3, 30, None)
    z["line"] = (rng.uniform(-1, 1, 200)[:, None] * line_direction()[None, :], 0.2, 30, None)
    z["axis_line"] = (np.c_[np.zeros(200), rng.uniform(-1, 1, 200), np.zeros(200)], 0.2, 30, None)
    z["duplicates"] = (np.repeat(rng.normal(size=(100, 3)), 5, axis=0), 0.8, 30, None)
    z["all_same"] = (np.tile(np.array([[1.5, -2.25, 0.75]]), (70, 1)), 0.5, 30, None)
    z["sparse"] = (_sparse(), 0.5, 30, None)
    z["far_offset"] = (synth.surface_points(1200, seed=2)[0] + np.array([2e4, -1e4, 5e3]), 0.8, 30, None)
    col = np.c_[_lattice2(7, 1.0), np.zeros(49)]
    stack = np.concatenate([col, col + [0, 0, 0.1], col + [0, 0, 0.2]])
    z["stack"] = (stack, 1.2, 30, np.tile([0.0, 0.0, 1.0], (len(stack), 1)))
    # 30 isolated pairs 0.05 apart in random directions: every count is 2, so the covariance must
    # be the identity (a pair's own covariance has rank 1 and an oblique null space)
    u = rng.normal(size=(30, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    first = np.c_[10.0 * np.arange(30), np.zeros(30), np.zeros(30)]
    z["pairs"] = (np.concatenate([first, first + 0.05 * u]), 0.5, 30, None)
    # 60 clusters of 8 points within 0.2 of centres 10 apart: the points of a cluster share one
    # neighbour set in different orders, so their normals differ by ulps and every pair's swap
    # test acos|a1| > acos|a2| is a near tie
    centres = np.repeat(np.c_[10.0 * np.arange(60), np.zeros(60), np.zeros(60)], 8, axis=0)
    z["clusters"] = (centres + rng.uniform(-0.115, 0.115, (480, 3)), 0.8, 30, None)
    out = {}
    for name, (pts, radius, max_nn, nrm) in z.items():
        pts = np.ascontiguousarray(pts, np.float64)
        pts.setflags(write=False)
        if nrm is not None:
            nrm = np.ascontiguousarray(nrm, np.float64)
            nrm.setflags(write=False)
        out[name] = SimpleNamespace(name=name, points=pts, radius=radius, max_nn=max_nn, normals=nrm)
    return out


@lru_cache(maxsize=None)
def zoo():
    """name → namespace(name, points, radius, max_nn, normals or None); arrays are read-only."""
    return _build()


def eigen_path(cov):
    return P.fast_eigen3x3_path(cov)[1]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@lru_cache(maxsize=None)
def nbrs(name, fpfh=False):
    """The oracle's hybrid lists of a zoo cloud at its own (radius, max_nn), or at the FPFH
    parameters (2·radius, 60).  Computed once per session."""
    c = zoo()[name]
    r, k = (2 * c.radius, FPFH_MAX_NN) if fpfh else (c.radius, c.max_nn)
    return _frozen(*P.hybrid_search(c.points, r, k))


@lru_cache(maxsize=None)
def oracle_normals(name):
    """→ (normals without orientation, eigen path per row) of a zoo cloud."""
    c = zoo()[name]
    idx, _, cnt = nbrs(name)
    cov = P.covariance(c.points, idx, cnt)
    paths = np.array([eigen_path(cov[i]) for i in range(len(cov))])
    nrm = P.estimate_normals(c.points, c.radius, c.max_nn, nbrs=nbrs(name))
    return _frozen(nrm, paths)


def _bumped(fn, ulps):
    if ulps == 0:
        return fn
    to = math.inf if ulps > 0 else -math.inf
    return lambda x: math.nextafter(fn(x), to)


def _normal_of(cov, acos, cos1, cos2):
    """estimate_normals' row without given normals, the solver's cos(angle) and
    cos(angle + 2π/3) taken from two functions."""
    calls = iter((cos1, cos2))
    n, _ = P.fast_eigen3x3_path(cov, acos=acos, cos=lambda x: next(calls)(x))
    if n[0] == 0 and n[1] == 0 and n[2] == 0:
        n = np.array([0.0, 0.0, 1.0])
    return n


def normal_spread(points, radius, max_nn, lists=None):
    """Per row: the largest move of the oracle's own normal when FastEigen3x3's acos and its two
    cos results are each bumped by one ulp, up or down (all 26 combinations)."""
    p = np.asarray(points, np.float64)
    idx, _, cnt = lists if lists is not None else P.hybrid_search(p, radius, max_nn)
    cov = P.covariance(p, idx, cnt)
    out = np.zeros(len(p))
    bumps = [b for b in itertools.product((-1, 0, 1), repeat=3) if b != (0, 0, 0)]
    for i in range(len(p)):
        base, path = P.fast_eigen3x3_path(cov[i])
        if path in LIBM_FREE_PATHS:
            continue
        for ba, b1, b2 in bumps:
            n = _normal_of(cov[i], _bumped(math.acos, ba), _bumped(math.cos, b1), _bumped(math.cos, b2))
            out[i] = max(out[i], float(np.abs(n - base).max()))
    return out


def normal_stable_mask(points, radius, max_nn, lists=None):
    return normal_spread(points, radius, max_nn, lists) < STABLE_TOL


@lru_cache(maxsize=None)
def stable(name):
    c = zoo()[name]
    spread, = _frozen(normal_spread(c.points, c.radius, c.max_nn, nbrs(name)))
    return spread < STABLE_TOL, spread


# name → the normals FPFH runs on: given ones, or the oracle's own
FPFH_CLOUDS = ("sparse", "all_same", "duplicates", "axis_line", "far_offset", "stack", "lattice_plane",
               "tilted_plane", "clusters")


def fpfh_normals(name):
    c = zoo()[name]
    if name == "lattice_plane":
        return np.tile([0.0, 0.0, 1.0], (len(c.points), 1))
    if name == "tilted_plane":
        return np.tile(tilt() @ np.array([0.0, 0.0, 1.0]), (len(c.points), 1))
    return c.normals if c.normals is not None else oracle_normals(name)[0]


@lru_cache(maxsize=None)
def fpfh_case(name):
    """→ (normals, oracle FPFH, bin-edge flags, neighbour count) of an FPFH cloud.  The flags are
    ``spfh_edge_sensitive`` with delta 1e-12 and no swap excuse (the device decides the swap test
    exactly)."""
    c = zoo()[name]
    nrm = fpfh_normals(name)
    idx, d2, cnt = nbrs(name, fpfh=True)
    ref = P.compute_fpfh(c.points, nrm, 2 * c.radius, FPFH_MAX_NN, nbrs=(idx, d2, cnt))
    flags = P.spfh_edge_sensitive(c.points, nrm, idx, cnt, delta=1e-12, delta_swap=0.0)
    return _frozen(np.ascontiguousarray(nrm, np.float64), ref, flags, cnt)


def swap_near_ties(name, tol=1e-14):
    """→ (pairs of the FPFH lists, pairs whose swap test has ||a1| − |a2|| < tol, of those the
    exact ties)."""
    c = zoo()[name]
    nrm = fpfh_normals(name)
    idx, _, cnt = nbrs(name, fpfh=True)
    pairs = near = ties = 0
    for i in range(len(c.points)):
        for k in range(1, int(cnt[i])):
            j = idx[i, k]
            dp = c.points[j] - c.points[i]
            f3 = math.sqrt(P._dot(dp, dp))
            if f3 == 0.0:
                continue
            a1, a2 = abs(P._dot(nrm[i], dp) / f3), abs(P._dot(nrm[j], dp) / f3)
            pairs += 1
            near += abs(a1 - a2) < tol
            ties += a1 == a2
    return pairs, near, ties


# ------------------------------------------------------------------------------- feature 1-NN
def feature_split(nq, nr):
    """feature_nn's launch arithmetic (feat.hip) → namespace(blocks, slices, slice_len,
    tiles_per_slice, last_slice, last_tile, last_block_lanes): query blocks of 128, reference
    slices rounded to 64-row tiles with about 2048 blocks in all; ``last_slice`` and
    ``last_tile`` are the reference counts of the last slice and of its last tile."""
    bx = (nq + FNN_BLOCK - 1) // FNN_BLOCK
    s = max(1, min((FNN_TARGET + bx - 1) // bx, (nr + FNN_TILE - 1) // FNN_TILE))
    s = min(s, FNN_MAX_SLICES)
    slice_len = (nr + s - 1) // s
    slice_len = (slice_len + FNN_TILE - 1) // FNN_TILE * FNN_TILE
    s = max(1, (nr + slice_len - 1) // slice_len)
    last_slice = nr - (s - 1) * slice_len
    return SimpleNamespace(blocks=bx, slices=s, slice_len=slice_len, tiles_per_slice=slice_len // FNN_TILE,
                           last_slice=last_slice, last_tile=(last_slice - 1) % FNN_TILE + 1,
                           last_block_lanes=(nq - 1) % FNN_BLOCK + 1)


def random_features(n, seed):
    """n×33 rows uniform in [0, 200), the range of FPFH bins."""
    return np.random.default_rng(seed).uniform(0.0, 200.0, (n, 33))


def tied_features(nq, nr, seed):
    """→ (queries nq×33, references nr×33, query base row, reference base row).  ``nr // 4`` base
    rows; every reference and every query is an exact copy of a random base row, so a query's
    minimum is 0 wherever its base row stands among the references: about four tied places."""
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.0, 200.0, (max(nr // 4, 1), 33))
    rb = rng.integers(0, len(base), nr)
    qb = rng.integers(0, len(base), nq)
    return base[qb], base[rb], qb, rb


def tie_census(nq, nr, seed):
    """How many queries of ``tied_features`` put the lowest-index rule to work: → (queries whose
    tied minima lie in more than one slice, queries with minima in more than one tile of some
    slice, queries with minima in more than one tile of the first slice that holds a minimum —
    where a wrong choice inside the slice survives the merge)."""
    _, _, qb, rb = tied_features(nq, nr, seed)
    sp = feature_split(nq, nr)
    where = {}
    for j, b in enumerate(rb):
        where.setdefault(int(b), []).append(j)
    across_slices = across_tiles = across_tiles_first = 0
    for b in qb:
        pos = where.get(int(b), [])
        if len(pos) < 2:
            continue
        slices = [j // sp.slice_len for j in pos]
        across_slices += len(set(slices)) > 1
        tiles = {}
        for j, s in zip(pos, slices):
            tiles.setdefault(s, set()).add(j // FNN_TILE)
        across_tiles += any(len(t) > 1 for t in tiles.values())
        across_tiles_first += len(tiles[slices[0]]) > 1
    return across_slices, across_tiles, across_tiles_first


FEATURE_SHAPES = ((1, 1), (5, 3), (129, 63), (130, 65), (200, 131), (3001, 9000), (8193, 4099), (16385, 1027))
TIED_SHAPES = FEATURE_SHAPES[3:]


def shape_seed(ns, nt):
    return 1000 * ns + nt


@lru_cache(maxsize=None)
def feature_case(ns, nt, tied):
    """→ (source rows, target rows, oracle correspondences without and with the mutual filter)."""
    if tied:
        fs, ft, _, _ = tied_features(ns, nt, shape_seed(ns, nt))
    else:
        fs, ft = random_features(ns, shape_seed(ns, nt)), random_features(nt, shape_seed(ns, nt) + 1)
    fs, ft = np.ascontiguousarray(fs), np.ascontiguousarray(ft)
    return _frozen(fs, ft, P.correspondences_from_features(fs, ft, False),
                   P.correspondences_from_features(fs, ft, True))


# ------------------------------------------------------------------------------- hybrid search
# (radius, k) on synth.surface_points(4000, seed=1): each k of a template boundary
# (lists of 1 / 2 / 4 slots per lane at k ≤ 64 / ≤ 128 / ≤ 256) with full and short lists
HYBRID_BOUNDARIES = ((1.2, 63), (1.2, 64), (1.2, 65), (1.7, 127), (1.7, 128), (2.4, 255), (2.4, 256))
HYBRID_SMALL_K = ((1.2, 1), (1.2, 2))


@lru_cache(maxsize=None)
def hybrid_points():
    pts, = _frozen(synth.surface_points(4000, seed=1)[0])
    return pts


@lru_cache(maxsize=None)
def hybrid_case(radius, k):
    return _frozen(*P.hybrid_search(hybrid_points(), radius, k))
