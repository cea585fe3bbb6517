"""Brute-force NN with the filtered deferred pass of nn_mfma_kernel: a group whose
every active query starts from a real seed keeps its flagged sub-tiles for after the sweep, and
there a lane runs the sub-tile's screen again and pushes only the rows whose value is negative for
its own query — bit `reg` of its mask is row (reg & 3) + 8·(reg >> 2) + 4·h of the sub-tile, read
from the wave's LDS stash.  The rows left out lie above the query's search bound, so the result
must not change at all: as in test_gpu_nn_reach.py, at each of three evaluations (the first
unseeded, the later ones seeded) the correspondences equal icp_oracle.nn_exact index for index and
the loop's points are the oracle's incremental points bit for bit.

A group is deferred only if every active query in it starts from a real seed, so every test
asserts, on the oracle's result, that all its queries had a correspondence at the earlier
evaluations — otherwise the filtered pass does not run — and states its own premise by an
assertion computed on the CPU.

Shapes: the smallest where the pass can go wrong — winners in every row position of a sub-tile
(both lanes of a pair, all 16 bits of the row map), a lane whose 16 rows are all candidates, ties
and near ties inside one sub-tile across the lane pair, more flagged sub-tiles than any batch
holds, one query, and a second wave of one query.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_oracle as I
from m3d import synth
from m3d.core import Cloud, IcpLoop

pytestmark = pytest.mark.gpu

R = 0.12
CELL = R * 1.001  # the cell size of the grid that orders the targets (m3d_icp_create)
BATCH = 16        # no batch of the deferred pass holds more sub-tiles (nn_mfma_kernel kStash)


def _blob(n, seed, centre, scale=0.1):
    """n points (and normals) of the synthetic surface shrunk to radius ≈ 5·scale around centre."""
    p, nrm = synth.surface_points(n, seed)
    return p * scale + np.asarray(centre, np.float64), nrm


def _check_loop(src, tgt, nrm, init=None, r=R, n_evals=3):
    """n_evals evaluations from reset(init): each one's points are the oracle's incremental pcd
    bit for bit and its correspondences the exact fp64 NN of those points, index for index.
    Returns the result, the correspondences and the update of every evaluation."""
    init = np.eye(4) if init is None else init
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), r, relative_fitness=-1, relative_rmse=-1,
                 max_iteration=n_evals, nn="brute")
    tree = cKDTree(tgt)
    lp.reset(init)
    want = I.initial_points(init, src)
    corrs, updates = [], []
    for it in range(n_evals):
        lp.step()
        pts = lp.points().cpu().numpy()
        np.testing.assert_array_equal(pts, want, err_msg=f"points, evaluation {it}")
        ref_j, _ = I.nn_exact(tree, tgt, pts, r)
        corr = lp.correspondences().cpu().numpy()
        np.testing.assert_array_equal(corr, ref_j, err_msg=f"evaluation {it}")
        corrs.append(corr)
        updates.append(np.array(lp.result().update))
        want = I.transform_points(updates[-1], pts)
    return lp.result(), corrs, updates


def _morton_rows(tgt):
    """Operand row of every target (numpy model of build_mfma_tiles' default order): Morton order
    of the cells of the grid that orders the targets (origin = the cloud's minimum, cell CELL, 10
    bits per axis, x bit b at key bit 3b), the points of one cell in row-major (z, y, x) cell
    order, stable in the index."""
    c = np.floor((tgt - tgt.min(axis=0)) / CELL).astype(np.int64)
    assert c.max() < 1024
    key = np.zeros(len(tgt), np.int64)
    for b in range(10):
        for a in range(3):
            key |= ((c[:, a] >> b) & 1) << (3 * b + a)
    cell_order = np.lexsort((np.arange(len(tgt)), c[:, 0], c[:, 1], c[:, 2]))
    order = cell_order[np.argsort(key[cell_order], kind="stable")]
    row = np.empty(len(tgt), np.int64)
    row[order] = np.arange(len(tgt))
    return row


def _all_seeded(corrs):
    """every query had a correspondence at every evaluation but the last: the later evaluations
    start every group from real seeds, which is what defers it"""
    return all((c >= 0).all() for c in corrs[:-1])


def test_every_row_position():
    """nt = 3000 (three tiles, the last ragged: its last sub-tile holds pads), ns = 700 queries
    drawn next to targets.  Premise: at both seeded evaluations the winners' operand rows cover
    all 32 values of row % 32 — both lanes of the pair and all 16 bits of the bit → row map carry
    a winner that only the filtered push can have delivered."""
    tgt, nrm = _blob(3000, 21, (0, 0, 0))
    rng = np.random.default_rng(22)
    pick = rng.choice(3000, 700, replace=False)
    smp = tgt[pick] + rng.normal(0.0, 0.004, (700, 3))
    T = synth.random_rigid(23, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    src = synth.apply(np.linalg.inv(T), smp)
    _, corrs, _ = _check_loop(src, tgt, nrm)
    assert _all_seeded(corrs)
    row = _morton_rows(tgt)
    for corr in corrs[1:]:
        assert len(set(row[corr] % 32)) == 32
    assert row.max() // 32 == 93 and 3000 % 32 != 0  # the last sub-tile is ragged


def _perp(v):
    """a unit vector perpendicular to each row of v"""
    a = np.cross(v, [0.0, 0.0, 1.0])
    b = np.cross(v, [0.0, 1.0, 0.0])
    p = np.where((np.linalg.norm(a, axis=1) > np.linalg.norm(b, axis=1))[:, None], a, b)
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def test_lane_with_sixteen_hits():
    """One query with 32 targets on a sphere around it, radius 0.05·(1 + k·2⁻²³): distinct in fp32
    and, squared, within 7.4e-6 of each other — band_of alone widens the bound by more than 1.2e-5
    (nnkey.h: ×1.000004 on the root and twice on the square, plus the absolute term that covers the
    fp32 rounding of the coordinates), so at a seeded evaluation every one of the 32 lies inside
    the query's search bound and must be flagged.  The sphere sits inside one grid cell of its own
    and filler targets at the grid origin (Morton key 0: the first rows) are added until the 32
    occupy one aligned sub-tile: each lane of the query's pair then has 16 hits and its bit loop
    runs 16 iterations, while the wave's other 63 queries — copies of lone targets three cells
    apart — have one candidate each and idle.  Residuals are zero by construction (the copies;
    the sphere's normals are perpendicular to its radii), so the three evaluations see the same
    geometry.  The nearest in fp64, k = 0, must win."""
    rng = np.random.default_rng(41)
    q = np.array([[1.5 * CELL, 1.5 * CELL, 5.5 * CELL]])
    u = rng.normal(size=(32, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    rad = 0.05 * (1.0 + np.arange(32) * 2.0 ** -23)
    sphere = q + u * rad[:, None]
    gi, gj = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    lone = np.column_stack([0.3 + 0.36 * gi.ravel(), 0.3 + 0.36 * gj.ravel(), np.full(64, 0.3)])[:63]
    ln = rng.normal(size=(63, 3))
    ln /= np.linalg.norm(ln, axis=1, keepdims=True)
    for nfill in range(1, 34):  # at least the corner itself: the grid's origin
        fill = np.column_stack([1.0e-4 * np.arange(nfill), np.zeros(nfill), np.zeros(nfill)])
        tgt = np.vstack([sphere, lone, fill])
        rows = _morton_rows(tgt)[:32]
        if rows.min() % 32 == 0 and rows.max() == rows.min() + 31:
            break
    else:
        raise AssertionError("the sphere's 32 targets never fill one aligned sub-tile")
    nrm = np.vstack([_perp(u), ln, np.tile([0.0, 0.0, 1.0], (nfill, 1))])
    # the premise: one aligned sub-tile (above), all 32 inside the seeded bound, one candidate for
    # every other query (its own target; the next one is three cells away)
    d2 = I.sq_dist(np.repeat(q, 32, axis=0), sphere)
    assert np.all(np.diff(np.sqrt(d2).astype(np.float32)) > 0)
    assert d2.max() <= d2.min() * (1.0 + 1.0e-5)
    dist, _ = cKDTree(tgt).query(lone, k=2)
    assert dist[:, 1].min() > 2.9 * CELL
    src = np.vstack([q, lone])  # ns = 64: one wave
    _, corrs, _ = _check_loop(src, tgt, nrm)
    assert _all_seeded(corrs)
    for corr in corrs:
        assert corr[0] == 0
        np.testing.assert_array_equal(corr[1:], 32 + np.arange(63))


@pytest.mark.parametrize("case", ["tie", "ulp_hi_nearer", "ulp_lo_nearer"])
def test_near_tie_inside_one_subtile(case):
    """Two targets equidistant (or nearly) from a query, in the same sub-tile but in the two lanes
    of the query's pair, under the tight bound of a seeded evaluation.  The construction of
    test_gpu_nn_reach.py's test_near_tie_across_tiles_seeded with the pair inside one cell: four
    queries at x = 7/16 in cell (3, 0, 0), `hi` = q + (d, 0, 0), `lo` = q − (d, 0, 0) with
    d = 5/128 (dyadic: the fp64 distances are exact), `hi` carrying the lower index.  The cell
    holds these eight targets only and, with the corner and three fillers in the origin's cell
    before it, they take rows 4–11: `hi` 4–7 and `lo` 8–11 differ in (row >> 2) & 1, so one lane of
    the pair holds `hi` and the other `lo`, and only the pair merge after the list compares them.
    Zero residuals (the pair's normals along z, every other source point a copy of its target):
    the update is the identity and all three evaluations see the same geometry.
      tie: equal bit for bit: `hi` (lower index) wins every evaluation.
      ulp_*: d² = 25/16384 has an even exponent, so an offset of 2⁻³¹ in y adds exactly one fp64
        ulp (2⁻⁶²) to the squared distance of the target that carries it and nothing to the fp32
        distance: the other target is nearer in fp64 and must win, whichever its index — which
        happens only if it was pushed and near2 landed in the band."""
    rng = np.random.default_rng(31)
    d = 0.0390625
    q = np.array([[0.4375, 0.03 + 0.02 * k, 0.05] for k in range(4)])
    hi, lo = q + [d, 0.0, 0.0], q - [d, 0.0, 0.0]
    if case == "ulp_hi_nearer":
        lo = lo + [0.0, 2.0 ** -31, 0.0]
    if case == "ulp_lo_nearer":
        hi = hi + [0.0, 2.0 ** -31, 0.0]

    x, y = rng.uniform(0.02, 0.9, 2988), rng.uniform(0.02, 0.9, 2988)
    z = 0.7 + 0.1 * np.sin(4.0 * x) * np.cos(4.0 * y)
    gx, gy = 0.4 * np.cos(4.0 * x) * np.cos(4.0 * y), -0.4 * np.sin(4.0 * x) * np.sin(4.0 * y)
    n3 = np.column_stack([-gx, -gy, np.ones(2988)])
    pt, pn = np.column_stack([x, y, z]), n3 / np.linalg.norm(n3, axis=1, keepdims=True)

    corner = np.column_stack([1.0e-3 * np.arange(4), np.zeros(4), np.zeros(4)])  # the grid's origin
    tgt = np.vstack([hi, lo, corner, pt])  # hi: 0..3, lo: 4..7; nt = 3000
    nrm = np.vstack([np.tile([0.0, 0.0, 1.0], (12, 1)), pn])
    dh, dl = I.sq_dist(q, hi), I.sq_dist(q, lo)
    if case == "tie":
        assert np.array_equal(dh, dl)
    elif case == "ulp_hi_nearer":
        assert np.array_equal(np.nextafter(dh, np.inf), dl)
    else:
        assert np.array_equal(np.nextafter(dl, np.inf), dh)
    row = _morton_rows(tgt)
    np.testing.assert_array_equal(row[:8], 4 + np.arange(8))  # one sub-tile, hi and lo in different lanes
    assert np.all((row[:4] >> 2) & 1 != (row[4:8] >> 2) & 1)
    src = np.vstack([q, pt[:696]])  # ns = 700
    _, corrs, updates = _check_loop(src, tgt, nrm)
    assert _all_seeded(corrs)
    for u in updates:  # the premise of "the same geometry three times"
        np.testing.assert_array_equal(u, np.eye(4))
    want = np.arange(4) + (4 if case == "ulp_lo_nearer" else 0)
    for corr in corrs:
        np.testing.assert_array_equal(corr[:4], want)
        np.testing.assert_array_equal(corr[4:], 12 + np.arange(696))


def test_more_subtiles_than_one_batch():
    """ns = 64: one wave whose queries sit next to a scattered 64-subset of an nt = 3000 blob, so
    that the wave flags far more sub-tiles than one batch of the deferred pass holds and its stash
    is overwritten between batches.  Premise, from the row model: at both seeded evaluations the
    winners alone lie in more than 2·BATCH distinct sub-tiles, more than BATCH of them in one
    tile (one list entry)."""
    tgt, nrm = _blob(3000, 51, (0, 0, 0))
    rng = np.random.default_rng(52)
    pick = rng.choice(3000, 64, replace=False)
    smp = tgt[pick] + rng.normal(0.0, 0.004, (64, 3))
    T = synth.random_rigid(53, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    src = synth.apply(np.linalg.inv(T), smp)
    _, corrs, _ = _check_loop(src, tgt, nrm)
    assert _all_seeded(corrs)
    row = _morton_rows(tgt)
    for corr in corrs[1:]:
        subs = np.unique(row[corr] // 32)
        assert len(subs) > 2 * BATCH
        assert np.bincount(subs // 32).max() > BATCH


@pytest.mark.parametrize("ns", [1, 65])
def test_one_query_and_a_second_wave_of_one(ns):
    """ns = 1: 63 inactive lanes and an empty second group; ns = 65: a second wave with a single
    query.  Against nt = 3000 (three tiles, ragged), the radius of the other tests.  The inactive
    lanes carry the threshold −1, so their masks must be empty, and a wave of one query must
    still end its bit loop."""
    tgt, nrm = _blob(3000, 3, (0, 0, 0))
    smp, _ = _blob(ns, 4, (0, 0, 0), scale=0.1003)
    _, corrs, _ = _check_loop(smp, tgt, nrm)
    assert _all_seeded(corrs)
