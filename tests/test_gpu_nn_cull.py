"""Brute-force NN with the box cull of nn_mfma_kernel: a query block skips the
1024-target tiles its box cannot reach, a wave the 256-target half tiles its own box cannot
reach.  The lemma says the skipped targets have d2f above every search bound concerned, so the
result must not change at all: at every evaluation of a short brute-force loop (the first
unseeded, the later ones seeded by the previous correspondences) the correspondences equal
icp_oracle.nn_exact index for index, with no tolerance, and the loop's points are the oracle's
incremental points bit for bit.

Shapes: the smallest where the skipping can go wrong — more than one 1024-target tile, a ragged
last tile (pads left out of its box), a ragged last 512-query block (a partly empty wave and
wholly empty 32-query groups, which must not widen a box).
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


def _blob(n, seed, centre, scale=0.1):
    """n points (and normals) of the synthetic surface shrunk to radius ≈ 5·scale around centre:
    bumpy, so point-to-plane is well conditioned on it."""
    p, nrm = synth.surface_points(n, seed)
    return p * scale + np.asarray(centre, np.float64), nrm


def _check_loop(src, tgt, nrm, init=None, r=R, n_evals=3):
    """n_evals evaluations from reset(init): each one's points are the oracle's incremental pcd
    (source under init, then moved by every update the device produced) bit for bit, and its
    correspondences the exact fp64 NN of those points, index for index."""
    init = np.eye(4) if init is None else init
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), r, relative_fitness=-1, relative_rmse=-1,
                 max_iteration=n_evals, nn="brute")
    tree = cKDTree(tgt)
    lp.reset(init)
    want = I.initial_points(init, src)
    corrs = []
    for it in range(n_evals):
        lp.step()
        pts = lp.points().cpu().numpy()
        np.testing.assert_array_equal(pts, want, err_msg=f"points, evaluation {it}")
        ref_j, _ = I.nn_exact(tree, tgt, pts, r)
        corr = lp.correspondences().cpu().numpy()
        np.testing.assert_array_equal(corr, ref_j, err_msg=f"evaluation {it}")
        corrs.append(corr)
        want = I.transform_points(lp.result().update, pts)
    return lp.result(), corrs


def _morton_rows(tgt):
    """Operand row of every target: Morton order of the cells of the grid that orders the targets
    (origin = the cloud's minimum, cell CELL, 10 bits per axis: x bit b at key bit 3b, y at 3b + 1,
    z at 3b + 2), the points of one cell in the grid's row-major (z, y, x) cell order, stable in
    the index — the order build_mfma_tiles packs by default.  A numpy model: the grid works on
    centred fp32 coordinates, so only cell memberships with a clear margin are meaningful."""
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


def test_two_clusters_most_tiles_skipped():
    """nt = 3000 (three tiles, the last one partly pads), ns = 700 (a second query block of 188:
    a partly empty wave and wholly empty groups).  Two clusters 25 radii apart along z: each is
    under 16 cells wide and the second starts past z cell 16, so in the Morton order of the cells
    (as in the row-major order) all of the first precedes all of the second and a tile lies in one
    cluster or straddles the gap: most
    (block, tile) pairs are out of reach, and the 188 queries of the last block, all of the
    second cluster, keep none of a launch slice that holds only the first cluster's tile."""
    ta, na = _blob(1500, 1, (0, 0, 0))
    tb, nb = _blob(1500, 2, (0, 0, 3))
    sa, _ = _blob(350, 3, (0, 0, 0))
    sb, _ = _blob(350, 4, (0, 0, 3))
    tgt, nrm = np.vstack([ta, tb]), np.vstack([na, nb])
    T = synth.random_rigid(5, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    src = synth.apply(np.linalg.inv(T), np.vstack([sa, sb]))
    res, corrs = _check_loop(src, tgt, nrm)
    for corr in corrs:  # both clusters register, each onto itself
        assert (corr[:350] >= 0).sum() > 300 and (corr[350:] >= 0).sum() > 300
        assert corr[:350].max() < 1500 and corr[350:][corr[350:] >= 0].min() >= 1500


@pytest.mark.parametrize("ulps", [-4, -1, 0, 1, 4, 16])
def test_radius_boundary_on_an_axis(ulps):
    """G = d2f: one query at x = 0 whose only target in reach sits on the x axis at distance
    d = r moved by `ulps` fp32 neighbours (np.nextafter), i.e. from clearly inside to the zone
    between the fp64 r² and the fp32 bound r2_hi and beyond it.  Every other query near it lies at
    x < 0 and every other target at x > 2, so along x the lone target is the face of its half
    tile's box and the query the face of its wave's box, and the boxes overlap in y and z: the
    box gap is the pair's own d2f, where a non-strict or mis-rounded test would drop the target
    (ulps ≤ 0: a correspondence is lost) or the exact pass would never see it.  The oracle decides
    d² < r² in fp64."""
    d = np.float32(R)
    for _ in range(abs(ulps)):
        d = np.nextafter(d, np.float32(1.0 if ulps > 0 else 0.0), dtype=np.float32)
    tgt_main, nrm_main = _blob(2999, 11, (3, 0, 0))  # x in [2.3, 3.7]: three tiles with the lone one
    src_main, _ = _blob(571, 12, (3, 0, 0))
    rng = np.random.default_rng(13)
    fill = np.column_stack([rng.uniform(-0.5, -0.01, 128), rng.uniform(-0.3, 0.3, 128),
                            rng.uniform(-0.3, 0.3, 128)])  # unmatched queries left of the pair
    q = np.array([[0.0, 0.05, -0.05]])
    lone = q + np.array([[float(d), 0.0, 0.0]])
    tgt = np.vstack([lone, tgt_main])
    nrm = np.vstack([[[1.0, 0.0, 0.0]], nrm_main])
    src = np.vstack([q, fill, src_main])  # ns = 700
    _, corrs = _check_loop(src, tgt, nrm)
    want0 = 0 if (float(d) * float(d) + 0.0) + 0.0 < R * R else -1
    assert corrs[0][0] == want0  # the first evaluation is the constructed one (identity init)
    assert np.all(corrs[0][1:129] == -1)


def test_exact_ties_across_tiles():
    """Two targets in different tiles at the same fp64 distance from a query, the lowest index in
    the LATER tile.  The rows follow the Morton order of the grid's cells, so the pair straddles
    the x = 8 cells plane, where Morton bit 9 flips: `lo` = q − (d, 0, 0) lies in x cell 7 (keys
    below 2⁷), `hi` = q + (d, 0, 0) in x cell 8 (keys ≥ 2⁹), and the 2991 targets of a patch in z
    cells 4–6 (keys 2⁸ … 2⁹ − 1, out of every query's reach) lie between them in row order: `lo`
    in tile 0, `hi` in tile 2 — with 700 queries also different grid.y slices, merged by the
    atomicMin of the keys.  All coordinates of the pairs are dyadic, so the two fp64 distances
    are equal bit for bit; `hi` carries the lower index and must win."""
    rng = np.random.default_rng(31)
    d = 0.09375
    q = np.array([[0.9609375, 0.05 + 0.12 * k, 0.05] for k in range(4)])  # 8·CELL = 0.96096
    hi, lo = q + [d, 0.0, 0.0], q - [d, 0.0, 0.0]

    def patch(n):
        x, y = rng.uniform(0.02, 0.9, n), rng.uniform(0.02, 0.9, n)
        z = 0.7 + 0.1 * np.sin(4.0 * x) * np.cos(4.0 * y)
        gx, gy = 0.4 * np.cos(4.0 * x) * np.cos(4.0 * y), -0.4 * np.sin(4.0 * x) * np.sin(4.0 * y)
        n3 = np.column_stack([-gx, -gy, np.ones(n)])
        return np.column_stack([x, y, z]), n3 / np.linalg.norm(n3, axis=1, keepdims=True)

    pt, pn = patch(2991)
    corner = np.zeros((1, 3))  # the grid's origin
    tgt = np.vstack([hi, lo, corner, pt])  # hi: 0..3, lo: 4..7; nt = 3000
    nrm = np.vstack([np.tile([1.0, 0.0, 0.0], (9, 1)), pn])
    assert np.array_equal(I.sq_dist(q, hi), I.sq_dist(q, lo))
    row = _morton_rows(tgt)
    for k in range(4):
        assert row[k] // 1024 == 2 and row[4 + k] // 1024 == 0, (row[k], row[4 + k])
    ps, _ = patch(696)
    src = np.vstack([q, ps])  # ns = 700
    _, corrs = _check_loop(src, tgt, nrm)
    np.testing.assert_array_equal(corrs[0][:4], np.arange(4))
    assert (corrs[0][4:] >= 0).sum() > 600


def test_rigid_init_boxes_follow_the_transform():
    """A 0.5 rad rotation and a shift of several radii as init: the query boxes must be those of
    the transformed queries.  Boxes of the stored points would skip the tiles the registration
    needs (or keep tiles nothing reaches)."""
    tgt, nrm = _blob(3000, 21, (0.4, -0.3, 0.2))
    smp, _ = _blob(700, 22, (0.4, -0.3, 0.2))
    c, s = np.cos(0.5), np.sin(0.5)
    init = np.array([[c, -s, 0, 0.5], [s, c, 0, -0.4], [0, 0, 1, 0.3], [0, 0, 0, 1.0]])
    src = synth.apply(np.linalg.inv(init), smp)
    assert np.abs(src - smp).max() > 3 * R
    _, corrs = _check_loop(src, tgt, nrm, init=init)
    assert (corrs[0] >= 0).sum() > 600


def test_radius_larger_than_the_cloud_skips_nothing():
    """The `force` path: the threshold leaves the fp16 range, every sub-tile takes the exact path
    and no box is out of reach — every query gets its global nearest target."""
    tgt, nrm = _blob(3000, 3, (0, 0, 0))
    smp, _ = _blob(700, 4, (0, 0, 0), scale=0.1003)
    _, corrs = _check_loop(smp, tgt, nrm, r=50.0)
    assert all((c >= 0).all() for c in corrs)


def test_no_overlap_skips_everything():
    """Source and target 100 units apart: every (block, tile) pair is out of reach, no tile is
    staged or swept; fitness 0 and the transformation stays the identity."""
    tgt, nrm = _blob(3000, 3, (0, 0, 0))
    smp, _ = _blob(700, 4, (100.0, 0, 0))
    res, corrs = _check_loop(smp, tgt, nrm)
    assert all((c == -1).all() for c in corrs)
    assert res.fitness == 0.0
    np.testing.assert_array_equal(res.transformation, np.eye(4))


def test_row_major_slab_tiles():
    """nt = 5000 on a gently curved patch of 6 × 6 units, the shape the choice of the target row
    order is about: in the row-major cell order (M3D_NN_TILE_MORTON=0 builds) a tile is a long
    strip across the whole patch, in the default Morton order a compact square like a query block,
    and the result must be the same either way.  Ragged last tile (5000 = 4 · 1024 + 904) and
    query block."""
    rng = np.random.default_rng(41)

    def patch(n):
        x, y = rng.uniform(0.0, 6.0, n), rng.uniform(0.0, 6.0, n)
        z = 0.3 * np.sin(1.5 * x) * np.cos(1.3 * y)
        gx, gy = 0.45 * np.cos(1.5 * x) * np.cos(1.3 * y), -0.39 * np.sin(1.5 * x) * np.sin(1.3 * y)
        n3 = np.column_stack([-gx, -gy, np.ones(n)])
        return np.column_stack([x, y, z]), n3 / np.linalg.norm(n3, axis=1, keepdims=True)

    tgt, nrm = patch(5000)
    smp, _ = patch(1100)
    T = synth.random_rigid(42, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.03)
    src = synth.apply(np.linalg.inv(T), smp)
    _, corrs = _check_loop(src, tgt, nrm)
    assert (corrs[-1] >= 0).sum() > 800
