"""Brute-force NN with the per-query reach test of nn_mfma_kernel: behind the
box-vs-box cull a wave keeps a 256-target half tile only if one of its queries reaches the half's
box with its own search bound, and a block keeps a tile only if one of its waves keeps one of its
halves (the waves' masks are ORed through LDS, one barrier per round of 16 tiles).  The lemma is
the box cull's with the query box shrunk to a point, so the result must not change at all: as in
test_gpu_nn_cull.py, at each of three evaluations (the first unseeded, the later ones seeded by
the previous correspondences, i.e. with per-query bounds far below r²) the correspondences equal
icp_oracle.nn_exact index for index and the loop's points are the oracle's incremental points bit
for bit.

Shapes: the smallest where the test can go wrong — a wave whose queries sit in two distant blobs
(its box spans everything between them), one reaching query among 63 that reach nothing, ties
and near ties across tiles under a tight seeded bound, one query, a second wave of one query, and
the smallest launch in which a block runs a second round of 16 tiles (LDS slots reused).
"""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import icp_oracle as I
from m3d import synth
from m3d.core import Cloud, IcpLoop

pytestmark = pytest.mark.gpu

R = 0.12
CELL = R * 1.001  # the cell size of the grid that orders the targets (m3d_icp_create)


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


def test_wave_straddles_two_blobs():
    """ns = 96: 40 queries in a blob at the origin, then 56 in a blob 25 radii away along z, so
    the first wave (slots 0–63) holds 40 of the one and 24 of the other and its box spans the
    whole gap.  nt = 3000: a tile's worth of targets at each blob and, between them, a patch of
    952 that lies inside that wave's box and more than r from every query: the box test keeps its
    half tiles for the wave, no query reaches them.  Both blobs must register onto themselves."""
    ta, na = _blob(1024, 1, (0, 0, 0))
    tb, nb = _blob(1024, 2, (0, 0, 3))
    rng = np.random.default_rng(5)
    mid = np.column_stack([rng.uniform(-0.2, 0.2, 952), rng.uniform(-0.2, 0.2, 952), rng.uniform(1.2, 1.8, 952)])
    sa, _ = _blob(40, 3, (0, 0, 0))
    sb, _ = _blob(56, 4, (0, 0, 3))
    tgt = np.vstack([ta, tb, mid])
    nrm = np.vstack([na, nb, np.tile([0.0, 0.0, 1.0], (952, 1))])
    smp = np.vstack([sa, sb])
    # the premise: the patch inside the first wave's box, out of every query's reach
    lo, hi = smp[:64].min(axis=0), smp[:64].max(axis=0)
    assert np.all(mid >= lo - R) and np.all(mid <= hi + R)
    assert cKDTree(smp).query(mid)[0].min() > 3 * R
    T = synth.random_rigid(5, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    src = synth.apply(np.linalg.inv(T), smp)
    _, corrs, _ = _check_loop(src, tgt, nrm)
    for corr in corrs:
        assert (corr[:40] >= 0).sum() > 30 and (corr[40:] >= 0).sum() > 45
        assert corr[:40].max() < 1024
        assert corr[40:][corr[40:] >= 0].min() >= 1024 and corr[40:].max() < 2048


@pytest.mark.parametrize("ulps", [-4, -1, 0, 1, 4, 16])
def test_one_reaching_lane(ulps):
    """One query of the first wave is the only one within reach of a lone target; the wave's other
    63 queries reach nothing at all, so that one lane's test alone keeps the half tile for the
    wave and the tile for the block.  The lone target sits on the x axis of the query at distance
    d = r moved by `ulps` fp32 neighbours and is the x face of its half tile's box (every other
    target lies at x > 2, the boxes overlap in y and z): the query's gap to the box is the pair's
    own d2f, from clearly inside to the zone between the fp64 r² and the fp32 bound and beyond.
    The oracle decides d² < r² in fp64."""
    d = np.float32(R)
    for _ in range(abs(ulps)):
        d = np.nextafter(d, np.float32(1.0 if ulps > 0 else 0.0), dtype=np.float32)
    tgt_main, nrm_main = _blob(2999, 11, (3, 0, 0))  # x in [2.3, 3.7]
    src_main, _ = _blob(300, 12, (3, 0, 0))
    rng = np.random.default_rng(13)
    fill = np.column_stack([rng.uniform(-0.5, -0.01, 63), rng.uniform(-0.3, 0.3, 63),
                            rng.uniform(-0.3, 0.3, 63)])  # x ≤ −0.01: more than r from the lone target
    q = np.array([[0.0, 0.05, -0.05]])
    lone = q + np.array([[float(d), 0.0, 0.0]])
    tgt = np.vstack([lone, tgt_main])
    nrm = np.vstack([[[1.0, 0.0, 0.0]], nrm_main])
    src = np.vstack([q, fill, src_main])  # wave 0 = the query and the 63; ns = 364
    _, corrs, _ = _check_loop(src, tgt, nrm)
    want0 = 0 if (float(d) * float(d) + 0.0) + 0.0 < R * R else -1
    assert corrs[0][0] == want0  # the first evaluation is the constructed one (identity init)
    assert np.all(corrs[0][1:64] == -1)


@pytest.mark.parametrize("case", ["tie", "ulp_hi_nearer", "ulp_lo_nearer"])
def test_near_tie_across_tiles_seeded(case):
    """Two targets in different tiles, equidistant (or nearly) from a query, under the tight bound
    of a seeded evaluation.  The Morton-cell construction of test_gpu_nn_cull.py's
    test_exact_ties_across_tiles: the pair straddles the x = 8 cells plane, `lo` = q − (d, 0, 0)
    in x cell 7 (tile 0), `hi` = q + (d, 0, 0) in x cell 8 (tile 2), a patch in z cells 4–6
    between them in row order; `hi` carries the lower index.  Every source point other than the
    four queries is a copy of a patch target and the pair's normals are along z, so every
    residual is exactly zero, the update is the identity and all three evaluations see the same
    geometry — the second and third with X = band_of(d²), barely above the distance of the other
    target, whose half tile the query must still reach.
      tie: dyadic coordinates, the two fp64 distances equal bit for bit: `hi` (lower index, later
        tile) wins every evaluation.
      ulp_*: d² = 25/4096 has an even exponent, so an offset of 2⁻³⁰ in y adds exactly one fp64
        ulp (2⁻⁶⁰) to the squared distance of the target that carries it and nothing to the fp32
        distance: the other target is nearer in fp64 and must win, whichever its index."""
    rng = np.random.default_rng(31)
    d = 0.09375 if case == "tie" else 0.078125
    q = np.array([[0.9609375, 0.05 + 0.12 * k, 0.05] for k in range(4)])  # 8·CELL = 0.96096
    hi, lo = q + [d, 0.0, 0.0], q - [d, 0.0, 0.0]
    if case == "ulp_hi_nearer":
        lo = lo + [0.0, 2.0 ** -30, 0.0]
    if case == "ulp_lo_nearer":
        hi = hi + [0.0, 2.0 ** -30, 0.0]

    x, y = rng.uniform(0.02, 0.9, 2991), rng.uniform(0.02, 0.9, 2991)
    z = 0.7 + 0.1 * np.sin(4.0 * x) * np.cos(4.0 * y)
    gx, gy = 0.4 * np.cos(4.0 * x) * np.cos(4.0 * y), -0.4 * np.sin(4.0 * x) * np.sin(4.0 * y)
    n3 = np.column_stack([-gx, -gy, np.ones(2991)])
    pt, pn = np.column_stack([x, y, z]), n3 / np.linalg.norm(n3, axis=1, keepdims=True)

    corner = np.zeros((1, 3))  # the grid's origin
    tgt = np.vstack([hi, lo, corner, pt])  # hi: 0..3, lo: 4..7; nt = 3000
    nrm = np.vstack([np.tile([0.0, 0.0, 1.0], (9, 1)), pn])
    dh, dl = I.sq_dist(q, hi), I.sq_dist(q, lo)
    if case == "tie":
        assert np.array_equal(dh, dl)
    elif case == "ulp_hi_nearer":
        assert np.array_equal(np.nextafter(dh, np.inf), dl)
    else:
        assert np.array_equal(np.nextafter(dl, np.inf), dh)
    row = _morton_rows(tgt)
    for k in range(4):
        assert row[k] // 1024 == 2 and row[4 + k] // 1024 == 0, (row[k], row[4 + k])
    src = np.vstack([q, pt[:696]])  # ns = 700
    _, corrs, updates = _check_loop(src, tgt, nrm)
    for u in updates:  # the premise of "the same geometry three times"
        np.testing.assert_array_equal(u, np.eye(4))
    want = np.arange(4) + (4 if case == "ulp_lo_nearer" else 0)
    for corr in corrs:
        np.testing.assert_array_equal(corr[:4], want)
        np.testing.assert_array_equal(corr[4:], 9 + np.arange(696))


@pytest.mark.parametrize("mode", ["near", "force", "apart"])
@pytest.mark.parametrize("ns", [1, 65])
def test_one_query_and_a_second_wave_of_one(ns, mode):
    """ns = 1: 63 inactive lanes and an empty second group; ns = 65: a second wave with a single
    query, six waves without any.  Against nt = 3000 (three tiles, ragged).  near: the radius of
    the other tests; force: r = 50, the threshold leaves the fp16 range, every sub-tile takes the
    exact path and nothing may be skipped; apart: the clouds 100 units apart, everything skipped,
    fitness 0 and the identity."""
    tgt, nrm = _blob(3000, 3, (0, 0, 0))
    smp, _ = _blob(ns, 4, (100.0 if mode == "apart" else 0.0, 0, 0), scale=0.1003)
    res, corrs, _ = _check_loop(smp, tgt, nrm, r=50.0 if mode == "force" else R)
    if mode == "force":
        assert all((c >= 0).all() for c in corrs)
    if mode == "apart":
        assert all((c == -1).all() for c in corrs)
        assert res.fitness == 0.0
        np.testing.assert_array_equal(res.transformation, np.eye(4))


def test_two_cull_rounds_per_block():
    """The smallest launch in which a block's strided tile set exceeds the 16 tiles of one cull
    round, so that the cross-wave OR and its LDS slots are used a second time: 65 query blocks
    (ns = 33 000) make grid.y at most ⌈slots / 65⌉ with slots = 2 resident blocks per CU, and
    16·⌈slots / 65⌉ + 9 tiles give every block of the first slices at least 17 tiles whether the
    launcher rounds slots / 65 up or down.  On 256 CUs: grid.y ≤ 8, 137 tiles, nt = 140 000.
    Synthetic surface, as the workload."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    gy = -(-2 * cus // 65)
    nt = 1024 * (16 * gy + 9) - 288
    if nt > 200_000 or gy < 2:
        pytest.skip(f"{cus} CUs: grid.y = {gy} would need nt = {nt} for a second cull round")
    src, tgt, nrm, _ = synth.icp_pair(33_000, nt, seed=7)
    _, corrs, _ = _check_loop(src, tgt, nrm)
    assert (corrs[-1] >= 0).mean() > 0.9
