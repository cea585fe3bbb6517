"""Brute-force NN with nn_mfma_kernel's per-lane hit record: a sweep step
pushes its sign bit into the lane's 32-bit shift register of its query group, and the wave builds
its (group, sub-tile) mask once per 1024-target tile.  The shapes are chosen by (query block of
512) × (target tile of 1024) counts: a single lane and a single sub-tile, ragged last blocks and
tiles, several tiles per block, hits in the first and the last sub-tile of a tile.  Every result
is compared bit for bit with the oracle's exact fp64 NN (icp_oracle.nn_exact) and with the grid
search.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_oracle as I
from m3d import synth
from m3d.core import Cloud, IcpLoop, nn1

pytestmark = pytest.mark.gpu


def _nn(src, tgt, T, r, nn="brute"):
    idx, d2 = nn1(Cloud(src), Cloud(tgt), T, r, nn=nn)
    return idx.cpu().numpy(), d2.cpu().numpy()


def _check(src, tgt, T, r):
    idx, d2 = _nn(src, tgt, T, r)
    ref_j, ref_d2 = I.nn_exact(cKDTree(tgt), tgt, I.transform_points(T, src), r)
    np.testing.assert_array_equal(idx, ref_j)
    np.testing.assert_array_equal(d2, ref_d2)
    ig, dg = _nn(src, tgt, T, r, nn="grid")
    np.testing.assert_array_equal(ig, idx)
    np.testing.assert_array_equal(dg, d2)
    return idx


@pytest.mark.parametrize("ns,nt", [
    (1, 1),            # one query lane, one real target: 63 idle lanes, 31 pad sub-tiles
    (513, 1025),       # 2 × 2 units, the second of each nearly empty
    (1100, 5000),      # 3 × 5 units
    (11769, 23557),    # 23 × 24 units
    (2660, 204797),    # 6 × 200 units: many tiles per block, ragged last query block
])
def test_unseeded_scan_matches_oracle(ns, nt):
    """The radii of test_gpu_icp.test_nn1_matches_kdtree: 0.3 below 5000 targets, else 0.12."""
    tgt, _ = synth.surface_points(nt, seed=1)
    src, _ = synth.surface_points(ns, seed=2)
    T = synth.random_rigid(3, rot_range=0.02, trans_range=0.05)
    _check(src, tgt, T, 0.3 if nt < 5000 else 0.12)


def test_hits_in_every_sub_tile_position():
    """Queries that are the targets themselves: each target's sub-tile (all 32 positions of every
    tile, the first and the last included) must be flagged for its own query, whatever the order
    of the record's bits."""
    tgt, _ = synth.surface_points(4096, seed=5)
    idx = _check(tgt.copy(), tgt, np.eye(4), 0.05)
    np.testing.assert_array_equal(idx, np.arange(len(tgt)))


def test_radius_beyond_fp16_range_takes_the_exact_path():
    """A radius far larger than the cloud: the threshold leaves the fp16 range and the group's
    mask is forced, with no hit recorded."""
    tgt, _ = synth.surface_points(3000, seed=3)
    _check(tgt[::7] * 1.001, tgt, np.eye(4), 50.0)


def test_duplicates_lowest_index_wins_across_tiles():
    """40 exact copies of 150 points (6 target tiles): every query's nearest distance is a 40-way
    tie whose candidates straddle sub-tile and tile boundaries."""
    rng = np.random.default_rng(21)
    dup = np.repeat(rng.normal(size=(150, 3)), 40, axis=0)
    _check(dup[::5][:1100] + 1e-3, dup, np.eye(4), 0.5)


def test_loop_of_three_evaluations_matches_grid_loop():
    """The first evaluation is unseeded (flagged sub-tiles resolved inside the tile, threshold
    refresh), the next two self-seed (flagged sub-tiles deferred to the per-wave list)."""
    src, tgt, nrm, _ = synth.icp_pair(1100, 5000, seed=19)
    out = {}
    for nn in ("brute", "grid"):
        lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), 0.12, relative_fitness=-1, relative_rmse=-1,
                     max_iteration=3, nn=nn)
        lp.reset(np.eye(4))
        for _ in range(3):
            lp.step()
        out[nn] = (lp.result().transformation, lp.correspondences().cpu().numpy())
    np.testing.assert_array_equal(out["brute"][1], out["grid"][1])
    np.testing.assert_array_equal(out["brute"][0], out["grid"][0])
    assert (out["brute"][1] >= 0).sum() > 500  # a real registration, not two empty results
