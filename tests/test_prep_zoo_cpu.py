"""Census of tests/prep_zoo.py on the CPU oracle alone: the inputs of test_gpu_prep_edges.py
reach the kernel paths that file claims to cover.  No device is involved; a failure here means
the inputs (or feat.hip's launch constants) changed and the GPU cases need new shapes."""
from collections import Counter

import numpy as np
import pytest

import prep_oracle as P
import prep_zoo as Z


def test_zoo_reaches_the_eigen_solver_returns():
    """Measured: zero (all_same 70, duplicates 30), diag-x (plane_x 85), diag-y (plane_y 85),
    diag-z (axis_line 200, lattice_plane 85, sparse 45, stack 11, far_offset 3), neg-v0 and
    pos-cross on every cloud with a real plane.  pos-v2, pos-v1, neg-v1 and neg-cross are reached
    by no zoo cloud."""
    seen = Counter()
    for name in Z.zoo():
        seen.update(Z.oracle_normals(name)[1].tolist())
    assert set(seen) <= set(Z.EIGEN_PATHS)
    assert {"zero", "diag-x", "diag-y", "diag-z", "neg-v0", "pos-cross"} <= set(seen), seen
    assert Counter(Z.oracle_normals("all_same")[1].tolist()) == {"zero": 70}
    assert Counter(Z.oracle_normals("axis_line")[1].tolist()) == {"diag-z": 200}
    assert "zero" in Z.oracle_normals("duplicates")[1]


def test_eigen_path_names_each_return():
    assert Z.eigen_path(np.zeros((3, 3))) == "zero"
    assert Z.eigen_path(np.diag([1.0, 2.0, 3.0])) == "diag-x"
    assert Z.eigen_path(np.diag([2.0, 1.0, 3.0])) == "diag-y"
    assert Z.eigen_path(np.diag([2.0, 3.0, 1.0])) == "diag-z"
    assert Z.eigen_path(np.eye(3)) == "diag-z"  # fewer than 3 neighbours: identity covariance


def test_sparse_has_rows_of_one_two_and_three_neighbours():
    """Measured: 25 rows of count 1, 20 of count 2, 15 of count 3 (and 25 of count 1 at the FPFH
    radius, whose FPFH rows must be zero)."""
    cnt = Counter(Z.nbrs("sparse")[2].tolist())
    assert cnt == {1: 25, 2: 20, 3: 15}
    assert int((Z.nbrs("sparse", fpfh=True)[2] == 1).sum()) == 25


def test_pairs_are_rows_of_two_neighbours_in_oblique_directions():
    """Every row of ``pairs`` has count 2 (identity covariance → (0, 0, 1)), and no pair lies
    along an axis: its own rank-1 covariance would give another normal."""
    c = Z.zoo()["pairs"]
    assert np.all(Z.nbrs("pairs")[2] == 2)
    assert Counter(Z.oracle_normals("pairs")[1].tolist()) == {"diag-z": 60}
    d = c.points[30:] - c.points[:30]
    assert np.abs(d).min() > 1e-4


def test_clusters_are_full_of_near_tied_swap_tests():
    """Measured: 3360 pairs, 364 with ||a1| − |a2|| < 1e-14, 130 of them exact ties; glibc's acos
    and a correctly rounded one (200-bit mpmath) decide all 3360 swap tests alike."""
    pairs, near, ties = Z.swap_near_ties("clusters")
    assert pairs == 480 * 7
    assert near >= 300 and near - ties >= 100, (near, ties)
    # exact planes with given normals: every swap test is an exact tie
    pairs, near, ties = Z.swap_near_ties("lattice_plane")
    assert pairs == ties > 0


@pytest.mark.parametrize("name", ["lattice_plane", "plane_x", "plane_y", "tilted_plane", "axis_line", "all_same",
                                  "sparse", "far_offset", "stack", "pairs", "clusters"])
def test_every_row_is_stable(name):
    """The oracle's normal moves less than 1e-12 on every row when acos / cos move by an ulp.
    Measured: the largest move is 4.4e-14 (far_offset), 1.3e-15 on tilted_plane, at most 4.5e-16 on
    the others (pairs 0, clusters 1.6e-15)."""
    mask, spread = Z.stable(name)
    assert mask.all(), (int(mask.sum()), spread.max())


def test_duplicates_is_mostly_stable_and_line_is_not():
    """Measured: duplicates 450 of 500 rows stable (moves up to 5.2e-14; the unstable rows move by
    at least 5.0e-11), line 9 of 200 (stable up to 6.2e-14, unstable from 7.2e-10): the 1e-12
    threshold sits in a gap of three decades."""
    mask, spread = Z.stable("duplicates")
    assert mask.mean() >= 0.85, mask.mean()
    assert spread[mask].max() < 1e-13 and spread[~mask].min() > 1e-11
    mask, spread = Z.stable("line")
    assert (~mask).sum() >= 1
    assert spread[~mask].min() > 1e-11


@pytest.mark.parametrize("name", Z.FPFH_CLOUDS)
def test_fpfh_bin_edge_flags_are_rare(name):
    """At most 5 % of the rows have a pair feature within 1e-12 of a bin edge.  Measured: 20 of
    500 on duplicates, 0 on every other cloud (stack, clusters and the planes with given
    normals included)."""
    _, ref, flags, _ = Z.fpfh_case(name)
    assert flags.mean() <= 0.05, int(flags.sum())
    assert np.isfinite(ref).all()


def test_fpfh_clouds_reach_the_degenerate_pairs():
    """duplicates and all_same have pairs at distance 0 (f3 == 0, dist == 0), stack has
    neighbours straight along the normal (vn == 0), sparse rows of count 1, all_same a zero
    group sum (its oracle groups sum to 100: the SPFH alone)."""
    d2, cnt = Z.nbrs("duplicates", fpfh=True)[1:]
    assert sum(int((d2[i, 1:c] == 0.0).sum()) for i, c in enumerate(cnt)) >= 4 * 500 - 500
    d2, cnt = Z.nbrs("all_same", fpfh=True)[1:]
    assert np.all(d2 == 0.0) and np.all(cnt == Z.FPFH_MAX_NN)
    sums = Z.fpfh_case("all_same")[1].reshape(-1, 3, 11).sum(axis=2)
    assert np.all(np.abs(sums - 100.0) < 1e-9)
    c = Z.zoo()["stack"]
    idx, _, cnt = Z.nbrs("stack", fpfh=True)
    above = 0
    for i in range(len(c.points)):
        dp = c.points[idx[i, 1:cnt[i]]] - c.points[i]
        above += int(((dp[:, 0] == 0) & (dp[:, 1] == 0)).sum())
    assert above == 2 * 147  # each point's two column mates


def test_feature_split_of_the_tested_shapes():
    """feature_nn's launch arithmetic at the shapes of test_gpu_prep_edges.py.  The existing
    3000 × 3000 tests reach 47 slices of exactly one full tile; these reach the single slice, a
    slice of one reference, several tiles per slice, tiles of 1, 2, 3 and 63 references (the
    scalar remainder after the 4-wide loop) and query blocks with one live lane."""
    def facts(nq, nr):
        s = Z.feature_split(nq, nr)
        return s.slices, s.tiles_per_slice, s.last_slice, s.last_tile

    assert facts(3000, 3000) == (47, 1, 56, 56)
    assert facts(1, 1) == (1, 1, 1, 1)
    assert facts(5, 3) == (1, 1, 3, 3)
    assert facts(129, 63) == (1, 1, 63, 63)
    assert facts(130, 65) == (2, 1, 1, 1)
    assert facts(200, 131) == (3, 1, 3, 3)
    assert facts(8193, 4099) == (22, 3, 67, 3)
    assert facts(16385, 1027) == (9, 2, 3, 3)
    assert facts(3001, 9000) == (71, 2, 40, 40)
    # the other direction of the mutual filter
    assert facts(65, 130) == (3, 1, 2, 2)
    assert facts(4099, 8193) == (43, 3, 129, 1)
    assert facts(1027, 16385) == (129, 2, 1, 1)
    assert facts(9000, 3001) == (24, 2, 57, 57)
    for nq in (1, 129, 8193, 16385):
        assert Z.feature_split(nq, 64).last_block_lanes == 1


@pytest.mark.parametrize("ns,nt", Z.TIED_SHAPES)
def test_tied_features_tie_across_slices_and_tiles(ns, nt):
    """Queries whose tied minima lie in different slices / in different tiles of the first slice
    that holds one.  Measured (across slices, across tiles of one slice, of those in the first
    slice with a minimum):
    (130, 65) 5, 0, 0;  (200, 131) 138, 0, 0;  (3001, 9000) 2718, 130, 23;
    (8193, 4099) 7450, 1627, 459;  (16385, 1027) 14771, 5643, 1663.
    (130, 65) cannot reach 100: its second slice holds one reference, so only the ~130/16 queries
    that copy that reference's base row can tie across slices."""
    slices, tiles, tiles_first = Z.tie_census(ns, nt, Z.shape_seed(ns, nt))
    sp = Z.feature_split(ns, nt)
    assert sp.slices > 1
    assert slices >= (100 if ns >= 200 else 1), slices
    if sp.tiles_per_slice > 1:
        assert tiles >= 100, tiles
        assert tiles_first >= 20, tiles_first
    # tied rows are exact copies: the oracle's minimum is 0 wherever the base row stands
    fs, ft, qb, rb = Z.tied_features(ns, nt, Z.shape_seed(ns, nt))
    hit = np.isin(qb, rb)
    assert hit.mean() > 0.9
    first = {}
    for j in range(nt - 1, -1, -1):
        first[int(rb[j])] = j
    want = np.array([first.get(int(b), -1) for b in qb])
    np.testing.assert_array_equal(P.feature_nn(fs, ft)[hit], want[hit])


@pytest.mark.parametrize("radius,k", Z.HYBRID_BOUNDARIES)
def test_hybrid_boundary_cases_have_full_and_short_lists(radius, k):
    """Share of full lists by the oracle — radius 1.2: k = 63 / 64 / 65 → 34.0 / 29.9 / 27.0 %;
    radius 1.7: k = 127 / 128 → 23.7 / 22.0 %; radius 2.4: k = 255 / 256 → 14.1 / 13.2 %."""
    cnt = Z.hybrid_case(radius, k)[2]
    assert 0.05 <= (cnt == k).mean() <= 0.95, (cnt == k).mean()
