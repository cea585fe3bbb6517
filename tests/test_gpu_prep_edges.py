"""The preprocessing and feature-matching kernels (prep.hip, feat.hip) on the edge-case inputs of
tests/prep_zoo.py, against the CPU oracle (oracle/prep_oracle.py).  test_prep_zoo_cpu.py asserts
on the oracle alone that these inputs reach the paths named here.

Bars:
* feature correspondences, hybrid lists: bit-equal (test_gpu_prep.py's own bar);
* normals: within 1e-9 of the oracle on the rows whose oracle normal is stable under a one-ulp
  change of acos / cos (the oracle's own spread there is 4.4e-14); bit-equal where the solver
  calls no libm (returns ``zero`` / ``diag-*``, fewer than 3 neighbours); unit length and finite
  everywhere;
* FPFH: bit-equal on every row without a pair feature within 1e-12 of a bin edge; every row
  finite, every 11-bin group sums to 200, 100 or 0; rows of one neighbour are zero.
"""
import numpy as np
import pytest

import prep_oracle as P
import prep_zoo as Z
from m3d import prep

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- feature 1-NN
@pytest.mark.parametrize("mutual", [False, True], ids=["oneway", "mutual"])
@pytest.mark.parametrize("ns,nt,tied", [(ns, nt, False) for ns, nt in Z.FEATURE_SHAPES] +
                         [(ns, nt, True) for ns, nt in Z.TIED_SHAPES])
def test_feature_correspondences_shapes(ns, nt, tied, mutual):
    """Single slice, a slice of one reference, several tiles per slice, tiles of 1, 2, 3 and 63
    references (the scalar remainder loop), query blocks with one live lane, ns ≠ nt; with
    ``tied`` every minimum is 0 at about four references in different tiles and slices, and the
    lowest index must win.  The mutual filter runs the search both ways (the transposed shape);
    (16385, 1027) has fewer mutual pairs than 0.1·ns and falls back to the one-directional set."""
    fs, ft, one_way, both = Z.feature_case(ns, nt, tied)
    got = prep.feature_correspondences(fs, ft, mutual)
    np.testing.assert_array_equal(got, both if mutual else one_way)


@pytest.mark.parametrize("ns,nt,tied", [(200, 131, False), (130, 65, True)])
def test_mutual_fallback_threshold(ns, nt, tied):
    """m mutual pairs are kept iff m ≥ int(ratio·ns): ratios 0, m/ns, (m+1)/ns and 1 stand on
    both sides of the threshold, by the oracle, and the device follows it on each."""
    fs, ft, _, both = Z.feature_case(ns, nt, tied)
    m = len(both)
    assert 0 < m < ns
    lengths = []
    for ratio in (0.0, m / ns, (m + 1) / ns, 1.0):
        ref = P.correspondences_from_features(fs, ft, True, ratio)
        lengths.append(len(ref))
        got = prep.feature_correspondences(fs, ft, True, ratio)
        np.testing.assert_array_equal(got, ref)
    assert lengths[0] == m and lengths[1] == m  # kept
    assert lengths[2] == ns and lengths[3] == ns  # fell back


@pytest.mark.parametrize("ns,nt", [(0, 0), (0, 7), (7, 0)])
@pytest.mark.parametrize("mutual", [False, True])
def test_feature_correspondences_empty(ns, nt, mutual):
    got = prep.feature_correspondences(np.zeros((ns, 33)), np.zeros((nt, 33)), mutual)
    assert got.shape == (0, 2) and got.dtype == np.int32


# ------------------------------------------------------------------------------- hybrid search
@pytest.mark.parametrize("radius,k", Z.HYBRID_BOUNDARIES + Z.HYBRID_SMALL_K)
def test_hybrid_search_template_boundaries(radius, k):
    """k on both sides of the list templates (1 / 2 / 4 slots per lane at k ≤ 64 / ≤ 128 / ≤ 256)
    and k = 1, 2; 13 to 34 % of the lists full at the boundaries, the rest short and padded."""
    gi, gd, gc = prep.hybrid_search(Z.hybrid_points(), radius, k)
    ri, rd, rc = Z.hybrid_case(radius, k)
    np.testing.assert_array_equal(gc, rc)
    np.testing.assert_array_equal(gi, ri)
    np.testing.assert_array_equal(gd, rd)


# ------------------------------------------------------------------------------- normals
@pytest.mark.parametrize("name", list(Z.zoo()))
def test_normals_on_the_zoo(name):
    """Exact planes (axis-aligned: the diagonal returns; tilted; 3-point neighbourhoods), lines,
    coinciding points (zero covariance → (0, 0, 1)), rows of 1 and 2 neighbours (``pairs``: two
    points in an oblique direction must still give the identity covariance's (0, 0, 1)), and a
    cloud 2·10⁴ from the origin (cum/c − mean² cancels 9 digits).
    Measured on the device, stable rows against the oracle (bar 1e-9): the largest difference is
    8.9e-16 (far_offset; tilted_plane 7.8e-16, clusters 5.0e-16, duplicates 2.2e-16, stack
    4.9e-32, 0 on the others); the unstable rows of duplicates and line agreed as well on that
    run."""
    c = Z.zoo()[name]
    ref, paths = Z.oracle_normals(name)
    mask, _ = Z.stable(name)
    cnt = Z.nbrs(name)[2]
    got = prep.estimate_normals(c.points, c.radius, c.max_nn)
    diff = np.abs(got - ref).max(axis=1)
    exact = np.isin(paths, Z.LIBM_FREE_PATHS) | (cnt < 3)
    print(f"{name}: stable {int(mask.sum())}/{len(mask)}, max diff on stable rows "
          f"{diff[mask].max() if mask.any() else 0.0:.3g}, on all rows {diff.max():.3g}, "
          f"libm-free rows {int(exact.sum())}")
    assert np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-12
    np.testing.assert_array_equal(got[exact], ref[exact])
    np.testing.assert_allclose(got[mask], ref[mask], rtol=0, atol=1e-9)


def test_normals_on_a_line_are_perpendicular_to_it():
    """A line has no plane: two eigenvalues vanish and the normal is any unit vector across the
    line, decided by rounding (9 of 200 rows are stable).  Held to the property alone: |n·d| at
    most 8 × the oracle's own maximum on this cloud (4.2e-14; the factor is room for a tail,
    both sides run the same arithmetic).
    Measured on the device: 4.24e-14, the oracle's own figure (bar 3.4e-13)."""
    c = Z.zoo()["line"]
    d = Z.line_direction()
    ref = np.abs(Z.oracle_normals("line")[0] @ d).max()
    got = prep.estimate_normals(c.points, c.radius, c.max_nn)
    dev = np.abs(got @ d).max()
    print(f"line: max |n.d| device {dev:.3g}, oracle {ref:.3g}")
    assert np.isfinite(got).all()
    assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 1e-12
    assert dev <= 8 * ref


def test_given_normals_orient_degenerate_rows():
    """A zero covariance falls back to the given normal, unchanged; a given (0, 0, −1) flips an
    exact plane's normals, diagonal-return rows included, and changes no magnitude."""
    c = Z.zoo()["all_same"]
    rng = np.random.default_rng(7)
    given = rng.normal(size=c.points.shape)
    given /= np.linalg.norm(given, axis=1)[:, None]
    np.testing.assert_array_equal(prep.estimate_normals(c.points, c.radius, c.max_nn, normals=given), given)

    c = Z.zoo()["lattice_plane"]
    plain = prep.estimate_normals(c.points, c.radius, c.max_nn)
    down = np.tile([0.0, 0.0, -1.0], (len(c.points), 1))
    got = prep.estimate_normals(c.points, c.radius, c.max_nn, normals=down)
    np.testing.assert_array_equal(np.abs(got), np.abs(plain))
    assert np.all(got[:, 2] < 0)
    flipped = plain[:, 2] > 0
    assert flipped.any()
    np.testing.assert_array_equal(got[flipped], -plain[flipped])
    np.testing.assert_array_equal(got[~flipped], plain[~flipped])
    ref = P.estimate_normals(c.points, c.radius, c.max_nn, prev_normals=down, nbrs=Z.nbrs("lattice_plane"))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)

    c = Z.zoo()["stack"]  # its zoo normals are given: (0, 0, 1)
    got = prep.estimate_normals(c.points, c.radius, c.max_nn, normals=c.normals)
    ref = P.estimate_normals(c.points, c.radius, c.max_nn, prev_normals=c.normals, nbrs=Z.nbrs("stack"))
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9)
    assert np.all(got @ np.array([0.0, 0.0, 1.0]) >= 0)


# ------------------------------------------------------------------------------- FPFH
def _group_sums_ok(f):
    sums = f.reshape(-1, 3, 11).sum(axis=2)
    return (np.abs(sums - 200.0) <= 1e-9) | (np.abs(sums - 100.0) <= 1e-9) | (sums == 0.0)


@pytest.mark.parametrize("name", Z.FPFH_CLOUDS)
def test_fpfh_on_the_zoo(name):
    """Pairs at distance 0 (duplicates, all_same: f3 == 0 in the SPFH, dist == 0 skipped in the
    weighting, a zero group sum on all_same), neighbours straight along the normal (stack:
    vn == 0), rows of one neighbour (sparse: all-zero rows), exact planes with given normals
    (every swap test an exact tie), the far offset, and ``clusters``, where the normals of a
    pair differ by ulps and 234 swap tests are near ties (decided as correctly rounded acos
    values would be)."""
    c = Z.zoo()[name]
    nrm, ref, flags, cnt = Z.fpfh_case(name)
    got = prep.compute_fpfh(c.points, nrm, 2 * c.radius, Z.FPFH_MAX_NN)
    rows_off = np.flatnonzero(np.any(got != ref, axis=1))
    print(f"{name}: {len(rows_off)} rows differ from the oracle ({int(flags.sum())} flagged), "
          f"max |diff| {np.abs(got - ref).max():.3g}")
    assert np.isfinite(got).all()
    assert _group_sums_ok(got).all()
    assert np.all(got[cnt <= 1] == 0.0)
    np.testing.assert_array_equal(got[~flags], ref[~flags])


def test_fpfh_of_single_neighbour_lists_is_zero():
    """max_nn = 1: every list holds the point alone, every row is zero."""
    c = Z.zoo()["far_offset"]
    got = prep.compute_fpfh(c.points, Z.oracle_normals("far_offset")[0], 2 * c.radius, 1)
    assert got.shape == (len(c.points), 33)
    assert np.all(got == 0.0)
