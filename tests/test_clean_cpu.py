"""Outlier removal without a GPU: the CPU restatement the GPU tests compare against
(tests/clean_restatement.py) is itself checked against scipy's k-d tree and numpy's statistics and
against the removal counts its seeded inputs were chosen for; the argument rules decided before any
device work; PointCloud.select_by_index; the C ABI's three new symbols."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
from scipy.spatial import cKDTree

import clean_restatement as R
from m3d import _lib, prep
from m3d.types import PointCloud

ROOT = Path(__file__).resolve().parents[1]

# every listed case keeps this relative distance between the threshold and the nearest mean
# distance, so the device's differently ordered sums cannot move a point across it
MARGIN = 6e-3


@pytest.mark.parametrize("name", ["A", "D"])
def test_restatement_lists_agree_with_the_kd_tree(name):
    P, k = R.points(name), R.CASES[name][1]
    idx, d2, cnt = R.knn_case(name, k)
    dist, ind = cKDTree(P).query(P, k=k)
    assert (cnt == k).all()
    np.testing.assert_allclose(np.sqrt(d2), dist, rtol=1e-12, atol=0.0)
    assert (np.diff(d2, axis=1) >= 0).all() and (d2[:, 0] == 0).all()
    # random data: no ties beyond the self match, so the index lists agree too
    np.testing.assert_array_equal(idx, ind)


@pytest.mark.parametrize("name", ["A", "B", "D", "E", "M", "L7_1"])
def test_restatement_statistics_agree_with_numpy(name):
    avg, st = R.stat_case(name)
    assert avg.min() > 0
    ratio = R.CASES[name][2]
    np.testing.assert_allclose(st.mean, np.mean(avg), rtol=1e-12)
    np.testing.assert_allclose(st.std_dev, np.std(avg, ddof=1), rtol=1e-12)
    np.testing.assert_allclose(st.threshold, np.mean(avg) + ratio * np.std(avg, ddof=1), rtol=1e-12)
    assert st.valid == len(avg)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_removed_counts_and_margins(name):
    avg, st = R.stat_case(name)
    assert len(avg) - len(st.indices) == R.CASES[name][3]
    assert st.margin >= MARGIN
    assert (np.diff(st.indices) > 0).all()


def test_far_pair_is_what_case_e_removes():
    P = R.points("E")
    _, st = R.stat_case("E")
    gone = np.setdiff1d(np.arange(len(P)), st.indices)
    assert sorted(np.abs(P[gone]).max(1).tolist()) == [1e3, 2e3]


def test_fewer_points_than_neighbours():
    idx, d2, cnt = R.knn_case("F", 20)
    assert (cnt == 12).all() and (idx[:, 12:] == -1).all() and np.isinf(d2[:, 12:]).all()
    assert (np.sort(idx[:, :12], axis=1) == np.arange(12)).all()


def test_coincident_twins_are_all_dropped():
    idx, d2, _ = R.knn_case("G", 2)
    avg, st = R.stat_case("G")
    assert not d2.any() and not avg.any()
    # the first entry is the lower index of the twin pair, not necessarily the point itself
    assert (idx[:, 0] < idx[:, 1]).all() and (idx[:, 0] != np.arange(600)).any()
    assert st.threshold == 0.0 and st.mean == 0.0 and len(st.indices) == 0


def test_one_neighbour_drops_everything():
    P = R.points("D")
    _, d2, cnt = R.knn(P[:50], 1)
    st = R.statistics(R.mean_distance(d2, cnt), 2.0)
    assert len(st.indices) == 0 and st.threshold == 0.0


def test_single_point_and_empty_cloud():
    _, d2, cnt = R.knn(np.array([[1.0, 2.0, 3.0]]), 5)
    st = R.statistics(R.mean_distance(d2, cnt), 2.0)
    assert st.valid == 1 and np.isnan(st.threshold) and np.isnan(st.std_dev) and len(st.indices) == 0
    st = R.statistics(np.zeros(0), 2.0)
    assert st.valid == 0 and len(st.indices) == 0


def test_lattice_radius_counts_are_strict():
    L = R.points("L7_1")
    assert (R.radius_counts(L, 0.25) == 1).all()  # d² == r² is outside
    v, c = np.unique(R.radius_counts(L, 0.25 * (1 + 2.0 ** -40)), return_counts=True)
    assert dict(zip(v.tolist(), c.tolist())) == {4: 8, 5: 72, 6: 216, 7: 216}


@pytest.mark.parametrize("kw", [dict(nb_neighbors=0, std_ratio=2.0), dict(nb_neighbors=20, std_ratio=0.0),
                                dict(nb_neighbors=-3, std_ratio=1.0), dict(nb_neighbors=20, std_ratio=-1.0)])
def test_statistical_filter_rejects_illegal_parameters_without_a_device(kw):
    with pytest.raises(ValueError, match="Illegal input parameters"):
        prep.remove_statistical_outlier(R.points("F"), **kw)


@pytest.mark.parametrize("kw", [dict(nb_points=0, radius=0.1), dict(nb_points=5, radius=0.0),
                                dict(nb_points=5, radius=-1.0)])
def test_radius_filter_rejects_illegal_parameters_without_a_device(kw):
    with pytest.raises(ValueError, match="Illegal input parameters"):
        prep.remove_radius_outlier(R.points("F"), **kw)


@pytest.mark.parametrize("k", [0, 257])
def test_knn_search_rejects_k_outside_1_256_without_a_device(k):
    with pytest.raises(ValueError, match="1 <= k <= 256"):
        prep.knn_search(R.points("F"), k)


def test_empty_cloud_is_an_empty_result_without_a_device():
    ind, st = prep.remove_statistical_outlier(np.zeros((0, 3)), 20, 2.0)
    assert ind.shape == (0,) and ind.dtype == np.int32 and (st.kept, st.valid) == (0, 0)
    ind = prep.remove_radius_outlier(np.zeros((0, 3)), 5, 0.1)
    assert ind.shape == (0,) and ind.dtype == np.int32


def test_select_by_index():
    rng = np.random.default_rng(0)
    pts, nrm = rng.normal(size=(10, 3)), rng.normal(size=(10, 3))
    pc = PointCloud(pts, nrm)
    sel = pc.select_by_index([7, 2, 5])
    np.testing.assert_array_equal(sel.points, pts[[2, 5, 7]])  # index order, as Open3D
    np.testing.assert_array_equal(sel.normals, nrm[[2, 5, 7]])
    inv = pc.select_by_index(np.array([7, 2, 5], np.int32), invert=True)
    rest = [0, 1, 3, 4, 6, 8, 9]
    np.testing.assert_array_equal(inv.points, pts[rest])
    np.testing.assert_array_equal(inv.normals, nrm[rest])
    bare = PointCloud(pts).select_by_index([1])
    assert bare.points.shape == (1, 3) and not bare.has_normals()
    assert len(pc.select_by_index([]).points) == 0 and len(pc.points) == 10


def test_the_three_entry_points_are_in_the_header_the_table_and_the_library():
    text = (ROOT / "include" / "m3d.h").read_text()
    syms = set(re.findall(r"\b(m3d_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name, nargs in (("m3d_knn_search", 7), ("m3d_remove_statistical_outlier", 9),
                        ("m3d_remove_radius_outlier", 8)):
        assert name in syms and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs
    assert lib.m3d_abi_version() == _lib.ABI_VERSION == 13
    assert C.sizeof(_lib.OutlierStats) == 40
    assert [f[0] for f in _lib.OutlierStats._fields_] == ["kept", "valid", "mean", "std_dev", "threshold"]
