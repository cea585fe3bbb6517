"""GPU parity of DBSCAN (m3d_cluster_dbscan through m3d.prep, PointCloud and Ply) against the CPU
restatement in tests/dbscan_restatement.py.

Everything is compared for equality: both sides decide a neighbour by the same fp64 expression
(dx·dx + dy·dy) + dz·dz < eps·eps without contraction, and the labels are a function of those
decisions alone (components of the core graph ranked by smallest member, a border point's
smallest neighbouring label).
"""
import numpy as np
import pytest

import clean_restatement as C
import dbscan_restatement as D
import prep_zoo
from m3d import plyio, prep
from m3d.core import Cloud
from m3d.types import PointCloud

# the shared inputs are read-only arrays; torch only notes that it will not write to them either
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The given NumPy array is not writable")]


def assert_outcome(got, ref, counts=None):
    """(labels, DbscanOutcome) of the device against a dbscan_restatement.solve namespace."""
    labels, out = got
    assert labels.dtype == np.int32 and labels.shape == ref.labels.shape
    np.testing.assert_array_equal(labels, ref.labels)
    n_noise = int((ref.labels < 0).sum())
    assert (out.num_clusters, out.num_core, out.num_noise) == (ref.num_clusters, int(ref.core.sum()), n_noise)
    np.testing.assert_array_equal(out.sizes, np.bincount(ref.labels[ref.labels >= 0], minlength=ref.num_clusters))
    if ref.num_clusters:
        assert out.largest_label == int(np.argmax(ref.sizes)) and out.largest_size == int(ref.sizes.max())
    else:
        assert out.largest_label == -1 and out.largest_size == 0
    np.testing.assert_array_equal(out.counts, ref.counts if counts is None else counts)


def same(a, b):
    (la, oa), (lb, ob) = a, b
    return (la.tobytes() == lb.tobytes() and oa.sizes.tobytes() == ob.sizes.tobytes()
            and oa.counts.tobytes() == ob.counts.tobytes()
            and (oa.num_clusters, oa.num_core, oa.num_noise, oa.largest_label, oa.largest_size)
            == (ob.num_clusters, ob.num_core, ob.num_noise, ob.largest_label, ob.largest_size))


def run(P, eps, mp):
    return prep.cluster_dbscan(P, eps, mp, with_details=True)


@pytest.mark.parametrize("name", list(D.CASES))
def test_table_case(name):
    ref = D.case(name)
    cloud = Cloud(ref.points)
    first = run(cloud, ref.eps, ref.min_points)
    assert_outcome(first, ref, C.radius_counts(ref.points, ref.eps))
    assert same(run(cloud, ref.eps, ref.min_points), first)
    prep.remove_radius_outlier(cloud, 3, ref.eps)  # the same cell size: the cloud's cached grid
    assert same(run(cloud, ref.eps, ref.min_points), first)
    np.testing.assert_array_equal(prep.cluster_dbscan(ref.points, ref.eps, ref.min_points), ref.labels)


def test_long_chain_shuffled():
    P, eps = D.chain()
    labels, out = run(P, eps, 2)
    assert out.num_clusters == 1 and out.num_noise == 0 and (labels == 0).all()
    assert out.largest_label == 0 and out.largest_size == len(P) and out.num_core == len(P)
    assert_outcome(run(P, eps, 4), D.solve(P, eps, 4))
    assert_outcome(run(P, eps, 3), D.solve(P, eps, 3))


def test_non_core_bridge():
    P, eps, mp, ix, iy = D.bridge()
    ref = D.solve(P, eps, mp)
    # the construction: the bridge is the only non-core point and touches one core point of each
    # blob; the blob that is cluster 0 (through index 1) touches it with its LAST index
    assert not ref.core[0] and ref.core[1:].all()
    assert list(ref.nbs[0]) == [0, iy, ix] and iy < ix
    assert ref.num_clusters == 2 and ref.labels[1] == 0 and ref.labels[ix] == 0 and ref.labels[iy] == 1
    assert ref.labels[0] == 0
    got = run(P, eps, mp)
    assert_outcome(got, ref)
    assert got[0][0] == 0


def test_numbering_follows_the_indices():
    ref = D.case("A_008_6")
    perm = np.random.default_rng(3).permutation(len(ref.points))
    Q = np.ascontiguousarray(ref.points[perm])
    ref_q = D.solve(Q, ref.eps, ref.min_points)
    got = run(Q, ref.eps, ref.min_points)
    assert_outcome(got, ref_q)
    assert not np.array_equal(got[0], ref.labels[perm])  # the numbers move with the indices


def test_exact_tie_lattice():
    P = C.points("L7_1")
    labels, out = run(P, 0.25, 1)
    np.testing.assert_array_equal(labels, np.arange(512))  # d² == eps² is outside: 512 singletons
    assert out.num_clusters == 512 and out.num_core == 512 and out.num_noise == 0
    assert (out.sizes == 1).all() and out.largest_label == 0 and out.largest_size == 1
    assert (out.counts == 1).all()
    labels, out = run(P, 0.25 * (1.0 + 2.0 ** -52), 1)  # one ulp beyond: the lattice connects
    assert (labels == 0).all() and out.num_clusters == 1 and out.largest_size == 512


@pytest.mark.parametrize("name", ["one_mp1", "one_mp2", "two_coincident", "n65", "cell200"])
def test_small_shapes(name):
    rng = np.random.default_rng(21)
    if name.startswith("one"):
        P, eps, mp = np.array([[4.0, -2.0, 9.0]]), 0.1, int(name[-1])
    elif name == "two_coincident":
        P, eps, mp = np.tile([[1.25, 2.5, -3.75]], (2, 1)), 0.1, 2
    elif name == "n65":  # one wave of candidates plus one, all within eps of each other
        P, eps, mp = np.array([7.0, 7.0, 7.0]) + rng.uniform(-0.01, 0.01, (65, 3)), 0.1, 65
    else:  # a cell holding 200 coincident points beside a few others
        P = np.concatenate([np.tile([[0.5, 0.5, 0.5]], (200, 1)), rng.uniform(0.0, 1.0, (40, 3))])
        P, eps, mp = P[rng.permutation(len(P))], 0.1, 5
    P = np.ascontiguousarray(P)
    ref = D.solve(P, eps, mp)
    if name == "one_mp1":
        assert ref.labels.tolist() == [0]
    if name == "one_mp2":
        assert ref.labels.tolist() == [-1]
    if name == "n65":
        assert (ref.labels == 0).all()
    got = run(P, eps, mp)
    assert_outcome(got, ref)
    assert same(run(P, eps, mp), got)


@pytest.mark.parametrize("name", ["far_offset", "duplicates", "stack", "clusters", "all_same", "sparse", "line"])
def test_zoo(name):
    c = prep_zoo.zoo()[name]
    ref = D.solve(c.points, c.radius, 5)
    assert_outcome(run(c.points, c.radius, 5), ref)


# ------------------------------------------------------------------------------- API
def test_pointcloud_cluster_dbscan():
    ref = D.case("C_01_5")
    pc = PointCloud(ref.points)
    labels = pc.cluster_dbscan(ref.eps, ref.min_points, print_progress=True)
    assert labels.dtype == np.int32
    np.testing.assert_array_equal(labels, ref.labels)
    np.testing.assert_array_equal(pc.cluster_dbscan(eps=ref.eps, min_points=ref.min_points), ref.labels)


def _scan(seed=4):
    """A table patch, a dense object above it, a smaller clump beside it and sparse clutter."""
    rng = np.random.default_rng(seed)
    table = np.column_stack([rng.uniform(-1, 1, 2500), rng.uniform(-1, 1, 2500), rng.normal(0.0, 0.002, 2500)])
    obj = np.column_stack([rng.uniform(-0.3, 0.3, 1500), rng.uniform(-0.2, 0.2, 1500), rng.uniform(0.05, 0.35, 1500)])
    clump = np.array([0.7, 0.7, 0.15]) + rng.uniform(-0.06, 0.06, (150, 3))
    clutter = rng.uniform(-1.5, 1.5, (80, 3)) + np.array([0.0, 0.0, 2.0])
    P = np.vstack([table, obj, clump, clutter])
    return np.ascontiguousarray(P[rng.permutation(len(P))])


def test_ply_keep_cluster(tmp_path):
    from ply.ply import Ply

    P = _scan()
    path = tmp_path / "scan.ply"
    plyio.write_ply(path, P, binary=True)
    plane = {"distance_threshold": 0.012, "num_iterations": 200, "seed": 7}
    keep = {"eps": 0.06, "min_points": 8}
    np.random.seed(0)
    a = Ply(path, 0.05, remove_plane=plane)
    assert "keep_cluster" not in a.stage_ms
    np.random.seed(0)
    b = Ply(path, 0.05, remove_plane=plane, keep_cluster=keep)
    assert "keep_cluster" in b.stage_ms
    # host-side recomputation on the points the plane removal left (a.pcd holds exactly those)
    rest = np.ascontiguousarray(a.pcd.points)
    ref = D.solve(rest, keep["eps"], keep["min_points"])
    assert ref.num_clusters >= 2 and ref.sizes.max() > 1000
    big = int(np.argmax(ref.sizes))
    assert (b.cluster_label, b.cluster_size, b.num_clusters) == (big, int(ref.sizes[big]), ref.num_clusters)
    members = rest[ref.labels == big]
    assert b.pcd.points.tobytes() == members.tobytes()
    assert len(b.pcd.normals) == len(members)
    # … and they are what reached the down-sample
    down, _ = prep.voxel_down_sample(members, 0.05)
    assert len(b.pcd_down.points) == len(down)
    c = Ply.from_arrays(rest, preprocess=True, voxel_size=0.05, keep_cluster=keep)
    assert c.pcd.points.tobytes() == members.tobytes()


def test_ply_keep_cluster_without_cluster_raises():
    from ply.ply import Ply

    P = np.column_stack([10.0 * np.arange(50), np.zeros(50), np.zeros(50)])
    with pytest.raises(ValueError, match="no cluster"):
        Ply.from_arrays(P, preprocess=True, voxel_size=0.5, keep_cluster={"eps": 0.5, "min_points": 3})
    with pytest.raises(ValueError, match="keep_cluster"):
        Ply.from_arrays(P, preprocess=True, voxel_size=0.5, keep_cluster={"eps": 0.5})
