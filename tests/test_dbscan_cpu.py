"""The DBSCAN restatement (tests/dbscan_restatement.py) checked on the CPU: the closed form the device
computes equals a literal port of Open3D's loop whatever the pop order, the case table's counts
hold, sklearn agrees wherever no pair sits at the radius and disagrees on the exact-tie lattice
(its test is ``<=``), and ``prep.cluster_dbscan`` rejects bad arguments without a device."""
import numpy as np
import pytest

import dbscan_restatement as D
from m3d import prep

TIE_MARGIN = 1e-9  # relative distance of every d² from eps² that makes `<` and `<=` the same test


@pytest.mark.parametrize("name", list(D.CASES))
def test_literal_equals_closed_form_and_table(name):
    r = D.case(name)
    _, _, mp, clusters, noise, border, multi = D.CASES[name]
    assert (r.num_clusters, int((r.labels < 0).sum()), int(r.border.sum()), int(r.multi.sum())) == \
        (clusters, noise, border, multi)
    np.testing.assert_array_equal(D.literal(r.nbs, mp), r.labels)
    for seed in (1, 2):
        np.testing.assert_array_equal(D.literal(r.nbs, mp, np.random.default_rng(seed)), r.labels)
    assert all(i in r.nbs[i] for i in range(0, len(r.nbs), 97))  # the point itself is a neighbour
    assert r.sizes.sum() + (r.labels < 0).sum() == len(r.labels)


def _sklearn_labels(r):
    cluster = pytest.importorskip("sklearn.cluster")
    return cluster.DBSCAN(eps=r.eps, min_samples=r.min_points, algorithm="brute").fit(r.points).labels_


@pytest.mark.parametrize("name", [n for n in D.CASES if n != D.TIE_CASE])
def test_sklearn_agrees_away_from_ties(name):
    r = D.case(name)
    sk = _sklearn_labels(r)
    assert D.tie_margin(r.points, r.eps) >= TIE_MARGIN
    # sklearn grows its clusters one after the other in index order of their first core point, so a
    # border point goes to the lowest-numbered cluster that touches it, as here
    np.testing.assert_array_equal(sk, r.labels)


def test_sklearn_differs_on_exact_ties():
    r = D.case(D.TIE_CASE)
    assert D.tie_margin(r.points, r.eps) == 0.0
    sk = _sklearn_labels(r)
    assert not np.array_equal(sk, r.labels)
    assert sk.max() == 0 and r.labels.max() == 511  # `<=` joins the lattice, `<` leaves 512 singletons


def test_chain_and_bridge_premises():
    P, eps = D.chain()
    r = D.solve(P, eps, 2)
    assert r.num_clusters == 1 and (r.labels == 0).all()
    P, eps, mp, ix, iy = D.bridge()
    r = D.solve(P, eps, mp)
    assert not r.core[0] and r.core[1:].all()
    assert list(r.nbs[0]) == [0, iy, ix] and iy < ix
    assert r.num_clusters == 2 and r.labels[ix] == 0 and r.labels[iy] == 1 and r.labels[0] == 0
    np.testing.assert_array_equal(D.literal(r.nbs, mp), r.labels)


@pytest.mark.parametrize("eps, min_points", [(0.0, 3), (-1.0, 3), (float("nan"), 3), (float("inf"), 3), (0.1, 0),
                                             (0.1, -2)])
def test_argument_errors_without_device(eps, min_points):
    with pytest.raises(ValueError):
        prep.cluster_dbscan(np.zeros((4, 3)), eps, min_points)


def test_empty_cloud_without_device():
    labels = prep.cluster_dbscan(np.zeros((0, 3)), 0.1, 3)
    assert labels.shape == (0,) and labels.dtype == np.int32
    labels, out = prep.cluster_dbscan(np.zeros((0, 3)), 0.1, 3, with_details=True)
    assert labels.shape == (0,) and out.num_clusters == 0 and out.largest_label == -1 and out.largest_size == 0
    assert out.sizes.shape == (0,) and out.counts.shape == (0,)
