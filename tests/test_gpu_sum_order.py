"""The order of summation of the registration evaluation and of the Generalized-ICP terms pass,
asserted bit for bit against a numpy emulation of it (icp.hip, "reduce": the order every consumer
of a loop's NN scan shares).

The emulation takes the per-slot values in the loop's Morton slot order
(``IcpLoop.source_slots()`` on the same Cloud objects and radius: the Morton copy is cached per
cloud and cell size) and adds them as the device does:
  * padded to a multiple of 256 with +0.0: a block holds 256 consecutive slots;
  * per 64-lane wave six rounds of v = v + v[lane ^ o], o = 32, 16, 8, 4, 2, 1 (every lane ends
    with the same sum);
  * per block t = 0.0, then t += wave[w] for w = 0..3;
  * group g = 0..31: v = 0.0, then v += partial[b] for b = g, g + 32, …;
  * t = 0.0, then t += group[g] for g = 0..31.
Every step is one IEEE fp64 addition, so numpy gives the device's bits or the order differs.

The per-slot values come from ``evaluate(with_distances=True, with_correspondences=True)``: d² and
the matched target index of every source (asserted equal to the oracle in test_gpu_eval.py), and
from the target's fp64 points x, y, z, x·x, y·y, z·z, x·y, x·z, y·z (one rounding each).
Unmatched slots contribute +0.0.

Shapes: ns = 1 (one lane), 257 (a ragged second block), 8453 (34 block rows: groups 0 and 1 add
two rows, the others one); a radius that leaves some sources unmatched.
"""
import numpy as np
import pytest

from m3d import _lib, synth
from m3d.core import Cloud, IcpLoop, evaluate, gicp_terms

pytestmark = pytest.mark.gpu

BLOCK, WAVE, GROUPS = 256, 64, 32
RADIUS = 0.25  # matches 1 of 1, 220 of 257 and 7162 of 8453 sources of the pair below


def device_sum(v):
    """The sum of the per-slot values v (slot order) in the device's order."""
    v = np.asarray(v, np.float64)
    nb = -(-len(v) // BLOCK)
    a = np.zeros(nb * BLOCK)
    a[: len(v)] = v
    w = a.reshape(-1, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    assert (w == w[:, :1]).all()
    wave = w[:, 0].reshape(nb, BLOCK // WAVE)
    partial = np.zeros(nb)
    for k in range(BLOCK // WAVE):
        partial = partial + wave[:, k]
    group = np.zeros(GROUPS)
    for g in range(GROUPS):
        t = np.float64(0.0)
        for b in range(g, nb, GROUPS):
            t = t + partial[b]
        group[g] = t
    t = np.float64(0.0)
    for g in range(GROUPS):
        t = t + group[g]
    return t


def information_of(m):
    """api_icp.cpp eval_information, restated: GᵀG from (count, Σd², Σx Σy Σz, Σx² Σy² Σz², Σxy Σxz Σyz)."""
    n, x, y, z, xx, yy, zz, xy, xz, yz = (m[k] for k in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10))
    U = np.array([[yy + zz, 0.0 - xy, 0.0 - xz, 0.0, 0.0 - z, y],
                  [0.0, xx + zz, 0.0 - yz, z, 0.0, 0.0 - x],
                  [0.0, 0.0, xx + yy, 0.0 - y, x, 0.0],
                  [0.0, 0.0, 0.0, n, 0.0, 0.0],
                  [0.0, 0.0, 0.0, 0.0, n, 0.0],
                  [0.0, 0.0, 0.0, 0.0, 0.0, n]])
    return np.where(np.arange(6)[:, None] <= np.arange(6)[None, :], U, U.T)


def bits(a):
    return np.asarray(a, np.float64).tobytes()


@pytest.fixture(scope="module")
def pair():
    src, tgt, _, T_true = synth.icp_pair(8453, 3000, seed=5)
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), T_true


@pytest.mark.parametrize("nn", ["brute", "grid"])
@pytest.mark.parametrize("ns", [1, 257, 8453])
def test_sums_have_the_documented_order(pair, ns, nn):
    src, tgt, T = pair
    src = src[:ns]
    s, t = Cloud(src), Cloud(tgt)
    out = evaluate(s, t, T, RADIUS, nn=nn, information=True, with_correspondences=True, with_distances=True)
    slots = IcpLoop(s, t, RADIUS, estimation=_lib.EST_POINT_TO_POINT, nn=nn).source_slots().cpu().numpy()
    assert sorted(slots.tolist()) == list(range(ns))
    idx = out.corr_idx.cpu().numpy()[slots]
    d2 = out.d2.cpu().numpy()[slots]
    hit = idx >= 0
    q = tgt[np.where(hit, idx, 0)]
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    per_slot = [np.ones(ns), d2, x, y, z, x * x, y * y, z * z, x * y, x * z, y * z]
    m = np.array([device_sum(np.where(hit, v, 0.0)) for v in per_slot])
    matched = int(m[0])
    print(f"ns {ns} nn {nn}: matched {matched}, sum d2 {m[1]!r}")
    assert matched == int(hit.sum())
    if ns > 1:
        assert 0 < matched < ns
    assert out.num_correspondences == matched
    rmse = np.sqrt(m[1] / np.float64(matched)) if matched > 0 else 0.0
    assert bits(out.inlier_rmse) == bits(rmse)
    assert bits(out.information) == bits(information_of(m))
    # the Generalized-ICP terms pass: the same winners on the same slots, the same order
    eye = np.tile(np.eye(3), (ns, 1, 1)), np.tile(np.eye(3), (len(tgt), 1, 1))
    sums, gidx = gicp_terms(s, t, T, RADIUS, src_cov=eye[0], tgt_cov=eye[1], nn=nn)
    np.testing.assert_array_equal(gidx.cpu().numpy()[slots], idx)
    assert bits(sums[28]) == bits(m[0])
    assert bits(sums[29]) == bits(m[1])
