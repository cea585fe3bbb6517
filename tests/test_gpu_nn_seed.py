"""Seed records of the self-seeded brute-force scan: the fused tail that hands the
keys back also leaves, per source in slot order, the centred fp32 point and the index of its
correspondence (the last 16 bytes of the 64-byte target record it gathered anyway), and the next
scan forms its starting key from that record instead of gathering tgt32[corr[i]].  The key is the
same fp32 operations on the same bits, so nothing may change — but a record that is merely too
loose, or always "none", would still give the right correspondences, only slower.  So the records
themselves are read back (m3d_debug_icp_seed_read) and compared bit for bit, and the loop is
checked as in test_gpu_nn_reach.py / test_gpu_nn_plan.py: at every evaluation the correspondences
equal icp_oracle.nn_exact index for index and the points are the oracle's incremental points.

Shapes: ns = 1100 (query blocks of 512, 512 and 76) against nt = 5000 (five tiles, the last
ragged), three blobs; one query; a target of one tile.
"""
import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import icp_oracle as I
from m3d import _lib, synth
from m3d.core import Cloud, IcpLoop, stream_handle
from shard_emulation import shard_step

from test_gpu_nn_plan import _blobs_pair, _force
from test_gpu_nn_reach import R, _blob

pytestmark = pytest.mark.gpu


def _records(lp):
    """(seed records ns×4 as uint32 bits, corr in slot order, the target's device fp32 rows as
    bits, live, mfma_ok)"""
    ns, nt = lp.src.n, lp.tgt.n
    seed, corr = np.zeros((max(ns, 1), 4), np.float32), np.zeros(max(ns, 1), np.int32)
    t32, info = np.zeros((max(nt, 1), 4), np.float32), np.zeros(2, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lp.ctx.check(lp.ctx.lib.m3d_debug_icp_seed_read(lp.h, vp(seed), vp(corr), vp(t32), vp(info), stream_handle()),
                 "seed_read")
    return seed[:ns].view(np.uint32), corr[:ns], t32[:nt].view(np.uint32), int(info[0]), int(info[1])


def _check_records(lp, what=""):
    """keys_clean ⇒ seed[i] describes corr[i]: w is corr[i]; where it names a target the xyz are
    that target's device fp32 row bit for bit; where it is −1 the query has no correspondence (in
    the caller's order too, through the slot map)."""
    seed, corr, t32, live, _ = _records(lp)
    assert live == 1, what
    w = seed[:, 3].view(np.int32)
    np.testing.assert_array_equal(w, corr, err_msg=f"record index, {what}")
    assert w.min() >= -1 and w.max() < lp.tgt.n
    has = w >= 0
    np.testing.assert_array_equal(seed[has, :3], t32[w[has], :3], err_msg=f"record point, {what}")
    user = lp.correspondences().cpu().numpy()
    slots = lp.source_slots().cpu().numpy()
    np.testing.assert_array_equal(user[slots], corr, err_msg=f"slot order, {what}")
    assert np.array_equal(user[slots[~has]], np.full((~has).sum(), -1))
    return seed, corr, t32


def _check_loop(src, tgt, nrm, plan=None, r=R, n_evals=3, init=None, estimation=_lib.EST_POINT_TO_PLANE):
    """test_gpu_nn_plan._check_loop with the records checked after every evaluation."""
    init = np.eye(4) if init is None else init
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), r, relative_fitness=-1, relative_rmse=-1,
                 max_iteration=n_evals, nn="brute", estimation=estimation)
    tree = cKDTree(tgt)
    lp.reset(init)
    if plan is not None:
        assert _force(lp, plan) == 0
    want = I.initial_points(init, src)
    corrs = []
    for it in range(n_evals):
        lp.step()
        pts = lp.points().cpu().numpy()
        np.testing.assert_array_equal(pts, want, err_msg=f"points, evaluation {it}")
        ref_j, _ = I.nn_exact(tree, tgt, pts, r)
        corr = lp.correspondences().cpu().numpy()
        np.testing.assert_array_equal(corr, ref_j, err_msg=f"evaluation {it}")
        _check_records(lp, f"evaluation {it}")
        corrs.append(corr)
        want = I.transform_points(np.array(lp.result().update), pts)
    return lp, corrs


@pytest.fixture(scope="module")
def blobs():
    return _blobs_pair()


def test_records_are_exact():
    """The blobs pair with 20 sources 50 units off (never a correspondence) and six sources a hair
    inside r around an isolated target, on both sides along each axis: whichever way the first
    update moves them, some lose that correspondence at the next evaluation."""
    src, tgt, nrm = _blobs_pair()
    star = np.array([0.0, -3.0, 0.0])
    tgt = np.vstack([tgt[:4999], star])
    nrm = np.vstack([nrm[:4999], [0.0, 0.0, 1.0]])
    arms = star + (R - 2e-4) * np.vstack([np.eye(3), -np.eye(3)])
    far = _blob(20, 9, (50.0, 0.0, 0.0))[0]
    src = np.vstack([src[:1074], far, arms])
    assert src.shape == (1100, 3) and tgt.shape == (5000, 3)
    lp, corrs = _check_loop(src, tgt, nrm)
    assert all((c[1074:1094] == -1).all() for c in corrs)
    assert (corrs[0][1094:] == 4999).all()
    lost = (corrs[0] >= 0) & (corrs[1] == -1)
    assert lost[1094:].any(), "premise: a first correspondence lost after the update"
    assert (corrs[-1] >= 0).mean() > 0.8


@pytest.mark.parametrize("plan", [None, (2, 5, 1)])
def test_loop_is_the_oracles(blobs, plan):
    """Under the loop's own plan and under a forced plan with S > 1: slice 0 publishes the seed
    every slice started from."""
    src, tgt, nrm = blobs
    _, corrs = _check_loop(src, tgt, nrm, plan=plan)
    assert (corrs[-1] >= 0).mean() > 0.8


@pytest.mark.parametrize("shape", ["one_query", "one_tile"])
def test_small_shapes(shape):
    if shape == "one_query":
        tgt, nrm = _blob(5000, 3, (0, 0, 0))
        src = _blob(1, 4, (0, 0, 0), scale=0.1003)[0]
    else:
        tgt, nrm = _blob(800, 3, (0, 0, 0))
        src = _blob(1100, 4, (0, 0, 0), scale=0.1003)[0]
    _, corrs = _check_loop(src, tgt, nrm)
    assert (corrs[-1] >= 0).all()


def test_ambiguous_winners():
    """Exact duplicates and 1e-9 near-duplicates (one fp32 point, two fp64 points), as
    test_icp_ambiguous_pairs_and_triples_exact builds them: the scan's k1 names the lowest index
    among equal fp32 distances, the fp64 winner may be the copy.  The record carries the winner:
    some records name a near-duplicate copy whose fp32 row equals the original's bit for bit, and
    the evaluations seeded from them still match the oracle."""
    base, bn = _blob(3000, 3, (0, 0, 0))
    near = base[1000:2000].copy()
    near[:, 0] += 1e-9
    tgt = np.vstack([base, base[:1000], near])  # originals 0..2999, exact copies 3000.., near copies 4000..
    nrm = np.vstack([bn, bn[:1000], bn[1000:2000]])
    src = _blob(1100, 4, (0, 0, 0), scale=0.1003)[0]
    lp, corrs = _check_loop(src, tgt, nrm, n_evals=4)
    seed, corr, t32 = _check_records(lp)
    assert np.isin(corr, np.arange(1000)).any() and not np.isin(corr, np.arange(3000, 4000)).any()
    copy = corr >= 4000
    same32 = (t32[corr[copy], :3] == t32[corr[copy] - 3000, :3]).all(axis=1)
    assert same32.any(), "premise: a winner whose fp32 point is also a lower index's"
    np.testing.assert_array_equal(seed[copy, 3].view(np.int32), corr[copy])


def test_point_to_point(blobs):
    src, tgt, nrm = blobs
    _check_loop(src, tgt, nrm, estimation=_lib.EST_POINT_TO_POINT)


def test_far_source_takes_the_plain_scan(blobs):
    """One source 3e4 units away puts the scaled query bound past the fp16 range (mfma_ok = 0):
    every evaluation, the seeded ones included, runs nn_slice_scan."""
    src, tgt, nrm = blobs
    src = np.vstack([src[:1099], [[3e4, 0.0, 0.0]]])
    lp, corrs = _check_loop(src, tgt, nrm)
    assert _records(lp)[4] == 0
    assert corrs[-1][1099] == -1 and (corrs[-1] >= 0).mean() > 0.8


_CODE = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1]]
import torch
from m3d.core import Cloud, IcpLoop
z = np.load(sys.argv[2])
src, tgt, nrm = z["src"], z["tgt"], z["nrm"]
out = {}
for nn in sys.argv[3:]:
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), 0.12, relative_fitness=-1, relative_rmse=-1, max_iteration=4, nn=nn)
    lp.reset(np.eye(4))
    out[nn] = []
    for it in range(4):
        lp.step()
        r = lp.result()
        out[nn].append([hashlib.sha256(lp.correspondences().cpu().numpy().tobytes()).hexdigest(),
                        hashlib.sha256(lp.points().cpu().numpy().tobytes()).hexdigest(),
                        np.asarray(r.transformation).tobytes().hex()])
print(json.dumps(out))
'''


def test_same_bits_as_the_gather_path(blobs, tmp_path):
    """M3D_ICP_FUSED=0 (separate tail, keyinit launch: no record is written or read) against the
    default, a process each, and the default's grid loop: transformation, correspondences and
    points of four evaluations equal in every bit."""
    root = Path(__file__).resolve().parents[1]
    np.savez(tmp_path / "pair.npz", src=blobs[0], tgt=blobs[1], nrm=blobs[2])
    res = {}
    for fused, nns in (("0", ["brute"]), ("1", ["brute", "grid"])):
        env = dict(os.environ, M3D_ICP_FUSED=fused)
        r = subprocess.run([sys.executable, "-c", _CODE, str(root / "3d-matching_amd"), str(tmp_path / "pair.npz")] + nns,
                           env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        res[fused] = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["0"]["brute"] == res["1"]["brute"]
    assert res["1"]["grid"] == res["1"]["brute"]


def _state(lp):
    r = lp.result()
    return (lp.correspondences().cpu().numpy(), lp.points().cpu().numpy(), np.array(r.transformation),
            (r.fitness, r.inlier_rmse, r.iterations))


def _assert_same(a, b):
    for x, y in zip(_state(a), _state(b)):
        np.testing.assert_array_equal(x, y)


def _mk(blobs, n=4):
    return IcpLoop(Cloud(blobs[0]), Cloud(blobs[1], blobs[2]), R, relative_fitness=-1, relative_rmse=-1,
                   max_iteration=n, nn="brute")


def test_reset_leaves_no_stale_record(blobs):
    """Three steps, a reset to another initial transform, three steps: a fresh loop's result (the
    first evaluation after the reset must not start from the old records)."""
    T2 = synth.random_rigid(8, center=blobs[1].mean(axis=0), rot_range=0.02, trans_range=0.05)
    a, b = _mk(blobs), _mk(blobs)
    a.reset(np.eye(4))
    for _ in range(3):
        a.step()
    assert _records(a)[3] == 1
    a.reset(T2)
    assert _records(a)[3] == 0
    b.reset(T2)
    for _ in range(3):
        a.step()
        b.step()
    _assert_same(a, b)
    _check_records(a)


def test_unseeded_evaluation_between_steps(blobs):
    """step, one evaluation by the target-shard calls (keyinit from corr, a tail that writes corr
    but no record), step: three plain steps' result, and the records describe the last corr."""
    a, b = _mk(blobs), _mk(blobs)
    a.reset(np.eye(4))
    b.reset(np.eye(4))
    a.step()
    sums = torch.empty(32, dtype=torch.float64, device="cuda")
    shard_step(a, 0, len(blobs[0]), sums)
    assert _records(a)[3] == 0
    a.step()
    for _ in range(3):
        b.step()
    _assert_same(a, b)
    _check_records(a)


def test_source_shard_calls_are_seeded(blobs):
    """The source-shard calls (keys kept inside, launch_icp_terms_reduce hands them back): records
    written and read as in step()."""
    a, b = _mk(blobs), _mk(blobs)
    a.reset(np.eye(4))
    b.reset(np.eye(4))
    sums = torch.empty(32, dtype=torch.float64, device="cuda")
    for _ in range(3):
        a.shard_nn(0, None)
        a.shard_terms(0, None, None, sums)
        a.solve(sums)
        _check_records(a)
        b.step()
    _assert_same(a, b)


def test_graph_replay_equals_steps(blobs):
    """steps(4) requested twice is captured and replayed: equal to four step() calls, records too."""
    a, b = _mk(blobs), _mk(blobs)
    a.reset(np.eye(4))
    a.steps(4)
    a.reset(np.eye(4))
    a.steps(4)  # the replay
    b.reset(np.eye(4))
    for _ in range(4):
        b.step()
    torch.cuda.synchronize()
    _assert_same(a, b)
    ra, rb = _check_records(a), _check_records(b)
    np.testing.assert_array_equal(ra[0], rb[0])
