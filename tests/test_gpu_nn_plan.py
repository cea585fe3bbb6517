"""The slice plan of the brute-force NN launch (nn_plan.h): query block x of
nn_mfma_kernel gets S_x blocks, sized from the tiles it kept in the previous evaluation by wave 1
of the fused tail's last block, read by every block of the next launch from a table of (x, y, S)
entries.  (k1, near2) is a function of the set of keys pushed and is merged by atomics, so the
partition of a query block's tiles over blocks must not change anything: as in
test_gpu_nn_reach.py, at each of three evaluations (the first unseeded, the later ones seeded)
the correspondences equal icp_oracle.nn_exact index for index and the loop's points are the
oracle's incremental points bit for bit — under forced plans (m3d_debug_icp_nn_plan) and under
the loop's own.

Shapes: ns = 1100 (query blocks of 512, 512 and 76 sources) against nt = 5000 (five tiles, the
last ragged) in three blobs of different size; one query; a target of one tile.  No case takes the
far-transform fallback.
"""
import ctypes as C
import hashlib
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
from m3d import synth
from m3d.core import Cloud, IcpLoop, stream_handle

from test_gpu_nn_reach import CELL, R, _blob, _morton_rows

pytestmark = pytest.mark.gpu

SMAX = 8  # nn_plan.h kPlanSmax
EMPTY = 0xFFFFFFFF


def _decode(table):
    t = np.asarray(table, np.uint32)
    t = t[t != EMPTY]
    return (t & 0xFFFF).astype(int), ((t >> 16) & 0xFF).astype(int), (t >> 24).astype(int)


def _force(lp, S):
    arr = np.asarray(S, np.int32)
    return lp.ctx.lib.m3d_debug_icp_nn_plan(lp.h, arr.ctypes.data_as(C.c_void_p), len(arr), stream_handle())


def _read(lp):
    """(query blocks, budget, flag, counts the planner last read, table)"""
    shape = np.zeros(3, np.int32)
    lib = lp.ctx.lib
    lp.ctx.check(lib.m3d_debug_icp_nn_plan_read(lp.h, None, None, shape.ctypes.data_as(C.c_void_p), stream_handle()),
                 "plan_read")
    nq, budget = int(shape[0]), int(shape[1])
    cnt, tab = np.zeros(max(nq, 1), np.uint32), np.zeros(max(budget, 1), np.uint32)
    lp.ctx.check(lib.m3d_debug_icp_nn_plan_read(lp.h, cnt.ctypes.data_as(C.c_void_p), tab.ctypes.data_as(C.c_void_p),
                                                shape.ctypes.data_as(C.c_void_p), stream_handle()), "plan_read")
    return nq, budget, int(shape[2]), cnt[:nq], tab[:budget]


def _host_rule(lib, counts, budget, smax, ntiles, with_tau=False):
    counts = np.ascontiguousarray(counts, np.uint32)
    out = np.zeros(budget, np.uint32)
    tau = lib.m3d_debug_nn_plan_host(counts.ctypes.data_as(C.c_void_p), len(counts), budget, smax, ntiles,
                                     out.ctypes.data_as(C.c_void_p))
    assert tau >= 1
    return (out, tau) if with_tau else out


def _check_loop(src, tgt, nrm, plan=None, r=R, n_evals=3, init=None):
    """test_gpu_nn_reach._check_loop with a plan forced after the reset (None: the loop's own).
    Returns the loop and every evaluation's correspondences and update."""
    init = np.eye(4) if init is None else init
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), r, relative_fitness=-1, relative_rmse=-1,
                 max_iteration=n_evals, nn="brute")
    tree = cKDTree(tgt)
    lp.reset(init)
    if plan is not None:
        assert _force(lp, plan) == 0
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
    if plan is not None:  # the planner left the forced plan alone
        nq, _, flag, _, tab = _read(lp)
        x, y, S = _decode(tab)
        assert flag == 2 and nq == len(plan)
        assert sorted(zip(x, y)) == [(k, j) for k in range(nq) for j in range(plan[k])]
        assert all(S[i] == plan[x[i]] for i in range(len(x)))
    return lp, corrs, updates


def _blobs_pair():
    """ns = 1100 against nt = 5000: blobs of 3000, 1500 and 500 targets, 600 / 400 / 100 sources."""
    parts = [_blob(3000, 1, (0, 0, 0)), _blob(1500, 2, (3, 0, 0)), _blob(500, 3, (0, 3, 0))]
    tgt, nrm = np.vstack([p for p, _ in parts]), np.vstack([n for _, n in parts])
    smp = np.vstack([_blob(600, 4, (0, 0, 0))[0], _blob(400, 5, (3, 0, 0))[0], _blob(100, 6, (0, 3, 0))[0]])
    T = synth.random_rigid(5, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    return synth.apply(np.linalg.inv(T), smp), tgt, nrm


@pytest.fixture(scope="module")
def blobs():
    return _blobs_pair()


@pytest.mark.parametrize("plan", [(1, 1, 1), (5, 1, 2), (2, 5, 1)])
def test_forced_plans(blobs, plan):
    src, tgt, nrm = blobs
    _, corrs, _ = _check_loop(src, tgt, nrm, plan=plan)
    assert (corrs[-1] >= 0).mean() > 0.8


def test_forced_plan_ties_across_slices():
    """(3, 3, 3): tiles 0 and 3 go to slice 0, 1 and 4 to slice 1, 2 to slice 2.  The Morton-cell
    construction of test_gpu_nn_reach.py's near ties, on five tiles: four queries on the x = 8
    cells plane, each with a target `lo` = q − (d, 0, 0) in tile 0 and `hi` = q + (d, 0, 0) in
    tile 4 — different slices — and a patch of 4991 targets between them in row order.  Queries 0
    and 1: exact ties in fp64, the lower index (`hi`) wins; query 2: `lo` moved by 2⁻³⁰ ≈ 1e-9 in
    y, one fp64 ulp farther, `hi` wins; query 3: `hi` moved, `lo` wins.  Every other source is a
    copy of a patch target: the update is the identity and all three evaluations, the seeded ones
    with the tight bound, see the same geometry."""
    rng = np.random.default_rng(31)
    d = 0.078125
    q = np.array([[0.9609375, 0.05 + 0.12 * k, 0.05] for k in range(4)])
    hi, lo = q + [d, 0.0, 0.0], q - [d, 0.0, 0.0]
    lo[2] += [0.0, 2.0 ** -30, 0.0]
    hi[3] += [0.0, 2.0 ** -30, 0.0]
    npatch = 4991
    x, y = rng.uniform(0.02, 0.9, npatch), rng.uniform(0.02, 0.9, npatch)
    z = 0.7 + 0.1 * np.sin(4.0 * x) * np.cos(4.0 * y)
    gx, gy = 0.4 * np.cos(4.0 * x) * np.cos(4.0 * y), -0.4 * np.sin(4.0 * x) * np.sin(4.0 * y)
    n3 = np.column_stack([-gx, -gy, np.ones(npatch)])
    pt, pn = np.column_stack([x, y, z]), n3 / np.linalg.norm(n3, axis=1, keepdims=True)
    tgt = np.vstack([hi, lo, np.zeros((1, 3)), pt])  # hi: 0..3, lo: 4..7, the grid's origin; nt = 5000
    nrm = np.vstack([np.tile([0.0, 0.0, 1.0], (9, 1)), pn])
    dh, dl = I.sq_dist(q, hi), I.sq_dist(q, lo)
    assert np.array_equal(dh[:2], dl[:2])
    assert np.nextafter(dh[2], np.inf) == dl[2] and np.nextafter(dl[3], np.inf) == dh[3]
    row = _morton_rows(tgt)
    for k in range(4):
        assert row[k] // 1024 == 4 and row[4 + k] // 1024 == 0, (row[k], row[4 + k])
    src = np.vstack([q, pt[:1096]])  # ns = 1100
    _, corrs, updates = _check_loop(src, tgt, nrm, plan=(3, 3, 3))
    for u in updates:
        np.testing.assert_array_equal(u, np.eye(4))
    for corr in corrs:
        np.testing.assert_array_equal(corr[:4], [0, 1, 2, 7])
        np.testing.assert_array_equal(corr[4:], 9 + np.arange(1096))


def test_forced_plan_errors(blobs):
    """S > the target's tiles, S < 1, Σ S > the resident slots and a wrong length are refused, and
    leave the loop without a forced plan."""
    src, tgt, nrm = blobs
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, relative_fitness=-1, relative_rmse=-1, max_iteration=3, nn="brute")
    lp.reset(np.eye(4))
    nq, budget, flag, _, _ = _read(lp)
    assert (nq, flag) == (3, 0) and budget >= 8
    assert _force(lp, (6, 1, 1)) != 0  # five tiles
    assert _force(lp, (0, 1, 1)) != 0
    assert _force(lp, (1, 1)) != 0
    ns2 = 512 * (budget // 5 + 1)  # enough query blocks that five slices each exceed the slots
    lp2 = IcpLoop(Cloud(np.tile(src, (ns2 // len(src) + 1, 1))[:ns2]), Cloud(tgt, nrm), R,
                  relative_fitness=-1, relative_rmse=-1, max_iteration=3, nn="brute")
    lp2.reset(np.eye(4))
    nq2 = _read(lp2)[0]
    assert nq2 * 5 > budget
    assert _force(lp2, [5] * nq2) != 0  # more slices than slots
    assert _read(lp)[2] == 0 and _read(lp2)[2] == 0


def test_own_plan_is_the_host_rule(blobs):
    """Four evaluations under the loop's own plan, each checked against the oracle; after each the
    table read back equals the host rule applied to the counts read back with it, the three query
    blocks' counts differ (the premise of the shape), and a reset clears the flag."""
    src, tgt, nrm = blobs
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, relative_fitness=-1, relative_rmse=-1, max_iteration=4, nn="brute")
    tree = cKDTree(tgt)
    lp.reset(np.eye(4))
    assert _read(lp)[2] == 0
    want = I.initial_points(np.eye(4), src)
    for it in range(4):
        lp.step()
        pts = lp.points().cpu().numpy()
        np.testing.assert_array_equal(pts, want, err_msg=f"points, evaluation {it}")
        np.testing.assert_array_equal(lp.correspondences().cpu().numpy(), I.nn_exact(tree, tgt, pts, R)[0])
        want = I.transform_points(np.array(lp.result().update), pts)
        nq, budget, flag, cnt, tab = _read(lp)
        print(f"evaluation {it}: counts {cnt.tolist()} plan S {sorted(set(zip(*_decode(tab)[::2])))}")
        assert (nq, flag) == (3, 1)
        assert 1 <= cnt.min() and cnt.max() <= 5 and cnt.max() > cnt.min()
        np.testing.assert_array_equal(tab, _host_rule(lp.ctx.lib, cnt, budget, SMAX, 5))
    lp.reset(np.eye(4))
    assert _read(lp)[2] == 0


_CODE = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [sys.argv[1]]
import torch
from m3d.core import Cloud, IcpLoop
z = np.load(sys.argv[2])
src, tgt, nrm = z["src"], z["tgt"], z["nrm"]
lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), 0.12, relative_fitness=-1, relative_rmse=-1, max_iteration=4, nn="brute")
lp.reset(np.eye(4))
out = []
for it in range(4):
    lp.step()
    r = lp.result()
    out.append([hashlib.sha256(lp.correspondences().cpu().numpy().tobytes()).hexdigest(),
                hashlib.sha256(lp.points().cpu().numpy().tobytes()).hexdigest(),
                np.asarray(r.transformation).tobytes().hex(), float(r.fitness).hex(), float(r.inlier_rmse).hex()])
print(json.dumps(out))
'''


def test_own_plan_equals_the_uniform_launch(blobs, tmp_path):
    """Four evaluations with the plan on and with M3D_NN_PLAN=0 (the uniform 2-D launch), a process
    each (the switch is read once): correspondences, points and result equal in every bit."""
    root = Path(__file__).resolve().parents[1]
    np.savez(tmp_path / "pair.npz", src=blobs[0], tgt=blobs[1], nrm=blobs[2])
    res = {}
    for on in ("0", "1"):
        env = dict(os.environ, M3D_NN_PLAN=on)
        r = subprocess.run([sys.executable, "-c", _CODE, str(root / "3d-matching_amd"), str(tmp_path / "pair.npz")], env=env,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        res[on] = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["0"] == res["1"]


@pytest.mark.parametrize("shape", ["one_query", "one_tile"])
def test_small_shapes(shape):
    """One query (a single query block, 63 inactive lanes) against five tiles, and 1100 queries
    against a target of one tile, where every S clamps to 1 whatever the counts."""
    if shape == "one_query":
        tgt, nrm = _blob(5000, 3, (0, 0, 0))
        src = _blob(1, 4, (0, 0, 0), scale=0.1003)[0]
    else:
        tgt, nrm = _blob(800, 3, (0, 0, 0))
        src = _blob(1100, 4, (0, 0, 0), scale=0.1003)[0]
    lp, corrs, _ = _check_loop(src, tgt, nrm)
    nq, budget, flag, cnt, tab = _read(lp)
    x, y, S = _decode(tab)
    assert flag == 1 and nq == (1 if shape == "one_query" else 3)
    np.testing.assert_array_equal(tab, _host_rule(lp.ctx.lib, cnt, budget, SMAX, 5 if shape == "one_query" else 1))
    if shape == "one_tile":
        assert S.tolist() == [1, 1, 1] and y.tolist() == [0, 0, 0] and x.tolist() == [0, 1, 2]
    else:
        assert len(S) == S[0] <= 5


def test_graph_replay_equals_steps(blobs):
    """steps(4) requested twice is captured into a graph and replayed (m3d_icp_steps): the plan's
    table, counts and flag are device state like everything else in the graph, so the replay
    equals four plain step() calls."""
    src, tgt, nrm = blobs
    mk = lambda: IcpLoop(Cloud(src), Cloud(tgt, nrm), R, relative_fitness=-1, relative_rmse=-1, max_iteration=4,
                         nn="brute")
    a, b = mk(), mk()
    a.reset(np.eye(4))
    a.steps(4)
    a.reset(np.eye(4))
    a.steps(4)  # the replay
    b.reset(np.eye(4))
    for _ in range(4):
        b.step()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(a.correspondences().cpu().numpy(), b.correspondences().cpu().numpy())
    np.testing.assert_array_equal(a.points().cpu().numpy(), b.points().cpu().numpy())
    ra, rb = a.result(), b.result()
    np.testing.assert_array_equal(ra.transformation, rb.transformation)
    assert (ra.fitness, ra.inlier_rmse, ra.iterations) == (rb.fitness, rb.inlier_rmse, rb.iterations)
    ta, tb = _read(a), _read(b)
    assert ta[2] == tb[2] == 1
    np.testing.assert_array_equal(ta[3], tb[3])
    np.testing.assert_array_equal(ta[4], tb[4])


def test_device_rule_with_tau_above_one():
    """The device planner divides by fp32 reciprocal with an fma correction, the host entry by
    integer division; the shapes above all end at τ = 1, where the quotient is the count itself.
    150 query blocks (ns = 76 800) against 59 tiles: the query blocks keep several tiles each, at
    τ = 1 the slices exceed the resident slots, so the bisection runs and ends above one.  The
    table the device wrote equals the host rule on the counts read back with it, at each of three
    evaluations, and the last evaluation's correspondences are the exact ones."""
    src, tgt, nrm, _ = synth.icp_pair(76_800, 60_000, seed=11)
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, relative_fitness=-1, relative_rmse=-1, max_iteration=3, nn="brute")
    lp.reset(np.eye(4))
    taus = []
    for it in range(3):
        lp.step()
        nq, budget, flag, cnt, tab = _read(lp)
        assert (nq, flag) == (150, 1)
        want, tau = _host_rule(lp.ctx.lib, cnt, budget, SMAX, 59, with_tau=True)
        print(f"evaluation {it}: budget {budget}, counts {cnt.min()}..{cnt.max()} (sum {cnt.sum()}), tau {tau}")
        np.testing.assert_array_equal(tab, want)
        assert len(set(cnt.tolist())) > 3  # remainders of several kinds under the division
        taus.append(tau)
    assert max(taus) > 1, taus
    pts = lp.points().cpu().numpy()
    np.testing.assert_array_equal(lp.correspondences().cpu().numpy(), I.nn_exact(cKDTree(tgt), tgt, pts, R)[0])
