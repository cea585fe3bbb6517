"""The iteration whose terms pass runs inside the brute-force NN launch:
nn_mfma_terms_kernel's blocks add, after their publish, to a ticket of their query block, and the
block that adds last runs that query block's terms pass in place; reduce_solve_kernel, one block,
follows.  The code of the terms pass and the summation order are the ones of the fused tail, so
every comparison here is between two loops on the same data — one with the path on, one with it
off through m3d_debug_icp_nn_terms — and bit for bit: transformation and update after every step,
fitness and rmse, correspondences, points, seed records, the plan's counts and table.

Shapes: ns = 1300 (query blocks of 512, 512 and 276), 512 and 513 (a second query block of one
source) against nt = 3000 (three tiles: the uniform slice count is clamped by the tile count);
nt = 9000 (nine tiles) where a forced plan asks for eight slices.  The selection rule itself is
checked without a GPU (test_selection_rule).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from m3d import _lib, synth
from m3d.core import Cloud, IcpLoop, stream_handle

from test_gpu_nn_plan import _force, _read
from test_gpu_nn_reach import R, _blob
from test_gpu_nn_seed import _records

gpu = pytest.mark.gpu
STEPS = 10


def _switch(lp, on):
    return lp.ctx.lib.m3d_debug_icp_nn_terms(lp.h, int(on))


def _tickets(lp):
    """(tickets, counts) of the loop's query blocks as they are on the device"""
    nq = _read(lp)[0]
    tix, cnt = np.full(max(nq, 1), 0xDEAD, np.uint32), np.full(max(nq, 1), 0xDEAD, np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lp.ctx.lib.m3d_debug_icp_nn_terms_read(lp.h, vp(tix), vp(cnt), stream_handle()) == nq
    return tix[:nq], cnt[:nq]


def _snap(lp):
    r = lp.result()
    seed, corr, _, live, mfma_ok = _records(lp)
    nq, budget, flag, seen, table = _read(lp)
    tix, cnt = _tickets(lp)
    return {"transformation": np.array(r.transformation), "update": np.array(r.update),
            "fitness": np.float64(r.fitness), "rmse": np.float64(r.inlier_rmse), "iterations": np.int64(r.iterations),
            "corr": corr, "corr_user": lp.correspondences().cpu().numpy(), "points": lp.points().cpu().numpy(),
            "seed": seed, "live": np.int64(live), "mfma_ok": np.int64(mfma_ok), "plan_flag": np.int64(flag),
            "plan_seen": seen, "plan_table": table, "counts": cnt, "tickets": tix}


def _same(a, b, what):
    sa, sb = _snap(a), _snap(b)
    for k in sa:
        np.testing.assert_array_equal(sa[k].view(np.uint64) if sa[k].dtype == np.float64 else sa[k],
                                      sb[k].view(np.uint64) if sb[k].dtype == np.float64 else sb[k],
                                      err_msg=f"{k}, {what}")
    assert not sa["tickets"].any(), f"tickets left, {what}"
    return sa


def _pair_of_loops(src, tgt, nrm, n=STEPS, **kw):
    kw = dict(dict(relative_fitness=-1, relative_rmse=-1, max_iteration=n, nn="brute"), **kw)
    on, off = (IcpLoop(Cloud(src), Cloud(tgt, nrm), R, **kw) for _ in range(2))
    assert _switch(on, 1) == 1, "the loop does not take the path"
    assert _switch(off, 0) == 0
    return on, off


def _run_pair(src, tgt, nrm, plan=None, n=STEPS, init=None):
    on, off = _pair_of_loops(src, tgt, nrm, n)
    snaps = []
    for lp in (on, off):
        lp.reset(np.eye(4) if init is None else init)
        if plan is not None:
            assert _force(lp, plan) == 0
    for it in range(n):
        on.step()
        off.step()
        snaps.append(_same(on, off, f"step {it}"))
    return on, off, snaps


def _cloud_pair(ns, nt, seed=0):
    tgt, nrm = _blob(nt, 1 + seed, (0, 0, 0))
    smp = _blob(ns, 4 + seed, (0, 0, 0))[0]
    T = synth.random_rigid(5 + seed, center=tgt.mean(axis=0), rot_range=0.01, trans_range=0.02)
    return synth.apply(np.linalg.inv(T), smp), tgt, nrm


@pytest.fixture(scope="module")
def pair1300():
    return _cloud_pair(1300, 3000)


@pytest.fixture(scope="module")
def pair9000():
    return _cloud_pair(1300, 9000, seed=1)


@gpu
@pytest.mark.parametrize("ns", [1300, 512, 513])
def test_shapes(ns, pair1300):
    """The loop's own plans: the first evaluation has none (the uniform assignment, S clamped to
    the three tiles), the later ones the planner's."""
    src, tgt, nrm = pair1300 if ns == 1300 else _cloud_pair(ns, 3000)
    _, _, snaps = _run_pair(src, tgt, nrm)
    assert snaps[0]["plan_flag"] == 1 and snaps[-1]["fitness"] > 0.8
    assert len(snaps[0]["counts"]) == -(-ns // 512)


@gpu
@pytest.mark.parametrize("plan", [(1, 1, 1), (8, 1, 3), (3, 8, 1)], ids=["all_one", "mixed_813", "mixed_381"])
def test_forced_plans(plan, pair9000):
    """Forced tables: one slice each (the block that scans is the block that runs the terms), and
    1 / 3 / 8 slices mixed; 3 to 12 live entries of the table's 512, the rest empty."""
    src, tgt, nrm = pair9000
    on, _, snaps = _run_pair(src, tgt, nrm, plan=plan)
    assert all(s["plan_flag"] == 2 for s in snaps)
    live = snaps[-1]["plan_table"] != 0xFFFFFFFF
    assert live.sum() == sum(plan) and not live.all()
    assert snaps[-1]["fitness"] > 0.8


@gpu
def test_query_block_without_a_neighbour(pair1300):
    """600 sources 50 units away: in Morton order they fill the last query block (and part of the
    one before), whose terms pass still stores a zero partial, corr = −1 and clears its ticket."""
    src, tgt, nrm = pair1300
    far = _blob(600, 9, (50.0, 0.0, 0.0))[0]
    src = np.vstack([src[:700], far])
    on, _, snaps = _run_pair(src, tgt, nrm)
    slots = on.source_slots().cpu().numpy()
    assert (slots[-512:] >= 700).all(), "premise: the last query block holds far sources only"
    assert (snaps[-1]["corr"][-512:] == -1).all() and (snaps[-1]["corr"][:512] >= 0).mean() > 0.8


@gpu
def test_duplicate_targets():
    """Exact and 1e-9 near-duplicates of targets (test_gpu_nn_seed.test_ambiguous_winners): ambiguous
    queries, resolved by resolve_wave inside the NN kernel."""
    base, bn = _blob(3000, 3, (0, 0, 0))
    near = base[1000:2000].copy()
    near[:, 0] += 1e-9
    tgt = np.vstack([base, base[:1000], near])
    nrm = np.vstack([bn, bn[:1000], bn[1000:2000]])
    src = _blob(1300, 4, (0, 0, 0), scale=0.1003)[0]
    _, _, snaps = _run_pair(src, tgt, nrm)
    assert (snaps[-1]["corr"] >= 4000).any(), "premise: a winner that is a near-duplicate copy"


@gpu
def test_far_source_takes_the_plain_scan(pair1300):
    """One source 3e4 units away: mfma_ok = 0, every evaluation runs nn_slice_scan and the same
    hand-off behind it."""
    src, tgt, nrm = pair1300
    src = np.vstack([src[:1299], [[3e4, 0.0, 0.0]]])
    _, _, snaps = _run_pair(src, tgt, nrm)
    assert all(s["mfma_ok"] == 0 for s in snaps)
    assert snaps[-1]["fitness"] > 0.8


@gpu
def test_graph_replay_and_resets(pair1300):
    """steps(3) from both entry states (after a reset: keyinit first; after steps: self-seeded),
    requested, captured and replayed, with resets in between, against step() calls of a loop with
    the path off; after every reset the tickets and the counts are zero."""
    src, tgt, nrm = pair1300
    on, off = _pair_of_loops(src, tgt, nrm, n=40)
    T2 = synth.random_rigid(8, center=tgt.mean(axis=0), rot_range=0.02, trans_range=0.05)
    for rnd, init in enumerate((np.eye(4), T2, np.eye(4))):  # round 0 requests, 1 captures, 2 replays
        for lp in (on, off):
            lp.reset(init)
            tix, cnt = _tickets(lp)
            assert not tix.any() and not cnt.any(), f"after reset {rnd}"
        for part in range(2):
            on.steps(3)
            for _ in range(3):
                off.step()
            torch.cuda.synchronize()
            _same(on, off, f"round {rnd}, part {part}")
    # a reset in the middle of a replayed run, then the other slot's graph
    on.steps(3)
    for _ in range(3):
        off.step()
    for lp in (on, off):
        lp.reset(T2)
        tix, cnt = _tickets(lp)
        assert not tix.any() and not cnt.any()
    on.steps(3)
    for _ in range(3):
        off.step()
    torch.cuda.synchronize()
    _same(on, off, "after the reset in the middle")


@gpu
def test_converged_loop_writes_nothing(pair1300):
    """max_iteration = 2: the third evaluation sets `done`; two more steps change nothing."""
    src, tgt, nrm = pair1300
    on, off = _pair_of_loops(src, tgt, nrm, n=2, relative_fitness=1e-6, relative_rmse=1e-6)
    for lp in (on, off):
        lp.reset(np.eye(4))
    for it in range(3):
        on.step()
        off.step()
        _same(on, off, f"step {it}")
    before = _snap(on)
    for it in range(2):
        on.step()
        off.step()
        after = _same(on, off, f"done, step {it}")
        for k in before:
            np.testing.assert_array_equal(before[k], after[k], err_msg=f"{k} written by a done loop")


# bits of m3d_debug_nn_terms_select
PLANNED, FUSED, RESET, P2PLANE, REC64, SEED, CLAIM, ONE_DEVICE, ON = (1 << k for k in range(9))
ALL = PLANNED | FUSED | RESET | P2PLANE | REC64 | SEED | ONE_DEVICE | ON


def test_selection_rule():
    """The path is selected for exactly one of the 512 combinations; every path that runs the
    launches it ran before is named here by the condition it fails."""
    sel = _lib.load().m3d_debug_nn_terms_select
    assert sel(ALL) == 1
    for bits in range(512):
        assert sel(bits) == (1 if bits == ALL else 0), bin(bits)
    unchanged = {
        "2-D launch (1M source, M3D_NN_PLAN=0), grid NN, cfg3": ALL & ~PLANNED,
        "M3D_ICP_FUSED=0, past 256 blocks without keys back": ALL & ~FUSED,
        "grid NN / empty source (the tail hands no keys back)": ALL & ~RESET,
        "point-to-point": ALL & ~P2PLANE,
        "no target records (empty target)": ALL & ~REC64,
        "no seed records": ALL & ~SEED,
        "target shard with a claim": ALL | CLAIM,
        "source shard of a multi-device loop": ALL & ~ONE_DEVICE,
        "switched off (M3D_NN_TERMS=0, m3d_debug_icp_nn_terms)": ALL & ~ON,
    }
    for what, bits in unchanged.items():
        assert sel(bits) == 0, what


@gpu
@pytest.mark.parametrize("case", ["grid", "point_to_point", "source_total"])
def test_other_loops_keep_their_launches(case, pair1300):
    """What m3d_debug_icp_nn_terms reports for loops the path does not apply to: 0 with the
    switch on."""
    src, tgt, nrm = pair1300
    kw = dict(relative_fitness=-1, relative_rmse=-1, max_iteration=3)
    if case == "grid":
        lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, nn="grid", **kw)
    elif case == "point_to_point":
        lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, nn="brute", estimation=_lib.EST_POINT_TO_POINT, **kw)
    else:
        lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), R, nn="brute", **kw)
        assert _switch(lp, 1) == 1
        lp.set_source_total(2 * len(src))
    assert _switch(lp, 1) == 0
