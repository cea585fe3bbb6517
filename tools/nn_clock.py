"""Per-block timeline of the last nn_mfma_kernel launch (diagnostic build: tools/ab_build.sh nnclk
-DM3D_NN_CLOCK=1 [-DM3D_NN_REACH=0], then AB_LIB=tools/ab/nnclk.so python tools/nn_clock.py [evals]).
cfg1 pair, brute force; the launch looked at is the last of `evals` evaluations (default 20).  Per
block the build records s_memrealtime (100 MHz, 10 ns) at entry, after the setup (queries, seeds,
boxes, first cull round, first tile staged), after the tile loop and at the exit of its last wave,
and when its last wave out finished the deferred exact passes, with the tiles the block kept and the
half tiles its slowest wave swept, and its slice: query block x, slice y and — since the
slice plan (nn_plan.h, EXPERIMENTS §R19) — the query block's slice count S (x | y << 32 | S << 48;
a build from before the plan leaves S at 0: grid.y).  With the plan it prints the S histogram and
the block durations against S.  M3D_NN_PLAN=0 in the environment: the uniform launch.
Where the launch is nn_mfma_terms_kernel (the terms pass inside the NN launch) the
record has two more words — the return of the block's hand-off ticket and, for the block that ran
its query block's terms pass, the end of that pass — and the tool prints how many query blocks had
finished their terms before the launch's last scan ended, and how long the launch runs past that
point.  A build from before those words (8 per record) is read as such."""
import ctypes as C
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import numpy as np
import torch

from m3d import _lib, synth

_lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d.core import Cloud, IcpLoop, context

CLK_BLOCKS, CLK_WORDS = 16384, 10  # nn_brute.hip kClkBlocks, kClkWords (8 before the hand-off's stamps)


def stats(v):
    return (f"mean {v.mean():.2f} p50 {np.median(v):.2f} p90 {np.percentile(v, 90):.2f} "
            f"p99 {np.percentile(v, 99):.2f} max {v.max():.2f}")


def main():
    evals = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    torch.cuda.set_device(0)
    ctx = context()
    n = 100_000
    src, tgt, nrm, _ = synth.icp_pair(n, n, seed=0)
    lp = IcpLoop(Cloud(src), Cloud(tgt, nrm), 0.12, relative_fitness=-1, relative_rmse=-1,
                 max_iteration=evals, nn="brute")
    lp.reset(np.eye(4))
    for _ in range(evals):  # single steps: every evaluation is a launch of its own
        lp.step()
    torch.cuda.synchronize()
    for words in (CLK_WORDS, 8):
        buf = (C.c_ulonglong * (words * CLK_BLOCKS))()
        rc = ctx.lib.m3d_debug_nn_clock(buf, C.c_int(words * CLK_BLOCKS))
        if rc == 0:
            break
    assert rc == 0, "m3d_debug_nn_clock failed"
    a = np.frombuffer(buf, dtype=np.uint64).reshape(-1, words).astype(np.int64)
    if words == 8:
        a = np.column_stack([a, np.zeros((len(a), 2), np.int64)])
    a = a[a[:, 3] > 0]
    bx, by, bs = a[:, 6] & 0xFFFFFFFF, (a[:, 6] >> 32) & 0xFFFF, a[:, 6] >> 48
    gx, gy = int(bx.max()) + 1, int(by.max()) + 1
    bs = np.where(bs > 0, bs, gy)
    us = 10e-3
    t0 = a[:, 0].min()
    st, en = (a[:, 0] - t0) * us, (a[:, 3] - t0) * us
    setup, loop, rest = (a[:, 1] - a[:, 0]) * us, (a[:, 2] - a[:, 1]) * us, (a[:, 3] - a[:, 2]) * us
    # (the deferred passes' end is the stamp of the block's last wave out, the exit the latest of all)
    defer, publish = (a[:, 7] - a[:, 2]) * us, (a[:, 3] - a[:, 7]) * us
    du = en - st
    tiles, slow = a[:, 4], a[:, 5]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    slots = 2 * cus  # two resident blocks per CU
    print(f"evaluation {evals} of cfg1: grid {gx} x {gy} = {len(a)} blocks recorded, {slots} resident slots; "
          f"launch span {en.max():.2f} us")
    print(f"block duration us: {stats(du)}")
    print(f"  setup          : {stats(setup)}")
    print(f"  tile loop      : {stats(loop)}")
    print(f"  deferred+publish: {stats(rest)}")
    print(f"    deferred passes : {stats(defer)}")
    print(f"    publish         : {stats(publish)}")
    hist, edges = np.histogram(du, bins=12)
    print("durations per bin:", " ".join(f"{e:.1f}:{h}" for e, h in zip(edges[:-1], hist)))
    print(f"tiles kept per block: {stats(tiles.astype(np.float64))}")
    print(f"half tiles swept by the slowest wave: {stats(slow.astype(np.float64))}")
    per_x = np.zeros(gx, np.int64)
    per_x[bx] = bs
    print("slices per query block (S: query blocks):", " ".join(f"{k}:{v}" for k, v in zip(*np.unique(per_x, return_counts=True))))
    print("duration against S (S: blocks, mean tiles, mean duration, p99, max):")
    for k in np.unique(bs):
        m = bs == k
        print(f"  {k:3d}: {m.sum():4d}  {tiles[m].mean():5.2f}  {du[m].mean():6.2f}  {np.percentile(du[m], 99):6.2f}  {du[m].max():6.2f}")
    print("duration against tiles kept (tiles: blocks, mean duration, mean tile loop, max duration):")
    for k in np.unique(tiles):
        m = tiles == k
        print(f"  {k:3d}: {m.sum():4d}  {du[m].mean():6.2f}  {loop[m].mean():6.2f}  {du[m].max():6.2f}")
    nz = tiles > 0
    if nz.sum() > 1:
        A = np.column_stack([np.ones(nz.sum()), tiles[nz], slow[nz]])
        coef = np.linalg.lstsq(A, loop[nz], rcond=None)[0]
        print(f"tile loop ~ {coef[0]:.2f} + {coef[1]:.2f} us per tile + {coef[2]:.2f} us per slowest-wave half tile")
    order = np.argsort(st, kind="stable")
    first = order[:slots]
    late = order[slots:]
    print(f"first round ({len(first)} earliest blocks): last start {st[first].max():.2f}, ends {stats(en[first])}")
    if len(late):
        print(f"later blocks ({len(late)}): starts {stats(st[late])}; ends {stats(en[late])}")
    k = int(np.argmax(en))
    print(f"the launch ends with block ({bx[k]}, {by[k]}) of S = {bs[k]}: start {st[k]:.2f}, duration {du[k]:.2f} "
          f"(setup {setup[k]:.2f}, loop {loop[k]:.2f}, rest {rest[k]:.2f}), tiles {tiles[k]}, slowest wave {slow[k]} halves")
    hist, edges = np.histogram(en, bins=12)
    print("ends per bin:  ", " ".join(f"{e:.1f}:{h}" for e, h in zip(edges[:-1], hist)))
    if (a[:, 8] > 0).any():  # nn_mfma_terms_kernel: the hand-off and the in-kernel terms
        tick, tend = (a[:, 8] - t0) * us, (a[:, 9] - t0) * us
        ran = a[:, 9] > 0
        last_scan = en.max()  # (en: the blocks' publish done, before the hand-off)
        launch_end = max(tick.max(), tend[ran].max())
        print(f"hand-off: ticket back {stats(tick - en)} us after the block's publish")
        print(f"in-kernel terms ({ran.sum()} query blocks): duration {stats(tend[ran] - tick[ran])}; "
              f"ends {stats(tend[ran])}")
        print(f"{(tend[ran] <= last_scan).sum()} of {ran.sum()} query blocks finished their terms before the "
              f"launch's last scan ended ({last_scan:.2f} us); the launch runs {launch_end - last_scan:.2f} us past it "
              f"(to {launch_end:.2f} us)")


if __name__ == "__main__":
    main()
