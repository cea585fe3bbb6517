#!/usr/bin/env python3
"""CPU model of the brute-force NN's slice plan (nn_plan.h, EXPERIMENTS §R19) on
the cfg1 pair, with tools/nn_cull_model.py's helpers (Morton rows, point test): per 512-query block
the surviving tiles at the bounds r², 0.06² and 0.03², and the distribution over the launched
blocks — tiles kept, half tiles swept by the slowest wave; mean / p90 / p99 / max — under the
uniform launch (S = 1, S = 2) and under the plan rule
  S_x = clamp(ceil(t_x / tau), 1, min(S_max, ntiles)), tau the smallest with sum S_x <= B,
sized from the same bound's counts (the previous evaluation's: the counts barely move) and, the
stale case, from the unseeded r² counts applied to a tighter bound.  numpy only, no GPU.
Usage: python tools/nn_plan_model.py [budget] [smax] [--counts FILE.json]  (FILE: the counts per
bound, the fixture of tests/test_nn_plan_rule.py)"""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
from nn_cull_model import R, boxes, dist, order_morton, synth, wave_half_masks  # noqa: E402


def plan(t, budget, smax, ntiles):
    """nn_plan.h plan_host: S per query block and tau."""
    t = np.minimum(np.asarray(t, np.int64), 1 << 20)
    cap = max(1, min(smax, ntiles, 255))
    S = lambda tau: np.clip(-(-t // tau), 1, cap)
    lo, hi = 1, max(int(t.max()), 1)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if S(mid).sum() <= budget:
            hi = mid
        else:
            lo = mid + 1
    return S(lo), lo


def launched(keep_bt, slow_bt, S):
    """tiles kept and slowest-wave half tiles of every launched block (x, y < S_x)."""
    tiles, slow = [], []
    for x, s in enumerate(S):
        for y in range(s):
            tiles.append(keep_bt[x, y::s].sum())
            slow.append(slow_bt[x, y::s].sum())
    return np.array(tiles), np.array(slow)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    budget = int(args[0]) if len(args) > 0 else 512
    smax = int(args[1]) if len(args) > 1 else 8
    n = 100_000
    src, tgt, _, _ = synth.icp_pair(n, n, seed=0)
    q = src[order_morton(src)]
    t = tgt[order_morton(tgt)]
    hlo, hhi = boxes(t, 256)
    nb = -(-n // 512)
    print(f"cfg1 plan model: {nb} query blocks, budget {budget}, S_max {smax}; distributions: mean p90 p99 max")
    model, counts = {}, {}
    for bound, bname in ((R * R, "r^2"), (0.06 ** 2, "0.06^2"), (0.03 ** 2, "0.03^2")):
        kw = wave_half_masks(q, hlo, hhi, bound, True)
        nt = kw.shape[1] // 4
        kwt = kw.reshape(nb, 8, nt, 4)
        keep_bt = kwt.any(axis=(1, 3))
        slow_bt = kwt.sum(axis=3).max(axis=1) * keep_bt
        model[bname] = (keep_bt, slow_bt, nt)
        counts[bname] = keep_bt.sum(axis=1)
        print(f"bound {bname}: tiles kept per query block: {dist(counts[bname])}")
    for bname, (keep_bt, slow_bt, nt) in model.items():
        print(f"bound {bname}:")
        rows = [("uniform S = 1", np.full(nb, 1)), ("uniform S = 2", np.full(nb, 2))]
        S, tau = plan(counts[bname], budget, smax, nt)
        rows.append((f"plan, own counts (tau {tau})", S))
        if bname != "r^2":
            S0, tau0 = plan(counts["r^2"], budget, smax, nt)
            rows.append((f"plan, stale r^2 counts (tau {tau0})", S0))
        for name, Sx in rows:
            tiles, slow = launched(keep_bt, slow_bt, Sx)
            hist = " ".join(f"{k}:{v}" for k, v in zip(*np.unique(Sx, return_counts=True)))
            print(f"  {name:34s} blocks {len(tiles):4d} | S histogram {hist:28s} | tiles per block {dist(tiles)} | "
                  f"slowest-wave halves {dist(slow)}")
    if "--counts" in sys.argv:
        path = sys.argv[sys.argv.index("--counts") + 1]
        Path(path).write_text(json.dumps({k: v.tolist() for k, v in counts.items()}) + "\n")


if __name__ == "__main__":
    main()
