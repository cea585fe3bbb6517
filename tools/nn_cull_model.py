#!/usr/bin/env python3
"""CPU model of nn_mfma_kernel's box cull (docs/EXPERIMENTS.md §3.5) on the cfg1
pair: which (512-query block, 1024-target tile) and (64-query wave, 256-target half tile) pairs
survive the test  box gap² > bound, and how many half tiles the slowest wave of a block sweeps (the
8 waves of a block meet at every tile barrier, so that is what the sweep costs the block).

Model: synth.icp_pair(100000, 100000, seed=0), identity transform; targets in the grid's
row-major (z, y, x) cell order or in Morton order of the same cells, cell = 0.12 · 1.001; queries
in Morton order of the same cell size; axis-aligned boxes, squared Euclidean box gap against the
bound r² (unseeded first evaluation) or 0.06² (a typical seeded bound).  numpy only, no GPU.
Usage: python tools/nn_cull_model.py [n]"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
from m3d import synth  # noqa: E402

R = 0.12
CELL = R * 1.001


def _cells(p):
    return np.floor((p - p.min(axis=0)) / CELL).astype(np.int64)


def _morton(c):
    key = np.zeros(len(c), np.int64)
    for b in range(10):
        for a in range(3):
            key |= ((c[:, a] >> b) & 1) << (3 * b + a)
    return key


def order_rowmajor(p):
    c = _cells(p)
    return np.lexsort((np.arange(len(p)), c[:, 0], c[:, 1], c[:, 2]))


def order_morton(p):
    return np.argsort(_morton(_cells(p)), kind="stable")


def boxes(p, size):
    """(lo, hi) of consecutive groups of `size` rows; the ragged last group is padded with its own
    last point (pads are left out of a box)."""
    n = -(-len(p) // size) * size
    q = np.vstack([p, np.repeat(p[-1:], n - len(p), axis=0)]).reshape(-1, size, 3)
    return q.min(axis=1), q.max(axis=1)


def gap2(qlo, qhi, tlo, thi):
    g = np.maximum(0.0, np.maximum(qlo[:, None, :] - thi[None, :, :], tlo[None, :, :] - qhi[:, None, :]))
    return (g * g).sum(axis=2)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    src, tgt, _, T = synth.icp_pair(n, n, seed=0)
    q = src[order_morton(src)]  # identity transform: the first evaluation's queries
    print(f"cfg1 model, n = {n}: bound, target order, (block, tile) pairs kept, (wave, half) pairs kept, "
          f"half tiles swept by the slowest wave of a block (mean over blocks) of the total")
    for bound, bname in ((R * R, "r^2"), (0.06 * 0.06, "0.06^2")):
        for oname, order in (("row-major", order_rowmajor), ("Morton", order_morton)):
            t = tgt[order(tgt)]
            blo, bhi = boxes(q, 512)
            wlo, whi = boxes(q, 64)
            tlo, thi = boxes(t, 1024)
            hlo, hhi = boxes(t, 256)
            keep_bt = gap2(blo, bhi, tlo, thi) <= bound
            keep_wh = gap2(wlo, whi, hlo, hhi) <= bound
            nb, nh = len(blo), 4 * len(tlo)  # all-pad halves and absent waves: never swept
            nw = -(-len(wlo) // 8) * 8
            kw = np.zeros((nw, nh), bool)
            kw[:len(wlo), :len(hlo)] = keep_wh
            # a wave sweeps a half only inside a tile its block keeps (always true when the wave
            # reaches it: the wave's box lies inside the block's); per tile the block waits for the
            # wave that sweeps most of its halves
            per_tile = kw.reshape(nb, 8, -1, 4).sum(axis=3).max(axis=1)  # (block, tile): halves of the slowest wave
            slow = per_tile.sum(axis=1)
            print(f"  {bname:7s} {oname:9s}  {100 * keep_bt.mean():5.1f} %   {100 * keep_wh.mean():5.1f} %   "
                  f"{slow.mean():6.1f} of {nh}")


if __name__ == "__main__":
    main()
