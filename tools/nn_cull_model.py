#!/usr/bin/env python3
"""CPU model of nn_mfma_kernel's cull (docs/EXPERIMENTS.md §3.5, §R10) on the cfg1
pair: which (512-query block, 1024-target tile) and (64-query wave, 256-target half tile) pairs
survive, and how the survivors are distributed over the launched blocks — a launch ends with its
slowest blocks, so the tail counts, not the mean.

Two tests: box-vs-box (box gap² > bound, box_out_of_reach) and, behind it, point-vs-box
(point_out_of_reach: a wave keeps a half tile only if one of its queries is within the bound of the
half's box, a block keeps a tile only if one of its waves keeps one of its halves).  Per launched
block (query block × grid.y slice of every grid.y-th tile): the tiles kept (a DMA and a barrier
each) and the half tiles swept by the slowest wave (the 8 waves meet at every tile barrier); per
64-query wave: the half tiles kept over the whole target.  mean / p90 / p99 / max.

Model: synth.icp_pair(100000, 100000, seed=0), identity transform; targets in the grid's
row-major (z, y, x) cell order, in Morton order or in Hilbert order (Skilling's transform) of the
same cells, cell = 0.12 · 1.001; queries in Morton order of the same cell size; axis-aligned boxes,
squared Euclidean gap against the bound r² (unseeded first evaluation) or 0.06² (a typical seeded
bound; the kernel's bound is per query and tighter still late in a loop).  numpy only, no GPU.
Usage: python tools/nn_cull_model.py [n] [grid_y]"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
from m3d import synth  # noqa: E402

R = 0.12
CELL = R * 1.001
BITS = 10


def _cells(p):
    return np.floor((p - p.min(axis=0)) / CELL).astype(np.int64)


def _morton(c):
    key = np.zeros(len(c), np.int64)
    for b in range(BITS):
        for a in range(3):
            key |= ((c[:, a] >> b) & 1) << (3 * b + a)
    return key


def hilbert_key(c, bits=BITS):
    """3-D Hilbert index of integer cell coordinates (n, 3) with `bits` bits per axis: Skilling's
    axes-to-transpose transform (J. Skilling, Programming the Hilbert curve, 2004), then the
    transposed bits interleaved, axis 0 most significant."""
    x = [c[:, a].astype(np.int64).copy() for a in range(3)]
    m = 1 << (bits - 1)
    q = m
    while q > 1:  # inverse undo
        p = q - 1
        for i in range(3):
            hit = (x[i] & q) != 0
            x[0] = np.where(hit, x[0] ^ p, x[0])
            t = np.where(hit, 0, (x[0] ^ x[i]) & p)
            x[0] ^= t
            x[i] ^= t
        q >>= 1
    for i in range(1, 3):  # Gray encode
        x[i] ^= x[i - 1]
    t = np.zeros_like(x[0])
    q = m
    while q > 1:
        t = np.where((x[2] & q) != 0, t ^ (q - 1), t)
        q >>= 1
    for i in range(3):
        x[i] ^= t
    key = np.zeros(len(c), np.int64)
    for b in range(bits):
        for a in range(3):
            key |= ((x[a] >> b) & 1) << (3 * b + (2 - a))
    return key


def order_rowmajor(p):
    c = _cells(p)
    return np.lexsort((np.arange(len(p)), c[:, 0], c[:, 1], c[:, 2]))


def order_morton(p):
    return np.argsort(_morton(_cells(p)), kind="stable")


def order_hilbert(p):
    return np.argsort(hilbert_key(_cells(p)), kind="stable")


def boxes(p, size):
    """(lo, hi) of consecutive groups of `size` rows; the ragged last group is padded with its own
    last point (pads are left out of a box)."""
    n = -(-len(p) // size) * size
    q = np.vstack([p, np.repeat(p[-1:], n - len(p), axis=0)]).reshape(-1, size, 3)
    return q.min(axis=1), q.max(axis=1)


def gap2(qlo, qhi, tlo, thi):
    g = np.maximum(0.0, np.maximum(qlo[:, None, :] - thi[None, :, :], tlo[None, :, :] - qhi[:, None, :]))
    return (g * g).sum(axis=2)


def dist(v):
    v = np.asarray(v, np.float64).ravel()
    return f"{v.mean():5.2f} {np.percentile(v, 90):4.0f} {np.percentile(v, 99):4.0f} {v.max():4.0f}"


def wave_half_masks(q, hlo, hhi, bound, point):
    """(waves padded to whole blocks, halves padded to whole tiles) bool: the half tiles each
    64-query wave keeps by the box test, refined by the point test if `point`."""
    wlo, whi = boxes(q, 64)
    nw, nh = -(-len(wlo) // 8) * 8, -(-len(hlo) // 4) * 4  # absent waves, all-pad halves: never kept
    kw = np.zeros((nw, nh), bool)
    kw[:len(wlo), :len(hlo)] = gap2(wlo, whi, hlo, hhi) <= bound
    if point:
        for w in range(len(wlo)):
            hs = np.nonzero(kw[w])[0]
            pts = q[64 * w:64 * w + 64]
            reach = (gap2(pts, pts, hlo[hs], hhi[hs]) <= bound).any(axis=0)
            kw[w, hs] = reach
    return kw


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    gy = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    src, tgt, _, T = synth.icp_pair(n, n, seed=0)
    q = src[order_morton(src)]  # identity transform: the first evaluation's queries
    print(f"cfg1 model, n = {n}, grid.y = {gy}; each distribution: mean p90 p99 max")
    print("bound   rows      test   | pairs kept: (block, tile) (wave, half) | tiles kept per launched block | "
          "half tiles of the slowest wave per launched block | half tiles kept per wave, whole target")
    for bound, bname in ((R * R, "r^2"), (0.06 * 0.06, "0.06^2")):
        for oname, order in (("row-major", order_rowmajor), ("Morton", order_morton), ("Hilbert", order_hilbert)):
            t = tgt[order(tgt)]
            blo, bhi = boxes(q, 512)
            hlo, hhi = boxes(t, 256)
            nb = len(blo)
            for point in (False, True):
                kw = wave_half_masks(q, hlo, hhi, bound, point)
                nt = kw.shape[1] // 4
                kwt = kw.reshape(nb, 8, nt, 4)
                if point:  # a tile survives if a wave keeps one of its halves
                    keep_bt = kwt.any(axis=(1, 3))
                else:      # ... if the block's box reaches one of its halves
                    kb = np.zeros((nb, 4 * nt), bool)
                    kb[:, :len(hlo)] = gap2(blo, bhi, hlo, hhi) <= bound
                    keep_bt = kb.reshape(nb, nt, 4).any(axis=2)
                slow_bt = kwt.sum(axis=3).max(axis=1) * keep_bt  # (block, tile): halves of the slowest wave
                tiles = np.stack([keep_bt[:, y::gy].sum(axis=1) for y in range(gy)])
                slow = np.stack([slow_bt[:, y::gy].sum(axis=1) for y in range(gy)])
                per_wave = kw[:-(-len(q) // 64)].sum(axis=1)
                print(f"{bname:7s} {oname:9s} {'point' if point else 'box  '}  | {100 * keep_bt.mean():5.1f} % "
                      f"{100 * kw.mean():5.1f} % | {dist(tiles)} | {dist(slow)} | {dist(per_wave)}")


if __name__ == "__main__":
    main()
