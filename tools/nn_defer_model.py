#!/usr/bin/env python3
"""CPU model of nn_mfma_kernel's deferred exact passes (docs/EXPERIMENTS.md §R12) on
the cfg1 pair: how much of the work of "every lane pushes all 16 of its rows of every flagged
sub-tile" the result needs, i.e. how many rows the MFMA screen can flag for a lane's own query.

Model: synth.icp_pair(100000, 100000, seed=0) at the converged transform (the true one); queries
in Morton order of their cells, 64 to a wave in two 32-query groups (column c = position in the
group); target rows in Morton order of the grid's cells (build_mfma_tiles), 32 rows to a sub-tile,
row r of a sub-tile in lane half (r >> 2) & 1.  A query's search bound is X = band_of(d_nn²) of
its nearest target (a seeded evaluation late in the loop), the screen flags every target with
d² ≤ X + eps, eps = the MFMA screen's error bound (refresh_rt32's screen_eps_m, the same formulas
in numpy; the threshold's own share, thr_operand, is smaller by orders of magnitude and left out).
A (group, sub-tile) pair is flagged if any of the group's 32 queries has a candidate in the
sub-tile.  Each distribution: mean p50 p90 p99 max.  numpy + scipy only, no GPU.
Usage: python tools/nn_defer_model.py [n]"""
import sys
from pathlib import Path

import numpy as np
from scipy.spatial import cKDTree

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
from m3d import synth  # noqa: E402

R = 0.12
CELL = R * 1.001
U32, U64 = 2.0 ** -24, 2.0 ** -53


def morton_order(p):
    c = np.floor((p - p.min(axis=0)) / CELL).astype(np.int64)
    key = np.zeros(len(p), np.int64)
    for b in range(10):
        for a in range(3):
            key |= ((c[:, a] >> b) & 1) << (3 * b + a)
    cell_order = np.lexsort((np.arange(len(p)), c[:, 0], c[:, 1], c[:, 2]))
    return cell_order[np.argsort(key[cell_order], kind="stable")]


def bounds(q, t):
    """(band_e, r2_hi, screen_eps_m) by refresh_rt32's formulas for centred queries q (already
    transformed: R = I, t' = 0 in the model's frame) and centred targets t."""
    pinf, qinf = np.abs(q).max(), np.abs(t).max()
    rowl1, tinf = 1.0, 0.0
    s3 = np.sqrt(3.0)
    E = 1.01 * U32 * (5.0 * rowl1 * pinf + 4.0 * tinf + qinf) + 8.0 * U64 * s3 * 52 * (pinf + qinf) + 1e-11
    eq = s3 * E * 1.01
    r2_hi = R * R + 2.0 * (3.0 * U32 * (R + s3 * E) ** 2 + 2.0 * s3 * E * R + 3.0 * E * E)
    Q = rowl1 * pinf + tinf
    S = 2.0 ** -np.frexp(np.linalg.norm(t, axis=1).max() / 32.0)[1]
    As, Ts = 2.0 * Q * S, qinf * S
    Ws, P = 3.0 * Ts * Ts, 3.0 * As * Ts
    u16, sig = 2.0 ** -11, 2.0 ** -25
    esplit = 3.0 * u16 * u16 * P + 12.0 * sig * (As + Ts) + u16 * u16 * Ws + 2.0 * sig
    eacc = 32.0 * U32 * 1.01 * (P + Ws)
    e1m = 1.05 * (esplit + eacc) / (S * S) + U32 * 3.0 * qinf * qinf
    return 2.0 * eq * 1.01, r2_hi, 2.0 * (e1m + 6.0 * U32 * r2_hi + 12.0 * U32 * Q * Q)


def dist(v):
    v = np.asarray(v, np.float64).ravel()
    return (f"{v.mean():6.2f} {np.median(v):4.0f} {np.percentile(v, 90):4.0f} "
            f"{np.percentile(v, 99):4.0f} {v.max():4.0f}")


def group_max(keys, values):
    """max of `values` per distinct key (keys int64); returns (distinct keys, maxima)"""
    k, inv = np.unique(keys, return_inverse=True)
    m = np.zeros(len(k), values.dtype)
    np.maximum.at(m, inv, values)
    return k, m


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100_000
    src, tgt, _, T = synth.icp_pair(n, n, seed=0)
    centre = tgt.mean(axis=0)
    q = synth.apply(T, src)
    q = q[morton_order(q)] - centre
    t = tgt[morton_order(tgt)] - centre  # row order
    be, r2_hi, eps = bounds(q, t)
    tree = cKDTree(t)
    d_nn, _ = tree.query(q)
    root = d_nn * 1.000004 + be
    X = np.minimum(root * root * 1.000004, r2_hi)
    X = np.where(d_nn * d_nn <= r2_hi, X, r2_hi)  # no seed within the radius: the radius itself
    print(f"cfg1 defer model, n = {n}: screen bound eps = {eps:.3e} (d^2 units), search bound X mean "
          f"{X.mean():.3e} p99 {np.percentile(X, 99):.3e}; each distribution: mean p50 p90 p99 max")
    cand = tree.query_ball_point(q, np.sqrt(X + eps), workers=-1)
    cnt = np.array([len(c) for c in cand])
    print(f"candidates per query (targets the screen may flag): {dist(cnt)}")
    qi = np.repeat(np.arange(len(q)), cnt)
    row = np.concatenate([np.asarray(c, np.int64) for c in cand])
    grp, sub = qi // 32, row // 32          # 32-query group (two to a wave), sub-tile
    half = (row >> 2) & 1                   # the lane of the query's pair that holds the row
    nsub = len(t) // 32 + 1
    pair = grp * nsub + sub                 # (group, sub-tile)
    pairs = np.unique(pair)
    wave_of_pair = pairs // nsub // 2
    nw = -(-len(q) // 64)
    per_wave = np.bincount(wave_of_pair, minlength=nw)
    print(f"flagged (group, sub-tile) pairs per wave:            {dist(per_wave)}")
    rows_hit = np.unique(pair * 32 + row % 32) // 32
    _, rows_per_pair = np.unique(rows_hit, return_counts=True)
    print(f"rows of a flagged pair's 32 that any query hits:     {dist(rows_per_pair)}")
    lane = (pair * 32 + qi % 32) * 2 + half  # (pair, query column, lane half)
    lanes, hits = np.unique(lane, return_counts=True)
    pk, most = group_max(lanes // 64, hits)
    print(f"most hits of any lane among its 16 rows, per pair:   {dist(most)}")
    it_wave = np.bincount(pk // nsub // 2, weights=most, minlength=nw)
    print(f"bit-loop iterations per wave (sum of the above):     {dist(it_wave)}")
    print(f"pushes per lane per wave: all rows {16 * per_wave.mean():.0f}, filtered {it_wave.mean():.1f} "
          f"({16 * per_wave.mean() / it_wave.mean():.1f} x fewer)")


if __name__ == "__main__":
    main()
