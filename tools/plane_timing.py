"""Time of plane segmentation (m3d_segment_plane) on a generated scan — 55 % of the points on a
4 x 4 table patch with N(0, 0.004) out-of-plane noise, 35 % in a 1.0 x 0.6 x 0.4 box above it,
10 % uniform strays in +-3 — at 180k points x 100 iterations and 1M x 1000.

* Whole calls, HIP events around each (the cloud is on the device already): the default
  probability (the loop stops early, as a caller's does) and probability = 1 (every iteration is
  scored).  Median and min..max over --repeats after --warmup.
* Kernel events of the library (m3d_profile_*), in a pass of their own, the probability = 1 call:
  fit, score, reduce + scan, inlier flags + select, refit.
* The score kernel's achieved fp64 rate: 8 fp64 operations per (point, hypothesis) — three
  multiplies and three adds of the distance, its square, the masked add — against the fp64 vector
  peak.  MI355X_MICROARCH tabulates the fp32 vector peak (157.3 TFLOPS, 64 FLOP/clk/SIMD); the fp64
  vector rate is half of it, 78.6 TFLOPS (AMD's published figure), counted with a fused
  multiply-add as two operations.  This kernel may not fuse (each operation is rounded on its own),
  so separate multiplies and adds can reach half of that peak at most.

Needs the GPU; prints readable lines and one JSON line.  AB_LIB=tools/ab/NAME.so times another
build of the library.
Usage: python tools/plane_timing.py [--repeats 15] [--warmup 3] [--small-only]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import os

import numpy as np
import torch

from m3d import _lib, prep

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d.core import Cloud, context

FP64_VECTOR_PEAK = 78.6e12  # half the fp32 vector peak of MI355X_MICROARCH.md (FMA = 2)
OPS_PER_EVAL = 8            # fp64 operations of plane_score_kernel per (point, hypothesis)
THR = 0.012


def scan(n, seed=0):
    rng = np.random.default_rng(seed)
    n_pl, n_ob = int(0.55 * n), int(0.35 * n)
    pl = np.column_stack([rng.uniform(-2, 2, n_pl), rng.uniform(-2, 2, n_pl), rng.normal(0.0, 0.004, n_pl)])
    ob = np.column_stack([rng.uniform(-0.5, 0.5, n_ob), rng.uniform(-0.3, 0.3, n_ob), rng.uniform(0.02, 0.42, n_ob)])
    st = rng.uniform(-3, 3, (n - n_pl - n_ob, 3))
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return (np.vstack([pl, ob, st]) @ Q.T)[rng.permutation(n)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out  # µs


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


def one_config(ctx, n, iters, repeats, warmup):
    cloud = Cloud(scan(n))
    calls = {
        "default_probability": lambda: prep.segment_plane(cloud, THR, 3, iters, seed=7, with_details=True),
        "probability_1": lambda: prep.segment_plane(cloud, THR, 3, iters, 1.0, seed=7, with_details=True),
    }
    res = {"n": n, "num_iterations": iters, "calls": {}}
    for name, fn in calls.items():
        us = []
        for rep in range(warmup + repeats):
            t, (plane, inl, out) = timed(fn)
            if rep >= warmup:
                us.append(t)
        res["calls"][name] = dict(spread(us), iterations=out.iterations, evaluated=out.evaluated,
                                  inliers=int(len(inl)), best_count=out.best_count)
    # kernel events, in a pass of their own: every iteration scored
    fn = calls["probability_1"]
    ids = {"fit": _lib.KERNEL_KABSCH, "score": _lib.KERNEL_SCORE, "reduce_scan": _lib.KERNEL_LOOP,
           "inliers": _lib.KERNEL_NN, "refit": _lib.KERNEL_TERMS}
    fn()
    ctx.profile(True)
    for k in ids.values():
        ctx.profile_read(k)
    reps = 3
    for _ in range(reps):
        fn()
    kern = {}
    for name, k in ids.items():
        ms, cnt = ctx.profile_read(k)
        kern[name] = {"us_per_call": ms * 1e3 / reps, "launches_per_call": cnt / reps}
    ctx.profile(False)
    res["kernel_events"] = kern
    s_us = kern["score"]["us_per_call"]
    ops = OPS_PER_EVAL * float(n) * iters
    res["score_fp64_ops"] = ops
    res["score_achieved_Tops"] = ops / (s_us * 1e-6) / 1e12 if s_us > 0 else None
    res["score_fraction_of_fp64_vector_peak"] = ops / (s_us * 1e-6) / FP64_VECTOR_PEAK if s_us > 0 else None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-only", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    configs = [(180_000, 100)] + ([] if args.small_only else [(1_000_000, 1000)])
    out = {"threshold": THR, "fp64_vector_peak": FP64_VECTOR_PEAK, "configs": []}
    for n, iters in configs:
        r = one_config(ctx, n, iters, args.repeats, args.warmup)
        out["configs"].append(r)
        print(f"n = {n}, num_iterations = {iters}")
        for name, v in r["calls"].items():
            print(f"  {name:>20}: {v['median_us']:9.1f} us per call (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
                  f"n {v['n']}); left at h = {v['iterations']}, {v['evaluated']} evaluated, {v['inliers']} inliers")
        for name, v in r["kernel_events"].items():
            print(f"  {name:>20}: {v['us_per_call']:9.1f} us per call in {v['launches_per_call']:.0f} launches "
                  "(probability 1)")
        print(f"  score kernel: {r['score_fp64_ops']:.3g} fp64 operations -> {r['score_achieved_Tops']:.2f} T/s = "
              f"{100 * r['score_fraction_of_fp64_vector_peak']:.1f} % of the {FP64_VECTOR_PEAK / 1e12:.1f} TFLOPS "
              "fp64 vector peak")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
