"""Per-evaluation time of Generalized ICP (m3d_gicp_run) beside the point-to-plane loop it is
built from, on the benchmark's seeded 100k <-> 100k pair (m3d.synth.icp_pair, seed 0, r = 0.12)
with the grid NN.

* Whole calls, HIP events around each: m3d_gicp_run and m3d_icp_run (point-to-plane) with
  max_iteration = N and 0 and convergence thresholds that never fire, so a call runs exactly
  N + 1 and 1 evaluations; per evaluation = (t(N) - t(0)) / N, the set-up of a call (grids, Morton
  copy, covariances) cancelling.  The two estimators alternate; median and min..max over --repeats.
* The yardstick of DESIGN section 6: the step-wise point-to-plane grid loop (IcpLoop.steps, a
  replayed HIP graph), events around --iters iterations.
* Kernel events of the library (m3d_profile_*), in a pass of their own: the NN scan and the terms
  launch(es) per evaluation — for Generalized ICP the plane-to-plane pass plus its reduce — and
  the achieved bytes/s of that pass against the 232 B per source it must move (gicp.hip).
* The one-evaluation call (m3d_gicp_terms) at 1,000 sources of the same pair, host-bound at that
  size: whole warm calls, median and min..max over 20 x --repeats.

AB_LIB=<libm3d.so of another build> times that build instead.
Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/gicp_timing.py [--ns 100000] [--iters 30] [--repeats 15] [--warmup 3]"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import numpy as np
import torch

from m3d import _lib, synth

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d.core import Cloud, IcpLoop, context, gicp, gicp_terms, icp

BYTES_PER_SOURCE = 232  # gicp.hip: point and covariance read + written, key, runner-up, corr, gathered target


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3, out  # µs


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    ns, N, r = args.ns, args.iters, 0.12
    src, tgt, tn, T = synth.icp_pair(ns, ns, seed=0)
    _, sn_world = synth.surface_points(ns, 100)  # icp_pair's source sampling: its normals, moved as it was
    sn = np.ascontiguousarray(sn_world @ np.linalg.inv(T)[:3, :3].T)
    s, t = Cloud(src, sn), Cloud(tgt, tn)
    kw = dict(relative_fitness=-1.0, relative_rmse=-1.0, with_correspondences=False, nn="grid")
    calls = {
        "gicp": lambda n: gicp(s, t, r, np.eye(4), max_iteration=n, **kw),
        "point_to_plane": lambda n: icp(s, t, r, np.eye(4), max_iteration=n, **kw),
    }
    per_eval = {k: [] for k in calls}
    for rep in range(args.warmup + args.repeats):
        for name, fn in calls.items():
            t0, _ = timed(lambda: fn(0))
            tN, out = timed(lambda: fn(N))
            assert out.iterations == N, (name, out.iterations)
            if rep >= args.warmup:
                per_eval[name].append((tN - t0) / N)
    res = {"ns": ns, "iters": N, "radius": r, "per_evaluation": {k: spread(v) for k, v in per_eval.items()}}
    g, p = res["per_evaluation"]["gicp"], res["per_evaluation"]["point_to_plane"]
    res["ratio_gicp_over_point_to_plane"] = g["median_us"] / p["median_us"]
    # the step-wise point-to-plane grid loop (DESIGN section 6's figure)
    lp = IcpLoop(s, t, r, relative_fitness=-1, relative_rmse=-1, max_iteration=10 ** 6, nn="grid")
    steps = []
    for rep in range(args.warmup + args.repeats):
        lp.reset(np.eye(4))
        lp.steps(1)  # the unseeded first evaluation stays outside, as in bench.py's amortised figure
        us, _ = timed(lambda: lp.steps(N))
        if rep >= args.warmup:
            steps.append(us / N)
    res["point_to_plane_step_loop"] = spread(steps)
    # the one-evaluation call at a size where the host's part of it dominates
    s1k, t1k = Cloud(src[:1000], sn[:1000]), Cloud(tgt[:1000], tn[:1000])
    one = []
    for rep in range(20 * (args.warmup + args.repeats)):
        us, _ = timed(lambda: gicp_terms(s1k, t1k, np.eye(4), r, with_correspondences=False))
        if rep >= 20 * args.warmup:
            one.append(us)
    res["gicp_terms_call_ns1000"] = spread(one)
    # kernel events, in a pass of their own
    kern = {}
    for name, fn in calls.items():
        fn(N)
        ctx.profile(True)
        ctx.profile_read(_lib.KERNEL_NN), ctx.profile_read(_lib.KERNEL_TERMS)
        for _ in range(3):
            fn(N)
        nn_ms, nn_n = ctx.profile_read(_lib.KERNEL_NN)
        t_ms, t_n = ctx.profile_read(_lib.KERNEL_TERMS)
        ctx.profile(False)
        kern[name] = {"nn_us": nn_ms / max(nn_n, 1) * 1e3, "terms_us": t_ms / max(t_n, 1) * 1e3,
                      "launches": int(t_n)}
    res["kernel_events"] = kern
    tu = kern["gicp"]["terms_us"]
    res["gicp_terms_bytes"] = BYTES_PER_SOURCE * ns
    res["gicp_terms_achieved_GBs"] = BYTES_PER_SOURCE * ns / (tu * 1e-6) / 1e9 if tu > 0 else None
    for k, v in res["per_evaluation"].items():
        print(f"{k:>15}: {v['median_us']:8.1f} us per evaluation (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
              f"n {v['n']})")
    v = res["point_to_plane_step_loop"]
    print(f"step-wise point-to-plane loop: {v['median_us']:.1f} us per iteration (min {v['min_us']:.1f}, "
          f"max {v['max_us']:.1f})")
    v = res["gicp_terms_call_ns1000"]
    print(f"m3d_gicp_terms at ns = 1000: {v['median_us']:.1f} us per call (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
          f"n {v['n']})")
    print(f"ratio gicp / point-to-plane per evaluation: {res['ratio_gicp_over_point_to_plane']:.2f}")
    for k, v in kern.items():
        print(f"{k:>15} kernel events: NN scan {v['nn_us']:.1f} us, terms launch {v['terms_us']:.1f} us "
              f"({v['launches']} launches)")
    print(f"gicp terms pass + reduce: {BYTES_PER_SOURCE * ns / 1e6:.1f} MB in {tu:.1f} us = "
          f"{res['gicp_terms_achieved_GBs']:.0f} GB/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
