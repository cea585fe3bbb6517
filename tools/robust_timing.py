"""Per-evaluation time of the robust-kernel loops (m3d_robust_icp_run, m3d_gicp_run_robust; Tukey)
beside the same calls with kernel=None (m3d_icp_run's fused point-to-plane tail, m3d_gicp_run), on
the benchmark's seeded 100k <-> 100k pair (m3d.synth.icp_pair, seed 0, r = 0.12) with the grid NN.

* Whole calls, HIP events around each, as tools/gicp_timing.py: max_iteration = N and 0 with
  convergence thresholds that never fire; per evaluation = (t(N) - t(0)) / N, the set-up of a call
  cancelling.  The four calls alternate; median and min..max over --repeats.
* Kernel events of the library (m3d_profile_*), in a pass of their own: the NN scan and the terms
  launches per evaluation, and the achieved bytes/s of the robust passes against the 112 B
  (point-to-plane) and 232 B (Generalized ICP) per source they must move (robust.hip).
* The eigendecomposition's share of the robust Generalized ICP pass, as an upper bound: that pass
  and gicp.hip's move the same bytes, so (robust - unweighted) / robust is what W = M^(-1/2)
  (Jacobi sweeps, three 1/sqrt) and three weighted rows instead of one M^-1 system cost together.

AB_LIB=<libm3d.so of another build> times that build instead.
Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/robust_timing.py [--ns 100000] [--iters 30] [--repeats 15] [--warmup 3]"""
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
from m3d.core import Cloud, context, gicp, icp
from matcher.robust import TukeyLoss

BYTES = {"robust_plane": 112, "robust_gicp": 232}  # robust.hip: bytes per source a pass must move


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
    # scales of a few residual σ of this pair: most rows keep a weight between 0 and 1
    k_plane, k_gicp = TukeyLoss(0.05), TukeyLoss(1.0)
    calls = {
        "robust_plane": lambda n: icp(s, t, r, np.eye(4), max_iteration=n, kernel=k_plane, **kw),
        "plane": lambda n: icp(s, t, r, np.eye(4), max_iteration=n, **kw),
        "robust_gicp": lambda n: gicp(s, t, r, np.eye(4), max_iteration=n, kernel=k_gicp, **kw),
        "gicp": lambda n: gicp(s, t, r, np.eye(4), max_iteration=n, **kw),
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
    pe = {k: v["median_us"] for k, v in res["per_evaluation"].items()}
    res["ratio_robust_plane_over_plane"] = pe["robust_plane"] / pe["plane"]
    res["ratio_robust_gicp_over_gicp"] = pe["robust_gicp"] / pe["gicp"]
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
    for name, b in BYTES.items():
        tu = kern[name]["terms_us"]
        res[f"{name}_terms_achieved_GBs"] = b * ns / (tu * 1e-6) / 1e9 if tu > 0 else None
    rg, g = kern["robust_gicp"]["terms_us"], kern["gicp"]["terms_us"]
    res["eigen_and_rows_share_of_robust_gicp_pass"] = (rg - g) / rg if rg > 0 else None
    for k, v in res["per_evaluation"].items():
        print(f"{k:>13}: {v['median_us']:8.1f} us per evaluation (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
              f"n {v['n']})")
    print(f"ratio robust / kernel=None per evaluation: point-to-plane {res['ratio_robust_plane_over_plane']:.2f}, "
          f"Generalized ICP {res['ratio_robust_gicp_over_gicp']:.2f}")
    for k, v in kern.items():
        print(f"{k:>13} kernel events: NN scan {v['nn_us']:.1f} us, terms launch {v['terms_us']:.1f} us "
              f"({v['launches']} launches)")
    for name, b in BYTES.items():
        print(f"{name} terms pass + reduce: {b * ns / 1e6:.1f} MB in {kern[name]['terms_us']:.1f} us = "
              f"{res[f'{name}_terms_achieved_GBs']:.0f} GB/s")
    print(f"W = M^(-1/2) and the three weighted rows: at most {100 * res['eigen_and_rows_share_of_robust_gicp_pass']:.0f} % "
          f"of the robust Generalized ICP pass ({rg:.1f} us against {g:.1f} us unweighted)")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
