"""Times of Colored ICP's two new passes (colored.hip) on the benchmark's seeded 100k <-> 100k pair
(m3d.synth.icp_pair, seed 0, r = 0.12, grid NN) with generated colours (a smooth field of the
position in the target's frame, r != g != b).

1. The gradient pass (m3d_color_gradients, radius 2r, max_nn 30: one wave per target point, the
   neighbour list kept in registers) against m3d_hybrid_search(2r, 30) ALONE on the same cloud:
   the search is the work the gradient pass contains, and the unfused composition (search, the
   N x 30 lists written and read back, then a thread-per-point pass) cannot take less than the
   search.  Both calls write into buffers allocated before the clock starts (no copy to the host),
   HIP events around each, grids cached by the warm-up calls; median and min..max over --repeats.
   The unfused composition itself is not built.
2. The colored terms evaluation against the robust point-to-plane one (m3d_robust_icp_run, Tukey),
   per evaluation = (t(N) - t(0)) / N of whole calls as tools/robust_timing.py, the gradients
   passed in so that their cost is in neither; and the library's kernel events of the terms launch
   (pass + reduce) with the achieved bytes/s against the 152 B (colored) and 112 B (robust
   point-to-plane) per source the passes must move.  The difference is the second row and 40 more
   bytes.

AB_LIB=<libm3d.so of another build> times that build instead.
Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/colored_timing.py [--ns 100000] [--iters 30] [--repeats 15] [--warmup 3]"""
import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import numpy as np
import torch

from m3d import _lib, synth

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d.core import Cloud, color_gradients, colored_icp, context, device_empty, icp, ptr, stream_handle, to_device
from matcher.robust import TukeyLoss
from robust_timing import spread, timed

BYTES = {"colored": 152, "robust_plane": 112}  # colored.hip / robust.hip: bytes per source a pass must move


def colour_field(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.ascontiguousarray(np.clip(np.stack([0.5 + 0.3 * np.sin(1.3 * x + 0.4 * y) * np.cos(0.7 * z),
                                                  0.45 + 0.25 * np.cos(0.9 * y - 0.5 * x),
                                                  0.55 + 0.2 * np.sin(1.1 * z + 0.8 * x + 0.3 * y)], axis=1), 0.0, 1.0))


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
    sc, tc = colour_field(synth.apply(T, src)), colour_field(tgt)
    s, t = Cloud(src), Cloud(tgt, tn)
    res = {"ns": ns, "iters": N, "radius": r}

    # 1. the gradient pass against the hybrid search alone
    tc_dev = to_device(tc)
    g_out = device_empty((ns, 3), torch.float64)
    idx, d2, cnt = (device_empty((ns, 30), torch.int32), device_empty((ns, 30), torch.float64),
                    device_empty((ns,), torch.int32))
    calls = {
        "color_gradients": lambda: ctx.check(ctx.lib.m3d_color_gradients(
            ctx.h, t.h, ptr(tc_dev), 2 * r, 30, ptr(g_out), stream_handle()), "color_gradients"),
        "hybrid_search": lambda: ctx.check(ctx.lib.m3d_hybrid_search(
            ctx.h, t.h, 2 * r, 30, ptr(idx), ptr(d2), ptr(cnt), stream_handle()), "hybrid_search"),
    }
    us = {k: [] for k in calls}
    for rep in range(args.warmup + args.repeats):
        for name, fn in calls.items():
            dt, _ = timed(fn)
            if rep >= args.warmup:
                us[name].append(dt)
    res["gradient_pass"] = {k: spread(v) for k, v in us.items()}
    res["lists_at_cap"] = int((cnt == 30).sum().item())
    gm, hm = res["gradient_pass"]["color_gradients"]["median_us"], res["gradient_pass"]["hybrid_search"]["median_us"]
    res["ratio_gradients_over_search"] = gm / hm
    for k, v in res["gradient_pass"].items():
        print(f"{k:>16}: {v['median_us']:9.1f} us per call (min {v['min_us']:.1f}, max {v['max_us']:.1f}, n {v['n']})")
    print(f"gradient pass / hybrid search alone: {gm / hm:.2f} ({res['lists_at_cap']} of {ns} lists at the cap of 30)")

    # 2. the colored terms evaluation against the robust point-to-plane one
    grad = color_gradients(t, tc, 2 * r, 30)
    kw = dict(relative_fitness=-1.0, relative_rmse=-1.0, with_correspondences=False, nn="grid")
    loops = {
        "colored": lambda n: colored_icp(s, t, sc, tc, r, np.eye(4), tgt_gradient=grad, max_iteration=n, **kw),
        "robust_plane": lambda n: icp(s, t, r, np.eye(4), max_iteration=n, kernel=TukeyLoss(0.05), **kw),
    }
    per_eval = {k: [] for k in loops}
    for rep in range(args.warmup + args.repeats):
        for name, fn in loops.items():
            t0, _ = timed(lambda: fn(0))
            tN, out = timed(lambda: fn(N))
            assert out.iterations == N, (name, out.iterations)
            if rep >= args.warmup:
                per_eval[name].append((tN - t0) / N)
    res["per_evaluation"] = {k: spread(v) for k, v in per_eval.items()}
    kern = {}
    for name, fn in loops.items():
        fn(N)
        ctx.profile(True)
        ctx.profile_read(_lib.KERNEL_NN), ctx.profile_read(_lib.KERNEL_TERMS)
        for _ in range(3):
            fn(N)
        nn_ms, nn_n = ctx.profile_read(_lib.KERNEL_NN)
        t_ms, t_n = ctx.profile_read(_lib.KERNEL_TERMS)
        ctx.profile(False)
        kern[name] = {"nn_us": nn_ms / max(nn_n, 1) * 1e3, "terms_us": t_ms / max(t_n, 1) * 1e3, "launches": int(t_n)}
    res["kernel_events"] = kern
    for k, v in res["per_evaluation"].items():
        print(f"{k:>13}: {v['median_us']:8.1f} us per evaluation (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
              f"n {v['n']})")
    for name, b in BYTES.items():
        tu = kern[name]["terms_us"]
        res[f"{name}_terms_achieved_GBs"] = b * ns / (tu * 1e-6) / 1e9 if tu > 0 else None
        print(f"{name:>13} kernel events: NN scan {kern[name]['nn_us']:.1f} us, terms pass + reduce {tu:.1f} us "
              f"({kern[name]['launches']} launches): {b * ns / 1e6:.1f} MB = {res[f'{name}_terms_achieved_GBs']:.0f} GB/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
