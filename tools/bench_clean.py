"""Outlier removal timed through the C ABI (clean.hip): the unbounded k-NN search at k = 20, the
statistical filter at (20, 2.0) and the radius filter, on the cfg4 generated scan (the 180k vertices
of synth.surface_mesh(300, 600), as the cfg4 tools build it) and on a 1M-point synth cloud, each
plain and with a few uniform strays added.  Baseline: m3d_hybrid_search at the same k with a radius
just large enough that every non-stray point finds its k neighbours (from the k-NN result itself).
Outputs stay on the device (no n×k copy in the timed region); every call is synchronous.  Median
of --reps warm calls; one extra call per search prints the ladder's levels (M3D_KNN_TRACE=1) to
stderr.  Prints one JSON line per cloud.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", "3d-matching_amd")]


def with_strays(P, count, seed):
    import numpy as np

    if count == 0:
        return P
    rng = np.random.default_rng(seed)
    lo, hi = P.min(0), P.max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2
    S = c + rng.uniform(-1.6, 1.6, size=(count, 3)) * h  # the box of the cloud widened by 60 %
    return np.ascontiguousarray(np.concatenate([P, S]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--mesh", type=int, default=300)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--strays", type=float, default=0.002, help="strays added, as a fraction of the cloud")
    a = ap.parse_args()
    import numpy as np
    import torch

    from m3d import _lib, synth

    if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
        _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
    from m3d.core import Cloud, device_empty, ptr, stream_handle

    k = a.k
    scan, _ = synth.surface_mesh(a.mesh, 2 * a.mesh, seed=1)
    big, _ = synth.surface_points(a.n, seed=5)
    clouds = []
    for name, P in (("cfg4_scan", np.ascontiguousarray(scan, np.float64)), ("synth_1m", big)):
        clouds.append((name, P, 0))
        clouds.append((name + "+strays", with_strays(P, int(round(a.strays * len(P))), 17), len(P)))

    def timed(fn):
        fn()  # warm: scratch grown, grids / blocks cached
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), float(np.min(ts))

    for name, P, n_clean in clouds:
        c = Cloud(P)
        ctx, n = c.ctx, c.n
        lib, st = ctx.lib, stream_handle()
        idx = device_empty((n, k), torch.int32)
        d2 = device_empty((n, k), torch.float64)
        cnt = device_empty((n,), torch.int32)
        ind = device_empty((n,), torch.int32)
        m = C.c_int64()
        stats = _lib.OutlierStats()

        def knn():
            ctx.check(lib.m3d_knn_search(ctx.h, c.h, k, ptr(idx), ptr(d2), ptr(cnt), st), "knn_search")

        def stat():
            ctx.check(lib.m3d_remove_statistical_outlier(ctx.h, c.h, k, 2.0, ptr(ind), C.byref(m), C.byref(stats),
                                                         None, st), "remove_statistical_outlier")

        os.environ["M3D_KNN_TRACE"] = "1"
        print(f"[{name}] n = {n}", file=sys.stderr, flush=True)
        knn()
        os.environ["M3D_KNN_TRACE"] = "0"
        t_knn = timed(knn)
        # the k-th neighbour distance of the cloud's own (non-stray) points
        dk = torch.sqrt(d2[: (n_clean or n), k - 1])
        r_hyb = float(dk.max()) * 1.0001
        r_rad = float(dk.median())
        t_stat = timed(stat)
        kept_stat = int(m.value)

        def hyb():
            ctx.check(lib.m3d_hybrid_search(ctx.h, c.h, r_hyb, k, ptr(idx), ptr(d2), ptr(cnt), st), "hybrid_search")

        def rad():
            ctx.check(lib.m3d_remove_radius_outlier(ctx.h, c.h, k - 4, r_rad, ptr(ind), C.byref(m), None, st),
                      "remove_radius_outlier")

        t_hyb = timed(hyb)
        found = int((cnt[: (n_clean or n)] == k).sum())
        t_rad = timed(rad)
        print(json.dumps({
            "cloud": name, "n": n, "k": k, "reps": a.reps,
            "knn_search_ms": round(t_knn[0], 3), "knn_search_min_ms": round(t_knn[1], 3),
            "statistical_filter_ms": round(t_stat[0], 3), "statistical_kept": kept_stat,
            "hybrid_search_ms": round(t_hyb[0], 3), "hybrid_radius": r_hyb,
            "hybrid_full_lists": found, "knn_over_hybrid": round(t_knn[0] / t_hyb[0], 3),
            "radius_filter_ms": round(t_rad[0], 3), "radius": r_rad, "nb_points": k - 4,
            "radius_kept": int(m.value)}), flush=True)
        del c


if __name__ == "__main__":
    main()
