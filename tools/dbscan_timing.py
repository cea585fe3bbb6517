"""Time of DBSCAN (m3d_cluster_dbscan) on the generated scan of tools/plane_timing.py with its plane
removed (segment_plane on the device first): 180k and 1M points before the removal, the object box
and the strays after it.  eps = --spacings (2.5) point spacings of the remaining cloud, min_points = 10.
The spacing is the MEDIAN nearest-neighbour distance (knn_search, k = 2): the object's, whereas the
mean is dominated by the strays, whose nearest neighbours lie ten times as far (both are printed).

* Whole calls, HIP events around each (the cloud is on the device already, its grid cached by the
  warm-up calls): ``cluster_dbscan`` (labels only, the core count stops at min_points),
  ``cluster_dbscan(with_details=True)`` (full counts and sizes) and, on the same cloud and radius,
  ``remove_radius_outlier(with_counts=True)`` — ONE full box scan, the yardstick.  Median and
  min..max over --repeats after --warmup.
* Kernel events of the library (m3d_profile_*), in a pass of their own: core flags, link, flatten +
  root scan, label, sizes / counts / largest.
* sklearn's DBSCAN (kd_tree, every host core it is given) on the same points, once; its labels are
  compared with the device's (equal unless a pair sits within rounding of the radius).

Needs the GPU; prints readable lines and one JSON line.  ``AB_LIB=tools/ab/NAME.so`` times another
build of the library (tools/ab_build.sh).
Usage: python tools/dbscan_timing.py [--repeats 15] [--warmup 3] [--small-only] [--no-sklearn]"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))

import numpy as np
import torch

from m3d import _lib, prep
from m3d.core import Cloud, context

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()

THR = 0.012
MIN_POINTS = 10


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


def one_config(ctx, n, spacings, repeats, warmup, with_sklearn):
    P = scan(n)
    _, inliers = prep.segment_plane(P, THR, 3, 100, seed=7)
    keep = np.ones(n, bool)
    keep[inliers] = False
    P = np.ascontiguousarray(P[keep])
    _, d2, _ = prep.knn_search(P, 2)
    spacing = float(np.median(np.sqrt(d2[:, 1])))
    mean_nn = float(np.sqrt(d2[:, 1]).mean())
    eps = spacings * spacing
    cloud = Cloud(P)
    calls = {
        "cluster_dbscan": lambda: prep.cluster_dbscan(cloud, eps, MIN_POINTS),
        "cluster_dbscan_details": lambda: prep.cluster_dbscan(cloud, eps, MIN_POINTS, with_details=True),
        "remove_radius_outlier_counts": lambda: prep.remove_radius_outlier(cloud, MIN_POINTS, eps, with_counts=True),
    }
    res = {"n_scan": n, "n": len(P), "spacing": spacing, "mean_nn_distance": mean_nn, "eps": eps, "min_points": MIN_POINTS, "calls": {}}
    for name, fn in calls.items():
        us = []
        for rep in range(warmup + repeats):
            t, out = timed(fn)
            if rep >= warmup:
                us.append(t)
        res["calls"][name] = spread(us)
    labels, out = calls["cluster_dbscan_details"]()
    res.update(num_clusters=out.num_clusters, num_core=out.num_core, num_noise=out.num_noise,
               largest_size=out.largest_size, mean_neighbours=float(out.counts.mean()))
    # kernel events, in a pass of their own
    ids = {"core_flags": _lib.KERNEL_SCORE, "link": _lib.KERNEL_NN, "flatten_scan": _lib.KERNEL_LOOP,
           "label": _lib.KERNEL_TERMS, "tally_largest": _lib.KERNEL_KABSCH}
    fn = calls["cluster_dbscan"]
    fn()
    ctx.profile(True)
    for k in ids.values():
        ctx.profile_read(k)
    reps = 5
    for _ in range(reps):
        fn()
    res["kernel_events"] = {}
    for name, k in ids.items():
        ms, cnt = ctx.profile_read(k)
        res["kernel_events"][name] = {"us_per_call": ms * 1e3 / reps, "launches_per_call": cnt / reps}
    ctx.profile(False)
    if with_sklearn:
        from sklearn.cluster import DBSCAN

        jobs = int(os.environ.get("OMP_NUM_THREADS", "0")) or min(16, os.cpu_count() or 1)
        t0 = time.perf_counter()
        sk = DBSCAN(eps=eps, min_samples=MIN_POINTS, algorithm="kd_tree", n_jobs=jobs).fit(P).labels_
        res["sklearn"] = {"seconds": time.perf_counter() - t0, "n_jobs": jobs,
                          "labels_equal": bool(np.array_equal(sk, labels))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spacings", type=float, default=2.5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--no-sklearn", action="store_true")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    out = {"configs": []}
    for n in [180_000] + ([] if args.small_only else [1_000_000]):
        r = one_config(ctx, n, args.spacings, args.repeats, args.warmup, not args.no_sklearn)
        out["configs"].append(r)
        print(f"scan of {n}: {r['n']} points without the plane, spacing {r['spacing']:.5f} (mean nearest-neighbour "
              f"distance {r['mean_nn_distance']:.5f}), eps "
              f"{r['eps']:.5f}, min_points {MIN_POINTS}: {r['num_clusters']} clusters, {r['num_core']} core, "
              f"{r['num_noise']} noise, largest {r['largest_size']}, {r['mean_neighbours']:.1f} neighbours per point")
        for name, v in r["calls"].items():
            print(f"  {name:>30}: {v['median_us']:9.1f} us per call (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
                  f"n {v['n']})")
        for name, v in r["kernel_events"].items():
            print(f"  {name:>30}: {v['us_per_call']:9.1f} us per call in {v['launches_per_call']:.0f} event brackets")
        if "sklearn" in r:
            s = r["sklearn"]
            print(f"  {'sklearn DBSCAN (kd_tree)':>30}: {s['seconds']:9.3f} s on {s['n_jobs']} host threads; labels "
                  f"equal: {s['labels_equal']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
