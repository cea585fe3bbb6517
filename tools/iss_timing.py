"""Time of the ISS keypoints (m3d_compute_iss_keypoints) on the generated scan of tools/plane_timing.py
with its plane removed (segment_plane on the device first, as tools/dbscan_timing.py does): 180k and
1M points before the removal.  Default radii (6 and 4 model resolutions) and parameters.

* Whole calls, HIP events around each (the cloud is on the device already, its grids cached by the
  warm-up calls): ``compute_iss_keypoints`` with default radii (the resolution step included), the
  same with the resolved radii passed in (pass A, the eigen launch, pass B, the compaction),
  ``model_resolution`` alone and, on the same cloud at ``salient_radius``,
  ``remove_radius_outlier(with_counts=True)`` — ONE full count scan, the yardstick.  Median and
  min..max over --repeats after --warmup.
* Kernel events of the library (m3d_profile_*), in a pass of their own, of the call with the radii
  passed in: pass A (moments), the eigen launch, pass B (non-maximum), the compaction.

Under ``rocprofv3 --kernel-trace --stats`` the kernels to read are ``moments_kernel`` against
``radius_count_kernel<true>``, ``eigen_kernel`` and ``nonmax_kernel``.

``--scale S`` multiplies the resolved radii by S for everything but the default-radii call: the
scan's strays inflate the mean nearest-neighbour distance several-fold over the object's spacing
(tools/dbscan_timing.py prints both), so the default radii hold thousands of neighbours; a scale of
0.25 shows the regime of a few dozen.

``AB_LIB=tools/ab/NAME.so`` times another build of the library (tools/ab_build.sh).

Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/iss_timing.py [--repeats 15] [--warmup 3] [--small-only] [--scale 1.0]"""
import argparse
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))

import numpy as np
import torch

from dbscan_timing import THR, scan, spread, timed
from m3d import _lib, prep
from m3d.core import Cloud, context

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()


def one_config(ctx, n, repeats, warmup, scale):
    P = scan(n)
    _, inliers = prep.segment_plane(P, THR, 3, 100, seed=7)
    keep = np.ones(n, bool)
    keep[inliers] = False
    P = np.ascontiguousarray(P[keep])
    cloud = Cloud(P)
    idx, out = prep.compute_iss_keypoints(cloud, with_details=True)
    rs, rn = scale * out.salient_radius, scale * out.non_max_radius
    if scale != 1.0:
        idx, out = prep.compute_iss_keypoints(cloud, rs, rn, with_details=True)
    calls = {
        "compute_iss_keypoints_default_radii": lambda: prep.compute_iss_keypoints(cloud),
        "compute_iss_keypoints_given_radii": lambda: prep.compute_iss_keypoints(cloud, rs, rn),
        "model_resolution": lambda: prep.model_resolution(cloud),
        "remove_radius_outlier_counts": lambda: prep.remove_radius_outlier(cloud, 5, rs, with_counts=True),
    }
    res = {"n_scan": n, "n": len(P), "scale": scale, "resolution": rs / (6.0 * scale), "salient_radius": rs, "non_max_radius": rn,
           "num_keypoints": out.num_keypoints, "num_salient": out.num_salient, "num_counted": out.num_counted,
           "mean_neighbours": float(out.counts.mean()), "calls": {}}
    for name, fn in calls.items():
        us = []
        for rep in range(warmup + repeats):
            t, _ = timed(fn)
            if rep >= warmup:
                us.append(t)
        res["calls"][name] = spread(us)
    c = res["calls"]
    res["ratio_to_count_scan"] = (c["compute_iss_keypoints_given_radii"]["median_us"]
                                  / c["remove_radius_outlier_counts"]["median_us"])
    # kernel events, in a pass of their own
    ids = {"pass_a_moments": _lib.KERNEL_SCORE, "eigen": _lib.KERNEL_LOOP, "pass_b_nonmax": _lib.KERNEL_NN,
           "compaction": _lib.KERNEL_KABSCH}
    fn = calls["compute_iss_keypoints_given_radii"]
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
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    out = {"configs": []}
    for n in [180_000] + ([] if args.small_only else [1_000_000]):
        r = one_config(ctx, n, args.repeats, args.warmup, args.scale)
        out["configs"].append(r)
        print(f"scan of {n}: {r['n']} points without the plane, resolution {r['resolution']:.5f}, scale {r['scale']}, salient radius "
              f"{r['salient_radius']:.5f}, non-max radius {r['non_max_radius']:.5f}: {r['num_keypoints']} keypoints of "
              f"{r['num_salient']} salient of {r['num_counted']} counted, {r['mean_neighbours']:.1f} neighbours per point")
        for name, v in r["calls"].items():
            print(f"  {name:>38}: {v['median_us']:9.1f} us per call (min {v['min_us']:.1f}, max {v['max_us']:.1f}, "
                  f"n {v['n']})")
        print(f"  {'given radii / count scan':>38}: {r['ratio_to_count_scan']:9.2f}")
        for name, v in r["kernel_events"].items():
            print(f"  {name:>38}: {v['us_per_call']:9.1f} us per call in {v['launches_per_call']:.0f} event brackets")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
