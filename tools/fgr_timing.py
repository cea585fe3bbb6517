"""Time of Fast Global Registration (matcher.fgr, csrc/fgr.hip) on the cfg4 generated scans
(two tessellations of the synthetic surface, STL -> PLY -> Ply(0.3)), beside feature-matching RANSAC.

* Whole calls, wall clock around each (every call is synchronous): global_registration_fgr end to
  end; its stages — the feature rows (prep.feature_correspondences, mutual), normalise + tuple test
  (prep.fgr_tuple_test), and the rest; global_registration at iteration 30 and 30000.  The pose
  error of each (max |T − T_true|), coarse and after refine_registration.
* The loop alone, from the library's kernel events (m3d_profile_*) in a pass of their own: 64
  iterations over the tuple test's 3000 rows on the one-workgroup path (one launch) and on the
  multi-block path forced onto the same rows (64 launches); the multi-block path at 1e5 and 1e6
  rows (the tuple test's rows drawn again with replacement).

Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/fgr_timing.py [--repeats 15] [--warmup 3] [--mesh 180]"""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))

import numpy as np
import torch

from m3d import _lib, plyio, prep, synth
from m3d.core import Cloud, context
from m3d.types import FastGlobalRegistrationOption
from matcher import global_registration, global_registration_fgr, refine_registration
from ply import Ply

V = 0.3


def wall(fn, repeats, warmup):
    us, out = [], None
    for rep in range(warmup + repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if rep >= warmup:
            us.append((time.perf_counter() - t) * 1e6)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "n": len(us)}, out


def loop_events(ctx, fn, reps=5):
    """µs per call between the events the library records around the loop's launches (M3D_KERNEL_LOOP)."""
    fn()
    ctx.profile(True)
    ctx.profile_read(_lib.KERNEL_LOOP)
    for _ in range(reps):
        fn()
    ms, cnt = ctx.profile_read(_lib.KERNEL_LOOP)
    ctx.profile(False)
    return {"us_per_call": ms * 1e3 / reps, "spans_per_call": cnt / reps}  # one event pair brackets the whole loop


def err(T, T_true):
    return float(np.abs(np.asarray(T) - T_true).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mesh", type=int, default=180)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    T = synth.random_rigid(31, rot_range=0.5, trans_range=0.5)
    nl = args.mesh
    with tempfile.TemporaryDirectory() as d:
        v_s, f_s = synth.surface_mesh(nl, 2 * nl, seed=1)
        v_t, f_t = synth.surface_mesh(int(nl * 1.1), int(nl * 2.2), seed=2)
        plyio.write_stl(f"{d}/src.stl", synth.apply(np.linalg.inv(T), v_s), f_s)
        plyio.write_stl(f"{d}/tgt.stl", v_t, f_t)
        plyio.convert_stl_to_ply(f"{d}/src.stl", f"{d}/src.ply")
        plyio.convert_stl_to_ply(f"{d}/tgt.stl", f"{d}/tgt.ply")
        np.random.seed(0)
        src, tgt = Ply(f"{d}/src.ply", V), Ply(f"{d}/tgt.ply", V)
    s_pts, t_pts = src.pcd_down.points, tgt.pcd_down.points
    opt = FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * V)
    out = {"mesh": nl, "ns_down": len(s_pts), "nt_down": len(t_pts), "calls": {}, "loop": {}}

    def coarse_and_fine(fn):
        c = fn()
        return err(c.transformation, T), err(refine_registration(src, tgt, c.transformation, V).transformation, T)

    calls = {
        "fgr_end_to_end": lambda: global_registration_fgr(src, tgt, V, opt),
        "ransac_iteration_30": lambda: global_registration(src, tgt, V, iteration=30),
        "ransac_iteration_30000": lambda: global_registration(src, tgt, V, iteration=30000),
    }
    for name, fn in calls.items():
        t, _ = wall(fn, args.repeats, args.warmup)
        ec, ef = coarse_and_fine(fn)
        out["calls"][name] = dict(t, coarse_err=ec, refined_err=ef)
    t_rows, corres = wall(lambda: prep.feature_correspondences(src.pcd_fpfh, tgt.pcd_fpfh, True, 0.0), args.repeats,
                          args.warmup)
    cs, ct = Cloud(s_pts), Cloud(t_pts)
    t_tup, (rows, trials) = wall(lambda: prep.fgr_tuple_test(cs, ct, corres, opt), args.repeats, args.warmup)
    t_all, _ = wall(lambda: prep.fgr_on_correspondences(cs, ct, corres, opt), args.repeats, args.warmup)
    out["stages"] = {"feature_rows": dict(t_rows, rows=len(corres)),
                     "normalise_tuple_test": dict(t_tup, rows=len(rows), trials=trials),
                     "fgr_on_correspondences": t_all}

    no_test = FastGlobalRegistrationOption(maximum_correspondence_distance=0.5 * V, tuple_test=False)
    for name, path in (("one_workgroup", 1), ("multi_block", 2)):
        out["loop"][f"{len(rows)}_rows_{name}"] = loop_events(
            ctx, lambda: prep.fgr_on_correspondences(cs, ct, rows, no_test, path=path))
    rng = np.random.default_rng(0)
    for n in (100_000, 1_000_000):
        big = rows[rng.integers(0, len(rows), n)]
        out["loop"][f"{n}_rows_multi_block"] = loop_events(ctx, lambda: prep.fgr_on_correspondences(cs, ct, big, no_test),
                                                           reps=3)

    print(f"cfg4 scans, mesh {nl}: {len(s_pts)} / {len(t_pts)} down-sampled points, {len(corres)} mutual rows, "
          f"{len(rows)} rows after {trials} trials")
    for name, v in out["calls"].items():
        print(f"  {name:>24}: {v['median_us']:10.1f} us (min {v['min_us']:.1f}, max {v['max_us']:.1f}, n {v['n']}); "
              f"pose error coarse {v['coarse_err']:.2e}, refined {v['refined_err']:.2e}")
    for name, v in out["stages"].items():
        print(f"  {name:>24}: {v['median_us']:10.1f} us (min {v['min_us']:.1f}, max {v['max_us']:.1f})")
    for name, v in out["loop"].items():
        print(f"  loop {name:>26}: {v['us_per_call']:10.1f} us")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
