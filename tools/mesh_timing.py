"""Time of the point-to-mesh distance (m3d_mesh_closest) on the cfg4 generated data: the target
mesh of bench.py's cfg4 (m3d.synth.surface_mesh, 1.1 x --mesh rings, seed 2) against the generated
scan it is registered with (the vertices of the source mesh, --mesh rings, seed 1; both tessellate
the same surface in the same frame, so the scan lies on the model up to the tessellation).

* Whole calls through the C ABI, the queries and the outputs on the device already, a host clock
  around each (the call returns after a stream synchronise).  Median and min..max over --repeats
  after --warmup; the first grid call, which builds the triangle grid, is timed on its own.
* Grid path and brute-force path at the cfg4 size, the ladder rounds and the references per
  triangle of the grid; brute force is skipped (and said so) where the sweep below predicts more
  than --brute-limit seconds per call.
* The crossover: the same scan against coarser tessellations of the model (--sweep rings), grid and
  brute force side by side, so that m3d_mesh_closest's automatic path can be set from a measurement
  (m3d_mesh_auto_brute_max).
* The yardstick users have today, in the same run: matcher.compute_point_cloud_distance of the
  scan against the mesh's VERTICES (whole call, the clouds packed and cached by the warm-up).

Needs the GPU; prints readable lines and one JSON line.  AB_LIB=<libm3d.so of another build>
times that build instead (tools/ab_build.sh).
Usage: python tools/mesh_timing.py [--mesh 300] [--repeats 7] [--warmup 2] [--brute-limit 20]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))

import numpy as np
import torch

from m3d import _lib, synth

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d.core import context, device_empty, ptr, stream_handle, to_device
from m3d.mesh import TriangleMesh


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


class Caller:
    """m3d_mesh_closest on device-resident queries with preallocated outputs."""

    def __init__(self, ctx, q):
        self.ctx, self.n = ctx, len(q)
        self.q = to_device(q)
        self.d2 = device_empty((self.n,), torch.float64)
        self.tri = device_empty((self.n,), torch.int32)
        self.pt = device_empty((self.n, 3), torch.float64)
        self.uv = device_empty((self.n, 2), torch.float64)
        self.reg = device_empty((self.n,), torch.uint8)

    def __call__(self, mesh, path):
        _, h = mesh._handle()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.ctx.check(self.ctx.lib.m3d_mesh_closest(self.ctx.h, h, ptr(self.q), self.n, None, path, 0.0, ptr(self.d2),
                                                     ptr(self.tri), ptr(self.pt), ptr(self.uv), ptr(self.reg),
                                                     stream_handle()), "mesh_closest")
        return (time.perf_counter() - t0) * 1e6

    def result(self):
        return tuple(t.cpu().numpy().tobytes() for t in (self.d2, self.tri, self.pt, self.uv, self.reg))


def one_mesh(call, rings, repeats, warmup, brute_limit_s, brute_pred_s):
    v, f = synth.surface_mesh(rings, 2 * rings, seed=2)
    mesh = TriangleMesh(v, f)
    res = {"rings": rings, "triangles": int(len(f)), "queries": call.n}
    res["grid_first_call_us"] = call(mesh, _lib.MESH_GRID)  # builds the grid
    us = [call(mesh, _lib.MESH_GRID) for _ in range(warmup + repeats)][warmup:]
    info = mesh.grid_info()
    grid_bits = call.result()
    res["grid"] = dict(spread(us), rounds=info["rounds"], cells=info["cells"], references=info["references"],
                       doublings=info["doublings"], references_per_triangle=info["references"] / len(f))
    if brute_pred_s is not None and brute_pred_s > brute_limit_s:
        res["brute"] = None
        res["brute_skipped"] = f"predicted {brute_pred_s:.1f} s per call > --brute-limit {brute_limit_s:g} s"
    else:
        reps = repeats if (brute_pred_s or 0.0) * (repeats + warmup) < 4 * brute_limit_s else 1
        wu = warmup if reps > 1 else 0
        us = [call(mesh, _lib.MESH_BRUTE) for _ in range(wu + reps)][wu:]
        res["brute"] = spread(us)
        res["same_bits"] = call.result() == grid_bits
    call(mesh, _lib.MESH_AUTO)
    res["auto_took"] = "brute" if mesh.grid_info()["rounds"] == 0 else "grid"
    return res, mesh, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=300, help="cfg4 source mesh rings (bench.py --cfg4-mesh)")
    ap.add_argument("--sweep", type=int, nargs="*", default=[8, 12, 16, 24, 32, 48, 64, 128])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--brute-limit", type=float, default=20.0, help="seconds per brute-force call")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    scan, _ = synth.surface_mesh(args.mesh, 2 * args.mesh, seed=1)
    call = Caller(ctx, scan)
    out = {"scan_points": len(scan), "auto_brute_max": int(ctx.lib.m3d_mesh_auto_brute_max()), "sweep": []}
    per_pair_s = None  # brute-force seconds per (query, triangle), from the last measured size
    for rings in list(args.sweep) + [int(args.mesh * 1.1)]:
        F = 2 * rings * 2 * rings
        pred = None if per_pair_s is None else per_pair_s * F * call.n
        r, mesh, v = one_mesh(call, rings, args.repeats, args.warmup, args.brute_limit, pred)
        if r["brute"] is not None:
            per_pair_s = r["brute"]["median_us"] * 1e-6 / (r["triangles"] * call.n)
        out["sweep"].append(r)
        g, b = r["grid"], r["brute"]
        print(f"F = {r['triangles']:7d} ({rings} rings), n = {call.n}: grid {g['median_us']:10.1f} us "
              f"(min {g['min_us']:.1f}, max {g['max_us']:.1f}; first call {r['grid_first_call_us']:.1f}), "
              f"{g['rounds']} rounds, {g['references_per_triangle']:.2f} references per triangle, "
              f"{g['cells']} cells, {g['doublings']} doublings; brute "
              + (f"{b['median_us']:10.1f} us (min {b['min_us']:.1f}, max {b['max_us']:.1f}, n {b['n']}), "
                 f"same bits: {r['same_bits']}" if b else f"skipped ({r['brute_skipped']})")
              + f"; auto took {r['auto_took']}")
    out["cfg4"] = out["sweep"][-1]
    # the yardstick: nearest VERTEX of the same mesh, whole calls
    from matcher import compute_point_cloud_distance

    us = []
    for rep in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dv = compute_point_cloud_distance(scan, v)
        us.append((time.perf_counter() - t0) * 1e6)
    out["vertex_nn_yardstick"] = dict(spread(us[args.warmup:]), vertices=len(v))
    dm = np.sqrt(call.d2.cpu().numpy())
    out["mean_distance_to_surface"] = float(dm.mean())
    out["mean_distance_to_nearest_vertex"] = float(dv.mean())
    y = out["vertex_nn_yardstick"]
    print(f"yardstick: compute_point_cloud_distance to the mesh's {len(v)} vertices {y['median_us']:.1f} us per whole "
          f"call (min {y['min_us']:.1f}, max {y['max_us']:.1f}); mean distance to the surface {dm.mean():.3g}, to the "
          f"nearest vertex {dv.mean():.3g}")
    faster = [r for r in out["sweep"] if r["brute"] and r["grid"]["median_us"] < r["brute"]["median_us"]]
    out["crossover_triangles"] = faster[0]["triangles"] if faster else None
    print(f"grid first faster than brute force at F = {out['crossover_triangles']}; path 0 takes brute force up to "
          f"F = {out['auto_brute_max']}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
