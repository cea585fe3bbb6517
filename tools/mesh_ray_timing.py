"""Time of ray casting against a mesh (m3d_mesh_cast_rays / m3d_mesh_count_rays) on the cfg4
generated data: the target mesh of bench.py's cfg4 (m3d.synth.surface_mesh, 1.1 x --mesh rings,
seed 2; 435,600 triangles at the default) and the generated scan it is registered with (the
vertices of the source mesh, --mesh rings, seed 1; 180,002 points).

* Whole calls through the C ABI, the rays and the outputs on the device already, a host clock around
  each (every call returns after a stream synchronise).  Median and min..max over --repeats after
  --warmup; the first grid call, which builds the triangle grid, is timed on its own.
* A --view x --view pinhole view of the model from outside (RaycastingScene.create_rays_pinhole):
  first hit on the grid path and on the brute-force path, count_intersections of the same rays.
  Brute force is skipped (and said so) where the sweep predicts more than --brute-limit seconds.
* The parity rays of compute_occupancy for the scan (one fixed direction from every scan point):
  the count call alone, and RaycastingScene.compute_signed_distance as a whole Python call (host
  ray construction, upload, m3d_mesh_closest, download) at nsamples 1 and 3.
* The yardstick in the same run: m3d_mesh_closest of the scan against the same mesh, grid path.
* The crossover: the same number of rays as the scan has points (a square view of that many pixels,
  rounded down) against coarser tessellations (--sweep rings), grid and brute force side by side,
  first hit and count, so that the automatic path of the ray calls can be set from a measurement
  (m3d_mesh_ray_auto_brute_max).

Needs the GPU; prints readable lines and one JSON line.
Usage: python tools/mesh_ray_timing.py [--mesh 300] [--view 1024] [--repeats 7] [--warmup 2]"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))

import numpy as np
import torch

from m3d import _lib, synth
from m3d.core import context, device_empty, ptr, stream_handle, to_device
from m3d.mesh import TriangleMesh
from m3d import raycast as RC


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


class Caller:
    """The two ray calls on device-resident rays with preallocated outputs."""

    def __init__(self, ctx, rays):
        flat = np.ascontiguousarray(rays.reshape(-1, 6))
        self.ctx, self.n = ctx, len(flat)
        self.rays = to_device(flat, "float64", (6,))
        self.t = device_empty((self.n,), torch.float64)
        self.tri = device_empty((self.n,), torch.int32)
        self.uv = device_empty((self.n, 2), torch.float64)
        self.cnt = device_empty((self.n,), torch.int32)

    def first(self, mesh, path):
        _, h = mesh._handle()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.ctx.check(self.ctx.lib.m3d_mesh_cast_rays(self.ctx.h, h, ptr(self.rays), self.n, 0.0, float("inf"), path,
                                                       ptr(self.t), ptr(self.tri), ptr(self.uv), stream_handle()),
                       "mesh_cast_rays")
        return (time.perf_counter() - t0) * 1e6

    def count(self, mesh, path):
        _, h = mesh._handle()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.ctx.check(self.ctx.lib.m3d_mesh_count_rays(self.ctx.h, h, ptr(self.rays), self.n, 0.0, float("inf"), path,
                                                        ptr(self.cnt), stream_handle()), "mesh_count_rays")
        return (time.perf_counter() - t0) * 1e6

    def first_bits(self):
        return tuple(x.cpu().numpy().tobytes() for x in (self.t, self.tri, self.uv))

    def count_bits(self):
        return self.cnt.cpu().numpy().tobytes()


def view_rays(v, side):
    scale = float(np.abs(v).max())
    eye = np.array([2.0, 1.2, 2.5]) * scale
    return RC.RaycastingScene.create_rays_pinhole(40.0, np.zeros(3), eye, (0.0, 0.0, 1.0), side, side)


def timed(fn, repeats, warmup):
    return spread([fn() for _ in range(warmup + repeats)][warmup:])


def one_mesh(ctx, rings, side, repeats, warmup, brute_limit_s, per_pair_s):
    """Grid and brute force, first hit and count, of a side x side view of the mesh of `rings`."""
    v, f = synth.surface_mesh(rings, 2 * rings, seed=2)
    mesh = TriangleMesh(v, f)
    call = Caller(ctx, view_rays(v, side))
    res = {"rings": rings, "triangles": int(len(f)), "rays": call.n}
    res["grid_first_call_us"] = call.first(mesh, _lib.MESH_GRID)  # builds the grid
    res["grid_first"] = timed(lambda: call.first(mesh, _lib.MESH_GRID), repeats, warmup)
    res["fallback_rays"] = RC.ray_info(mesh)["fallback"]
    gf = call.first_bits()
    res["hits"] = int((call.tri.cpu().numpy() >= 0).sum())
    res["grid_count"] = timed(lambda: call.count(mesh, _lib.MESH_GRID), repeats, warmup)
    gc = call.count_bits()
    info = mesh.grid_info()
    res["cells"], res["references_per_triangle"] = info["cells"], info["references"] / len(f)
    pred = None if per_pair_s is None else per_pair_s * len(f) * call.n
    if pred is not None and pred > brute_limit_s:
        res["brute_first"] = res["brute_count"] = None
        res["brute_skipped"] = f"predicted {pred:.1f} s per call > --brute-limit {brute_limit_s:g} s"
    else:
        reps, wu = (repeats, warmup) if (pred or 0.0) * (repeats + warmup) < brute_limit_s else (1, 0)
        res["brute_first"] = timed(lambda: call.first(mesh, _lib.MESH_BRUTE), reps, wu)
        res["same_bits_first"] = call.first_bits() == gf
        res["brute_count"] = timed(lambda: call.count(mesh, _lib.MESH_BRUTE), reps, wu)
        res["same_bits_count"] = call.count_bits() == gc
    return res, mesh, v


def line(r):
    def us(x):
        return "skipped" if x is None else f"{x['median_us']:10.1f} us ({x['min_us']:.1f}..{x['max_us']:.1f}, n {x['n']})"

    same = "" if r["brute_first"] is None else f"; same bits: {r['same_bits_first']} {r['same_bits_count']}"
    return (f"F = {r['triangles']:7d} ({r['rings']} rings), {r['rays']} rays, {r['hits']} hit: first hit grid "
            f"{us(r['grid_first'])}, brute {us(r['brute_first'])}; count grid {us(r['grid_count'])}, brute "
            f"{us(r['brute_count'])}; grid first call {r['grid_first_call_us']:.1f} us, {r['cells']} cells, "
            f"{r['references_per_triangle']:.2f} references per triangle, {r['fallback_rays']} fallback rays{same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=300, help="cfg4 source mesh rings (bench.py --cfg4-mesh)")
    ap.add_argument("--view", type=int, default=1024, help="pixels per side of the pinhole view")
    ap.add_argument("--sweep", type=int, nargs="*", default=[4, 6, 8, 12, 16, 24, 32, 48, 64, 128])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--brute-limit", type=float, default=20.0, help="seconds per brute-force call")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    scan, _ = synth.surface_mesh(args.mesh, 2 * args.mesh, seed=1)
    out = {"scan_points": len(scan), "ray_auto_brute_max": int(ctx.lib.m3d_mesh_ray_auto_brute_max()), "sweep": []}
    side = int(np.sqrt(len(scan)))
    per_pair_s = None  # brute-force seconds per (ray, triangle), from the last measured size
    for rings in args.sweep:
        r, _, _ = one_mesh(ctx, rings, side, args.repeats, args.warmup, args.brute_limit, per_pair_s)
        if r["brute_first"] is not None:
            per_pair_s = r["brute_first"]["median_us"] * 1e-6 / (r["triangles"] * r["rays"])
        out["sweep"].append(r)
        print(line(r))
    for key in ("first", "count"):
        faster = [r for r in out["sweep"] if r[f"brute_{key}"] and
                  r[f"grid_{key}"]["median_us"] < r[f"brute_{key}"]["median_us"]]
        out[f"crossover_triangles_{key}"] = faster[0]["triangles"] if faster else None
    print(f"grid first faster than brute force at F = {out['crossover_triangles_first']} (first hit), "
          f"{out['crossover_triangles_count']} (count); path 0 takes brute force up to F = {out['ray_auto_brute_max']}")
    # the cfg4 mesh: the big view, then the scan's parity rays and the signed distance
    r, mesh, v = one_mesh(ctx, int(args.mesh * 1.1), args.view, args.repeats, args.warmup, args.brute_limit,
                          per_pair_s)
    out["cfg4_view"] = r
    print("cfg4 view: " + line(r))
    rays = np.hstack([scan, np.broadcast_to(RC.occupancy_directions(1)[0], scan.shape)])
    call = Caller(ctx, rays)
    out["scan_parity_count"] = timed(lambda: call.count(mesh, _lib.MESH_GRID), args.repeats, args.warmup)
    out["scan_parity_fallback_rays"] = RC.ray_info(mesh)["fallback"]
    scene = RC.RaycastingScene()
    scene.add_triangles(mesh)
    for ns in (1, 3):
        def whole():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scene.compute_signed_distance(scan, ns)
            return (time.perf_counter() - t0) * 1e6

        out[f"signed_distance_nsamples_{ns}"] = timed(whole, args.repeats, args.warmup)
    occ = scene.compute_occupancy(scan, 3)
    out["scan_inside_fraction"] = float(occ.mean())
    # the yardstick: m3d_mesh_closest of the scan against the same mesh (grid path), device-resident
    q = to_device(scan)
    n = len(scan)
    d2, tri = device_empty((n,), torch.float64), device_empty((n,), torch.int32)
    pt, uv = device_empty((n, 3), torch.float64), device_empty((n, 2), torch.float64)
    reg = device_empty((n,), torch.uint8)
    _, h = mesh._handle()

    def closest():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.check(ctx.lib.m3d_mesh_closest(ctx.h, h, ptr(q), n, None, _lib.MESH_GRID, 0.0, ptr(d2), ptr(tri), ptr(pt),
                                           ptr(uv), ptr(reg), stream_handle()), "mesh_closest")
        return (time.perf_counter() - t0) * 1e6

    out["closest_yardstick"] = timed(closest, args.repeats, args.warmup)
    y = out["closest_yardstick"]
    p, s1, s3 = out["scan_parity_count"], out["signed_distance_nsamples_1"], out["signed_distance_nsamples_3"]
    print(f"scan ({n} points) against F = {r['triangles']}: parity count call {p['median_us']:.1f} us "
          f"({p['min_us']:.1f}..{p['max_us']:.1f}), {out['scan_parity_fallback_rays']} fallback rays; "
          f"compute_signed_distance whole Python call nsamples 1 {s1['median_us']:.1f} us "
          f"({s1['min_us']:.1f}..{s1['max_us']:.1f}), nsamples 3 {s3['median_us']:.1f} us "
          f"({s3['min_us']:.1f}..{s3['max_us']:.1f}); inside fraction {out['scan_inside_fraction']:.3f}; yardstick "
          f"m3d_mesh_closest {y['median_us']:.1f} us ({y['min_us']:.1f}..{y['max_us']:.1f})")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
