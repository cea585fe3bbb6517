"""Time of ICP against a mesh's surface (m3d_mesh_icp_run) on the cfg4 generated data: the target
mesh of bench.py's cfg4 (m3d.synth.surface_mesh, 1.1 x --mesh rings, seed 2) and the generated scan
(the vertices of the source mesh, --mesh rings, seed 1), moved by the inverse of a small known
rigid motion; radius --radius.

* Per evaluation, from the library's event pairs (m3d_profile_*): the scan (M3D_KERNEL_NN), terms +
  reduce (M3D_KERNEL_TERMS) and the solve (M3D_KERNEL_LOOP) of loops that run a fixed number of
  evaluations (relative_fitness = relative_rmse = 0: no early stop, no skipped launch), seeded and
  unseeded, grid and (coarse meshes only) brute force; and the whole call on a host clock, per
  evaluation.  Median and min..max over --repeats after --warmup.
* Two yardsticks from the same run: m3d_mesh_closest(path = grid, r0 = radius) on the same points
  (whole call), and the robust point-to-plane loop's terms + reduce and solve at the same ns (the scan
  against the mesh's vertices with their normals, M3D_KERNEL_TERMS and M3D_KERNEL_LOOP per evaluation).
* The brute / grid crossover of this loop over coarser tessellations (--sweep rings).
* What users compare: the whole cold matcher.refine_registration_to_mesh call and
  matcher.refine_registration against the mesh's vertices on the same pair, with both final pose
  errors (the largest |T·p − T_true·p| over the scan).

Needs the GPU; prints readable lines and one JSON line.  AB_LIB=<libm3d.so of another build>
times that build instead (tools/ab_build.sh).
Usage: python tools/mesh_icp_timing.py [--mesh 300] [--radius 0.12] [--evals 8] [--repeats 5] [--warmup 2]"""
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

import matcher
from m3d import _lib, synth

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d import cache as _cache
from m3d.core import Cloud, context, device_empty, icp, ptr, stream_handle, to_device
from m3d.mesh import TriangleMesh, closest_points, icp_to_mesh
from m3d.types import PointCloud


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


def fmt(s):
    return f"{s['median_us']:9.1f} us ({s['min_us']:.1f} … {s['max_us']:.1f})"


def loop_times(ctx, cloud, mesh, radius, init, evals, path, seed, repeats, warmup):
    """Per-evaluation times of `evals` evaluations: scan, terms + reduce, solve (events), whole call (host)."""
    rows = {"scan": [], "terms_reduce": [], "solve": [], "call": []}
    out = None
    for rep in range(warmup + repeats):
        ctx.profile(True)
        for k in (_lib.KERNEL_NN, _lib.KERNEL_TERMS, _lib.KERNEL_LOOP):
            ctx.profile_read(k)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = icp_to_mesh(cloud, mesh, radius, init=init, relative_fitness=0.0, relative_rmse=0.0,
                          max_iteration=evals - 1, path=path, seed=seed)
        call = (time.perf_counter() - t0) * 1e6
        got = {n: ctx.profile_read(k) for n, k in (("scan", _lib.KERNEL_NN), ("terms_reduce", _lib.KERNEL_TERMS),
                                                    ("solve", _lib.KERNEL_LOOP))}
        ctx.profile(False)
        assert out.iterations == evals - 1 and all(n == evals for _, n in got.values()), (out.iterations, got)
        if rep >= warmup:
            for n, (ms, cnt) in got.items():
                rows[n].append(ms * 1e3 / cnt)
            rows["call"].append(call / evals)
    return {n: spread(v) for n, v in rows.items()}, out


def worst_error(T, T_true, pts):
    d = (pts @ T[:3, :3].T + T[:3, 3]) - (pts @ T_true[:3, :3].T + T_true[:3, 3])
    return float(np.sqrt((d * d).sum(axis=1)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=300, help="cfg4 source mesh rings (bench.py --cfg4-mesh)")
    ap.add_argument("--sweep", type=int, nargs="*", default=[8, 12, 16, 24, 32, 64])
    ap.add_argument("--radius", type=float, default=0.12)
    ap.add_argument("--evals", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--brute-max", type=int, default=20000, help="largest F the brute-force loop is timed at")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    on, _ = synth.surface_mesh(args.mesh, 2 * args.mesh, seed=1)
    T_true = synth.random_rigid(5, on.mean(axis=0), rot_range=0.005, trans_range=0.03)
    Ti = np.linalg.inv(T_true)
    scan = np.ascontiguousarray(on @ Ti[:3, :3].T + Ti[:3, 3])
    cloud = Cloud(scan)
    r = args.radius
    out = {"scan_points": len(scan), "radius": r, "evals": args.evals, "start_error": worst_error(np.eye(4), T_true, scan),
           "auto_brute_max": int(ctx.lib.m3d_mesh_auto_brute_max()), "sweep": []}
    print(f"scan {len(scan)} points, start error {out['start_error']:.3g}, radius {r}")
    for rings in list(args.sweep) + [int(args.mesh * 1.1)]:
        v, f = synth.surface_mesh(rings, 2 * rings, seed=2)
        mesh = TriangleMesh(v, f)
        row = {"rings": rings, "triangles": int(len(f))}
        for name, path, seed in (("grid_seeded", "grid", True), ("grid_unseeded", "grid", False), ("brute", "brute", False)):
            if path == "brute" and len(f) > args.brute_max:
                row[name] = None
                continue
            row[name], res = loop_times(ctx, cloud, mesh, r, np.eye(4), args.evals, path, seed, args.repeats, args.warmup)
            row[name]["bits"] = res.transformation.tobytes().hex()
            row[name]["fitness"] = res.fitness
        row["same_bits"] = len({row[n]["bits"] for n in ("grid_seeded", "grid_unseeded", "brute") if row[n]}) == 1
        for n in ("grid_seeded", "grid_unseeded", "brute"):
            if row[n]:
                del row[n]["bits"]
        out["sweep"].append(row)
        print(f"F = {len(f):7d} ({rings} rings), fitness {row['grid_seeded']['fitness']:.3f}, same bits {row['same_bits']}")
        for n in ("grid_seeded", "grid_unseeded", "brute"):
            if row[n]:
                t = row[n]
                print(f"   {n:14s} scan {fmt(t['scan'])}  terms+reduce {fmt(t['terms_reduce'])}  solve {fmt(t['solve'])}"
                      f"  whole call / evaluation {fmt(t['call'])}")
    out["cfg4"] = out["sweep"][-1]
    cross = [x for x in out["sweep"] if x["brute"] and x["grid_seeded"]["scan"]["median_us"] < x["brute"]["scan"]["median_us"]]
    out["crossover_triangles"] = cross[0]["triangles"] if cross else None
    print(f"grid scan first faster than the brute-force scan at F = {out['crossover_triangles']}")
    # yardstick 1: m3d_mesh_closest on the same points (on the device already, outputs preallocated),
    # grid path, first radius = the loop's
    q = to_device(scan)
    d2 = device_empty((len(scan),), torch.float64)
    tri = device_empty((len(scan),), torch.int32)
    pt = device_empty((len(scan), 3), torch.float64)
    _, h = mesh._handle()
    us = []
    for rep in range(args.warmup + args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.check(ctx.lib.m3d_mesh_closest(ctx.h, h, ptr(q), len(scan), None, _lib.MESH_GRID, float(r), ptr(d2),
                                           ptr(tri), ptr(pt), None, None, stream_handle()), "mesh_closest")
        us.append((time.perf_counter() - t0) * 1e6)
    out["mesh_closest_yardstick"] = dict(spread(us[args.warmup:]), rounds=mesh.grid_info()["rounds"])
    print(f"yardstick m3d_mesh_closest(path = grid, r0 = {r}), whole call, {out['mesh_closest_yardstick']['rounds']} "
          f"rounds: {fmt(out['mesh_closest_yardstick'])}")
    # yardstick 2: the robust point-to-plane loop's terms + reduce and solve at the same ns (target: the mesh's vertices)
    vn = np.zeros_like(v)
    cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    for k in range(3):
        np.add.at(vn, f[:, k], cr)
    vn /= np.linalg.norm(vn, axis=1, keepdims=True)
    tgt = Cloud(v, vn)
    us, us_solve = [], []
    for rep in range(args.warmup + args.repeats):
        ctx.profile(True)
        ctx.profile_read(_lib.KERNEL_TERMS)
        ctx.profile_read(_lib.KERNEL_LOOP)
        o = icp(cloud, tgt, r, init=np.eye(4), relative_fitness=0.0, relative_rmse=0.0, max_iteration=args.evals - 1,
                kernel=matcher.TukeyLoss(0.05))
        ms, cnt = ctx.profile_read(_lib.KERNEL_TERMS)
        ms_s, cnt_s = ctx.profile_read(_lib.KERNEL_LOOP)
        ctx.profile(False)
        us.append(ms * 1e3 / max(cnt, 1))
        us_solve.append(ms_s * 1e3 / max(cnt_s, 1))
    out["robust_terms_reduce_yardstick"] = spread(us[args.warmup:])
    out["robust_solve_yardstick"] = spread(us_solve[args.warmup:])
    print(f"yardstick robust point-to-plane loop per evaluation at ns = {len(scan)}: terms + reduce "
          f"{fmt(out['robust_terms_reduce_yardstick'])}, solve {fmt(out['robust_solve_yardstick'])}")
    # what users compare: the whole cold calls and their pose errors, at three tessellations
    out["refine"] = []
    for rings in (24, 64, int(args.mesh * 1.1)):
        v, f = synth.surface_mesh(rings, 2 * rings, seed=2)
        vn = np.zeros_like(v)
        cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        for k in range(3):
            np.add.at(vn, f[:, k], cr)
        vn /= np.linalg.norm(vn, axis=1, keepdims=True)
        _cache.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res_m = matcher.refine_registration_to_mesh(scan, TriangleMesh(v, f), np.eye(4), r / 0.4)
        cold_m = time.perf_counter() - t0
        _cache.clear()
        t0 = time.perf_counter()
        res_v = matcher.refine_registration(scan, PointCloud(v, vn), np.eye(4), r / 0.4)
        cold_v = time.perf_counter() - t0
        row = {"triangles": int(len(f)), "vertices": int(len(v)),
               "to_mesh": {"cold_ms": cold_m * 1e3, "pose_error": worst_error(res_m.transformation, T_true, scan),
                           "fitness": res_m.fitness, "rmse": res_m.inlier_rmse},
               "to_vertices": {"cold_ms": cold_v * 1e3, "pose_error": worst_error(res_v.transformation, T_true, scan),
                               "fitness": res_v.fitness, "rmse": res_v.inlier_rmse}}
        out["refine"].append(row)
        print(f"F = {len(f):7d}: refine_registration_to_mesh cold {cold_m * 1e3:7.1f} ms, pose error "
              f"{row['to_mesh']['pose_error']:.3g}, fitness {res_m.fitness:.4f} | refine_registration against the "
              f"{len(v)} vertices cold {cold_v * 1e3:7.1f} ms, pose error {row['to_vertices']['pose_error']:.3g}, "
              f"fitness {res_v.fitness:.4f}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
