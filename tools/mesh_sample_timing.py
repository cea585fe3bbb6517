"""Time of surface sampling (m3d_mesh_sample) and minimum-distance thinning (m3d_thin_min_distance)
on the cfg4 generated model: the target mesh of bench.py's cfg4 (m3d.synth.surface_mesh, 1.1 x
--mesh rings, seed 2; 435,600 triangles at the default).

* --samples (1M) uniform samples: whole calls through the C ABI, the outputs on the device already, a
  host clock around each (the call returns after a stream synchronise).  The first call, which builds
  the cumulative weights, is timed on its own; median and min..max over --repeats after --warmup.
* Thinning those samples at a radius that leaves about --keep (100k) of them (found by one
  correction step from the jamming density of dart throwing), with its round count; the first call,
  which builds the cloud's grid of that cell, on its own.
* Yardsticks in the same run: the numpy restatement of both contracts
  (tests/mesh_sample_restatement.py, one run each; the thinning's mask is compared), and
  prep.voxel_down_sample of the same cloud with the radius as voxel size.
* The cfg4 pose error, coarse (register(..., refine=False), the reference's iteration=30) and
  refined, with the target built from the model's VERTICES as today (refine_registration against
  them) against Ply.from_mesh (refine_registration_to_mesh: register_to_mesh's two stages).

Needs the GPU; prints readable lines and one JSON line.  Nothing is asserted.
Usage: python tools/mesh_sample_timing.py [--mesh 300] [--samples 1000000] [--keep 100000] [--no-numpy]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "3d-matching_amd"))
sys.path.insert(0, str(ROOT / "tests"))

import numpy as np
import torch

from m3d import prep, synth
from m3d.core import Cloud, context, device_empty, ptr, stream_handle
from m3d.mesh import TriangleMesh


def spread(v):
    return {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v), "n": len(v)}


def fmt(s):
    return f"{s['median_us']:.1f} us (min {s['min_us']:.1f}, max {s['max_us']:.1f}, n {s['n']})"


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e6, r


def worst_error(T, T_true, pts):
    d = (pts @ T[:3, :3].T + T[:3, 3]) - (pts @ T_true[:3, :3].T + T_true[:3, 3])
    return float(np.sqrt((d * d).sum(axis=1)).max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mesh", type=int, default=300, help="cfg4 source mesh rings (bench.py --cfg4-mesh)")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--keep", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-numpy", action="store_true", help="skip the numpy restatement yardsticks")
    ap.add_argument("--no-pose", action="store_true", help="skip the cfg4 registration")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    ctx = context()
    rings = int(args.mesh * 1.1)
    v, f = synth.surface_mesh(rings, 2 * rings, seed=2)
    mesh = TriangleMesh(v, f)
    area = mesh.get_surface_area()
    n = args.samples
    out = {"triangles": int(len(f)), "area": area, "samples": n}

    # ---- sampling
    _, h = mesh._handle()
    pt = device_empty((n, 3), torch.float64)
    tri = device_empty((n,), torch.int32)
    uv = device_empty((n, 2), torch.float64)
    nrm = device_empty((n, 3), torch.float64)

    def sample():
        ctx.check(ctx.lib.m3d_mesh_sample(ctx.h, h, n, 0, ptr(pt), ptr(tri), ptr(uv), ptr(nrm), stream_handle()),
                  "mesh_sample")

    first, _ = clock(sample)
    us = [clock(sample)[0] for _ in range(args.warmup + args.repeats)][args.warmup:]
    out["sample"] = dict(spread(us), first_call_us=first, **mesh.sample_info())
    print(f"F = {len(f)}, area {area:.2f}: {n} uniform samples {fmt(out['sample'])}; first call (builds the weights) "
          f"{first:.1f} us; {out['sample']['nonzero']} triangles with weight")
    pts = pt.cpu().numpy()

    # ---- thinning
    cloud = Cloud(pt)
    dec = device_empty((n,), torch.int32)
    kept, rounds = C.c_int64(0), C.c_int32(0)

    def thin(r):
        ctx.check(ctx.lib.m3d_thin_min_distance(ctx.h, cloud.h, float(r), 0, ptr(dec), C.byref(kept), C.byref(rounds),
                                                stream_handle()), "thin_min_distance")
        return int(kept.value), int(rounds.value)

    r = float(np.sqrt(0.65 * area / args.keep))
    k0, _ = thin(r)
    r = float(r * np.sqrt(k0 / args.keep))  # the kept count goes with 1 / r²
    first, (k, nr) = clock(lambda: thin(r))
    us = [clock(lambda: thin(r))[0] for _ in range(args.warmup + args.repeats)][args.warmup:]
    out["thin"] = dict(spread(us), first_call_us=first, radius=r, kept=k, rounds=nr)
    print(f"thinning at r = {r:.5f}: {k} of {n} kept in {nr} rounds, {fmt(out['thin'])}; first call (builds the grid) "
          f"{first:.1f} us")
    kept_dev = dec.cpu().numpy() > 0
    us = [clock(lambda: prep.voxel_down_sample(pt, r))[0] for _ in range(args.warmup + args.repeats)][args.warmup:]
    nv = len(prep.voxel_down_sample(pt, r)[0])
    out["voxel_down_sample"] = dict(spread(us), voxel=r, voxels=nv)
    print(f"yardstick: voxel_down_sample of the same cloud at voxel {r:.5f} → {nv} points, {fmt(out['voxel_down_sample'])} "
          "(whole call, result copied to the host)")
    if not args.no_numpy:
        import mesh_sample_restatement as R

        t0 = time.perf_counter()
        ref = R.sample(v, f, n, 0)
        t_s = time.perf_counter() - t0
        same = ref["point"].tobytes() == pts.tobytes()
        t0 = time.perf_counter()
        d_ref, r_ref = R.thin_rounds(pts, r, 0)
        t_t = time.perf_counter() - t0
        out["numpy"] = {"sample_s": t_s, "sample_same_bits": same, "thin_s": t_t, "thin_rounds": r_ref,
                        "thin_same_mask": bool(((d_ref > 0) == kept_dev).all())}
        print(f"yardstick: numpy restatement, sampling {t_s:.2f} s (same bits: {same}), thinning {t_t:.2f} s "
              f"({r_ref} rounds, same mask: {out['numpy']['thin_same_mask']})")

    # ---- cfg4 pose error: vertices as today against Ply.from_mesh
    if not args.no_pose:
        import matcher
        from ply import Ply

        T = synth.random_rigid(31, rot_range=0.5, trans_range=0.5)
        v_s, _ = synth.surface_mesh(args.mesh, 2 * args.mesh, seed=1)
        scan = synth.apply(np.linalg.inv(T), v_s)
        np.random.seed(0)
        src = Ply.from_arrays(scan, voxel_size=0.3, preprocess=True)
        rows = {}
        for name in ("vertices", "from_mesh"):
            t0 = time.perf_counter()
            tgt = Ply.from_arrays(v, voxel_size=0.3, preprocess=True) if name == "vertices" \
                else Ply.from_mesh(mesh, voxel_size=0.3)
            t1 = time.perf_counter()
            coarse = matcher.register(src, tgt, 0.3, refine=False)
            t2 = time.perf_counter()
            fine = matcher.refine_registration(src, tgt, coarse.transformation, 0.3) if name == "vertices" \
                else matcher.refine_registration_to_mesh(src, mesh, coarse.transformation, 0.3)
            t3 = time.perf_counter()
            rows[name] = {"target_points": len(tgt.pcd.points), "target_down": len(tgt.pcd_down.points),
                          "target_ms": (t1 - t0) * 1e3, "coarse_ms": (t2 - t1) * 1e3, "refine_ms": (t3 - t2) * 1e3,
                          "coarse_max_abs_err": float(np.abs(coarse.transformation - T).max()),
                          "coarse_worst_point_err": worst_error(coarse.transformation, T, scan),
                          "fine_max_abs_err": float(np.abs(fine.transformation - T).max()),
                          "fine_worst_point_err": worst_error(fine.transformation, T, scan),
                          "coarse_fitness": coarse.fitness, "fine_fitness": fine.fitness, "fine_rmse": fine.inlier_rmse}
            q = rows[name]
            print(f"cfg4, target from {name}: {q['target_points']} points ({q['target_down']} down-sampled, built in "
                  f"{q['target_ms']:.0f} ms); coarse {q['coarse_ms']:.0f} ms, max |T - T_true| {q['coarse_max_abs_err']:.3g}, "
                  f"worst point {q['coarse_worst_point_err']:.3g}; refined {q['refine_ms']:.0f} ms, max |T - T_true| "
                  f"{q['fine_max_abs_err']:.3g}, worst point {q['fine_worst_point_err']:.3g}, fitness "
                  f"{q['fine_fitness']:.4f}, rmse {q['fine_rmse']:.3g}")
        out["cfg4"] = rows
    print(json.dumps(out))


if __name__ == "__main__":
    main()
