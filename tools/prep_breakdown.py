#!/usr/bin/env python3
"""Wall-time breakdown of Ply()'s full-cloud normals stage (ply.py:66 EstimateNormals on the
full-resolution cloud, radius 2v, max_nn 30) on a generated 180k-vertex scan: upload, cloud
pack, grid, neighbourhoods + normals, download.  --k: another max_nn (up to 256) for both calls.
AB_LIB=<libm3d.so of another build> times that build instead."""
import argparse
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import numpy as np
import torch

from m3d import _lib

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
from m3d import prep, synth
from m3d.core import Cloud


def lap(t0, name, out):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out[name] = round((t - t0) * 1e3, 3)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    v, _ = synth.surface_mesh(300, 600, seed=1)
    pts = v.astype(np.float32).astype(np.float64)
    for rep in range(a.reps):
        out = {}
        torch.cuda.synchronize()
        t = time.perf_counter()
        c = Cloud(pts)
        t = lap(t, "cloud_create", out)
        nrm = prep.estimate_normals(c, 0.6, a.k)
        t = lap(t, "estimate_normals(total)", out)
        idx, d2, cnt = prep.hybrid_search(c, 0.6, a.k)
        t = lap(t, "hybrid_search+download", out)
        print(rep, len(pts), a.k, out, "mean neighbours", float(cnt.mean()))


if __name__ == "__main__":
    main()
