#!/usr/bin/env python3
"""Call time of m3d_evaluate_registration (grid, information on) against m3d_nn1 on the same
inputs: icp_pair(100_000), r = 0.12, a transform near the true one.  Both calls are synchronous,
so a host clock around each warm, repeated call measures enqueue + device work + the one sync;
outputs are preallocated and the C entry points are called directly (no Python result objects).
AB_LIB=<libm3d.so of another build> times that build instead (a build without the evaluation
entry point reports nn1 only).
Usage: python tools/evaluate_timing.py [calls]"""
import ctypes as C
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1] / "3d-matching_amd"))
import numpy as np
import torch

from m3d import _lib, synth

if os.environ.get("AB_LIB"):
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
    if not hasattr(C.CDLL(os.fspath(_lib.LIB_PATH)), "m3d_evaluate_registration"):
        del _lib.SIGNATURES["m3d_evaluate_registration"]
from m3d.core import Cloud, _T16, context, ptr, stream_handle

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
torch.cuda.set_device(0)
ctx = context()
lib = ctx.lib
src, tgt, _, T_true = synth.icp_pair(100_000, 100_000, seed=0)
T = _T16(synth.random_rigid(11, rot_range=0.01, trans_range=0.05) @ T_true)
s, t = Cloud(src), Cloud(tgt)
idx = torch.empty(len(src), dtype=torch.int32, device="cuda")
d2 = torch.empty(len(src), dtype=torch.float64, device="cuda")
res = _lib.EvalResult()
st = stream_handle()


def nn1():
    ctx.check(lib.m3d_nn1(ctx.h, s.h, t.h, T, 0.12, _lib.NN_GRID, ptr(idx), ptr(d2), st), "nn1")


def evaluate():
    ctx.check(lib.m3d_evaluate_registration(ctx.h, s.h, t.h, T, 0.12, _lib.NN_GRID, _lib.EVAL_INFORMATION,
                                            C.byref(res), ptr(idx), ptr(d2), st), "evaluate")


def clock(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts = np.array(ts) * 1e6
    return f"median {np.median(ts):.1f} us, mean {ts.mean():.1f} us, p10 {np.percentile(ts, 10):.1f} us"


fns = [("nn1", nn1)] + ([("evaluate_registration", evaluate)] if "m3d_evaluate_registration" in _lib.SIGNATURES else [])
for rep in range(2):  # alternating, to see the spread
    for name, fn in fns:
        print(f"{name} (grid, 100k x 100k, r 0.12) pass {rep}: {clock(fn)} over {calls} calls", flush=True)
if len(fns) > 1:
    print(f"fitness {res.fitness:.4f} rmse {res.inlier_rmse:.5f} pairs {res.num_correspondences}", flush=True)
