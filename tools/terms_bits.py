"""The bits of every side terms pass (terms_pass.h: Generalized ICP, the robust kernels, Colored
ICP), for a diff between two builds of libm3d.so: run once as is and once with
AB_LIB=<libm3d.so of another build> (tools/ab_build.sh, or the Makefile's BUILD= / OUT=), and
`diff` the two outputs — empty when both builds compute the same bits.

* One evaluation: estimator x kernel kind x {grid, brute} x the restatements' EVAL_NS, the 30 sums
  as hex floats and a checksum of the correspondences.
* Loops: the restatements' loop fixtures (tests/gicp_restatement.py, robust_restatement.py,
  colored_restatement.py) from both inits, grid and brute: the 16 doubles of the final
  transformation, fitness, inlier_rmse as hex floats, and the iterations.
Inputs are the restatement modules' generated cases only.  Needs the GPU.
Usage: [AB_LIB=tools/ab/NAME.so] python tools/terms_bits.py > bits.txt"""
import os
import sys
import zlib
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
for p in ("3d-matching_amd", "tests", "oracle"):
    sys.path.insert(0, str(ROOT / p))
import numpy as np

from m3d import _lib

if os.environ.get("AB_LIB"):  # another build of libm3d.so
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()
import colored_restatement as CI
import gicp_restatement as G
import matcher
import robust_restatement as R
from m3d.core import Cloud, colored_icp, colored_terms, gicp, gicp_terms, icp, robust_terms

LOSS = {R.L2: lambda k: matcher.L2Loss(), R.L1: lambda k: matcher.L1Loss(), R.HUBER: matcher.HuberLoss,
        R.CAUCHY: matcher.CauchyLoss, R.GM: matcher.GMLoss, R.TUKEY: matcher.TukeyLoss}
NAME = {v: k for k, v in R.KINDS.items()}


def hexes(v):
    return " ".join(float(x).hex() for x in np.asarray(v, np.float64).reshape(-1))


def terms_line(what, sums, idx):
    print(f"{what}: corr crc {zlib.crc32(idx.cpu().numpy().tobytes()):08x} sums {hexes(sums)}")


def run_line(what, out):
    print(f"{what}: iterations {out.iterations} converged {int(out.converged)} fitness {hexes(out.fitness)} "
          f"rmse {hexes(out.inlier_rmse)} pairs crc {zlib.crc32(out.correspondence_set.tobytes()):08x} "
          f"T {hexes(out.transformation)}")


def main():
    for ns in R.EVAL_NS:
        c = R.eval_case(ns)
        s, t = Cloud(c["src"], c["sn"]), Cloud(c["tgt"], c["tn"])
        for kind in sorted(NAME):
            for nn in ("grid", "brute"):
                terms_line(f"plane {NAME[kind]} {nn} ns={ns}",
                           *robust_terms(s, t, c["T"], G.RADIUS, LOSS[kind](c["k_plane"]), nn=nn))
                terms_line(f"gicp {NAME[kind]} {nn} ns={ns}",  # L2: the call without a kernel, gicp.hip's pass
                           *gicp_terms(s, t, c["T"], G.RADIUS, epsilon=G.EPS, nn=nn, kernel=LOSS[kind](c["k_gicp"])))
    for ns in CI.EVAL_NS:
        f = CI.eval_case(ns)
        s, t = Cloud(f["src"], f["sn"]), Cloud(f["tgt"], f["tn"])
        for kind in sorted(NAME):
            for nn in ("grid", "brute"):
                terms_line(f"colored {NAME[kind]} {nn} ns={ns}",
                           *colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, nn=nn, kernel=LOSS[kind](f["k"])))
        terms_line(f"colored given-gradient ns={ns}",
                   *colored_terms(s, t, f["sc"], f["tc"], f["T"], G.RADIUS, tgt_gradient=f["grad"]))
    src, sn, tgt, tn, _ = G.bumpy_pair(2000, 2000, G.LOOP_SEED)
    o, cp = R.outlier_pair(), CI.colored_pair(2000, 2000, CI.LOOP_SEED)
    gs, gt = Cloud(src, sn), Cloud(tgt, tn)
    os_, ot = Cloud(o["src"], o["sn"]), Cloud(o["tgt"], o["tn"])
    cs, ct = Cloud(cp["src"], cp["sn"]), Cloud(cp["tgt"], cp["tn"])
    for init_kind in ("identity", "perturbed"):
        init = G.loop_init(init_kind)
        for nn in ("grid", "brute"):
            run_line(f"gicp loop {init_kind} {nn}", gicp(gs, gt, G.LOOP_RADIUS, init, epsilon=G.EPS, nn=nn))
            for kind in (R.TUKEY, R.HUBER):
                run_line(f"plane {NAME[kind]} loop {init_kind} {nn}",
                         icp(os_, ot, G.LOOP_RADIUS, init, kernel=LOSS[kind](o["k"][("plane", kind)]), nn=nn))
                run_line(f"gicp {NAME[kind]} loop {init_kind} {nn}",
                         gicp(os_, ot, G.LOOP_RADIUS, init, epsilon=G.EPS, nn=nn,
                              kernel=LOSS[kind](o["k"][("gicp", kind)])))
            run_line(f"colored loop {init_kind} {nn}",
                     colored_icp(cs, ct, cp["sc"], cp["tc"], G.LOOP_RADIUS, init, nn=nn))
            run_line(f"colored tukey loop {init_kind} {nn}",
                     colored_icp(cs, ct, cp["sc"], cp["tc"], G.LOOP_RADIUS, init, nn=nn, kernel=matcher.TukeyLoss(0.05)))


if __name__ == "__main__":
    main()
