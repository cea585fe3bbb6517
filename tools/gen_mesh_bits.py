"""Record tests/golden/mesh_icp_bits.npz: the raw output bits of m3d_mesh_icp_run,
m3d_mesh_icp_terms and m3d_mesh_closest on the fixed cases of tests/mesh_bits_cases.py.

The committed fixture was recorded from the build before mesh_icp.hip's solve kernel, host-built
state, triangle sweep and box walk were merged with icp.hip's and mesh.hip's; the test
test_gpu_mesh_icp.py::test_bits_of_the_recorded_build holds every later build to it.  Record it
again only when the contract itself changes, and say so in the commit.

Every case runs on every path variant; the contract says they return the same bits, and the
recording stops if they do not.  Needs the GPU.  AB_LIB=<libm3d.so of another build> records that
build instead (tools/ab_build.sh).
Usage: python tools/gen_mesh_bits.py [--out tests/golden/mesh_icp_bits.npz]"""
import argparse
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT / "3d-matching_amd"), str(ROOT / "tests")]

import numpy as np

from m3d import _lib

if os.environ.get("AB_LIB"):  # another build of libm3d.so (tools/ab_build.sh)
    _lib.LIB_PATH = Path(os.environ["AB_LIB"]).resolve()

import mesh_bits_cases as B


def pack(rec):
    """{"call/case/field": array}, in the order B.record yields them → one byte string per call (the
    test walks the same order and takes each field's bytes off the front)."""
    blobs = {}
    for key, a in rec.items():
        blobs.setdefault(key.split("/")[0], []).append(np.ascontiguousarray(a).tobytes())
    return {call: np.frombuffer(b"".join(parts), np.uint8) for call, parts in blobs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "mesh_icp_bits.npz"))
    args = ap.parse_args()
    assert _lib.load().m3d_mesh_brute_tile() == B.TILE
    rec = {}
    for call in ("run", "terms", "closest"):
        for key, variant, fields in B.record(call):
            for name, a in fields.items():
                a = np.ascontiguousarray(a)
                if f"{key}/{name}" not in rec:
                    rec[f"{key}/{name}"] = a
                assert B.same_bits(rec[f"{key}/{name}"], a), f"{key} {name}: {variant} differs from the first variant"
            if call == "run":
                print(f"{key} {variant}: fitness {fields['fit_rmse'][0]:.3f}, count, iterations, converged {fields['counts']}")
            elif call == "terms":
                print(f"{key} {variant}: matched {int(fields['sums'][28])} of {len(fields['tri'])}")
            else:
                print(f"{key} {variant}: regions {np.bincount(fields['region'], minlength=7)[:7]}, "
                      f"unanswered {(fields['triangle'] < 0).sum()}")
    np.savez_compressed(args.out, **pack(rec))
    print(f"{args.out}: {len(rec)} arrays, {Path(args.out).stat().st_size} bytes")


if __name__ == "__main__":
    main()
