"""The inputs of tests/test_gpu_fgr.py, built once and shared with tests/test_fgr_cpu.py, which
checks on the restatement alone that no decision of any of them hangs on a last bit."""
from __future__ import annotations

import functools

import numpy as np

import fgr_restatement as R

TRIAL_BATCH = 16384   # m3d/_lib.py FGR_TRIAL_BATCH (test_fgr_cpu pins the two to each other)
ONE_WG_ROWS = 3072    # m3d/_lib.py FGR_ONE_WG_ROWS

POSE_SEED = 16        # the 600-point scene of the pose test (see test_fgr_cpu's docstring)

TERMS_N = (1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 3000, ONE_WG_ROWS - 1, ONE_WG_ROWS,
           ONE_WG_ROWS + 1, 2 * ONE_WG_ROWS + 7)
TERMS_PAR = (1.0, 0.025)

LOOP_ROWS = (10, 11, 64, 65, 3000, ONE_WG_ROWS)
LOOP_ITERS = (0, 1, 4, 5, 64)
# decrease_mu with a radius at which par stops falling mid-run: 1 / 1.4^k first drops to <= 0.05 at
# k = 9, the division of iteration 32
LOOP_MAXCD = 0.05


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def terms_rows():
    """2·ONE_WG_ROWS + 7 rows of normalised-size points with residuals of every size against par."""
    rng = np.random.default_rng(7)
    n = max(TERMS_N)
    q = rng.uniform(-1.0, 1.0, (n, 3))
    p = q + rng.standard_normal((n, 3)) * rng.choice([1e-3, 0.05, 0.5], (n, 1))
    return frozen(p, q)


@functools.lru_cache(maxsize=None)
def scene600():
    """600 points, about half the rows wrong, σ = 0.01; the target has 37 more points (ns ≠ nt)."""
    return R.scene(600, 0.5, 0.01, seed=3, nt_extra=37)


@functools.lru_cache(maxsize=None)
def big_scene():
    """ONE_WG_ROWS rows, three in ten wrong: the loop cases are its prefixes."""
    return R.scene(ONE_WG_ROWS, 0.3, 0.01, seed=5)


@functools.lru_cache(maxsize=None)
def accepted600():
    """Every accepted trial of scene600 (cap beyond reach), for the caps at the batch boundary."""
    S, G, rows, _ = scene600()
    nz = R.normalise(S, G)
    pr, qr = R.gather(S, G, rows, nz)
    return R.tuple_test(pr, qr, 0, 0.95, 10 ** 9).accepted


def boundary_caps():
    """(cap whose stopping trial is the last accepted trial of batch 0, that + 1: the first of batch 1)."""
    k = int(np.searchsorted(accepted600(), TRIAL_BATCH))
    return k, k + 1


@functools.lru_cache(maxsize=None)
def tuple_cases():
    """name → (S, G, rows, option fields)."""
    S, G, rows, _ = scene600()
    k0, k1 = boundary_caps()
    far = frozen(G * 3.0)[0]  # every target edge three times its source edge: no trial passes
    return {
        "n3": (S, G, rows[:3], {}),
        "n10": (S, G, rows[:10], {}),
        "n600_cap_mid_batch": (S, G, rows, {}),
        "n600_abs_scale": (S, G, rows, dict(use_absolute_scale=True)),
        "n600_stop_last_of_batch": (S, G, rows, dict(maximum_tuple_count=k0)),
        "n600_stop_first_of_next": (S, G, rows, dict(maximum_tuple_count=k1)),
        "n600_cap1": (S, G, rows, dict(maximum_tuple_count=1)),
        "n600_cap0": (S, G, rows, dict(maximum_tuple_count=0)),
        "n600_seed9": (S, G, rows, dict(seed=9)),
        "none_pass": (S, far, rows, {}),
    }


def loop_options():
    for iters in LOOP_ITERS:
        for mu in (False, True):
            yield dict(tuple_test=False, iteration_number=iters, decrease_mu=mu,
                       maximum_correspondence_distance=LOOP_MAXCD)


@functools.lru_cache(maxsize=None)
def degenerate_cases():
    S, G, rows, _ = scene600()
    one = np.tile(rows[5:6], (20, 1))
    t = np.linspace(-1.0, 1.0, 40)
    line = np.column_stack([t, 2.0 * t + 0.1, -0.5 * t])
    Sl = np.vstack([line, [[0.3, -0.8, 0.9]]])        # (the extra point keeps the scale off the line's)
    Gl = np.vstack([line + [0.2, 0.1, -0.3], [[1.0, 1.0, 1.0]]])
    lrows = np.column_stack([np.arange(40), np.arange(40)]).astype(np.int32)
    frozen(one, Sl, Gl, lrows)
    return {"one_pair": (S, G, one), "collinear": (Sl, Gl, lrows)}
