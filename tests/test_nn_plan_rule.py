"""The slice plan rule of the brute-force NN launch (nn_plan.h) through its host
entry m3d_debug_nn_plan_host (integer division; the device planner's fp32 form of the same
quotient is compared with it on the GPU, tests/test_gpu_nn_plan.py): S_x = clamp(⌈t_x / τ⌉, 1,
min(S_max, ntiles)) for the smallest τ with Σ S_x ≤ B, and a table of B entries that enumerates
every (x, y < S_x) once.  No GPU."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from m3d import _lib

EMPTY = 0xFFFFFFFF
GOLDEN = Path(__file__).resolve().parent / "golden" / "nn_plan_cfg1_counts.json"


def rule(counts, budget, smax=8, ntiles=98):
    """(S per query block, tau, the table's live entries as (x, y, S) rows); None when refused."""
    lib = _lib.load()
    t = np.ascontiguousarray(counts, np.uint32)
    out = np.full(max(budget, 1), 0xDEADBEEF, np.uint32)
    tau = lib.m3d_debug_nn_plan_host(t.ctypes.data_as(C.c_void_p), len(t), budget, smax, ntiles,
                                     out.ctypes.data_as(C.c_void_p))
    if tau < 1:
        return None
    live = out[out != EMPTY]
    ent = np.column_stack([live & 0xFFFF, (live >> 16) & 0xFF, live >> 24]).astype(np.int64)
    # the live entries come first, the rest are empty
    assert np.all(out[:len(live)] != EMPTY) and np.all(out[len(live):] == EMPTY)
    S = np.zeros(len(t), np.int64)
    S[ent[:, 0]] = ent[:, 2]
    return S, tau, ent


def check(counts, budget, smax=8, ntiles=98):
    """The properties every plan has; returns S."""
    S, tau, ent = rule(counts, budget, smax, ntiles)
    t = np.minimum(np.asarray(counts, np.int64), 1 << 20)
    cap = min(smax, ntiles)
    assert S.sum() <= budget
    assert S.min() >= 1 and S.max() <= cap
    np.testing.assert_array_equal(S, np.clip(-(-t // tau), 1, cap))
    if tau > 1:  # the smallest: one less would not fit
        assert np.clip(-(-t // (tau - 1)), 1, cap).sum() > budget
    order = np.argsort(t, kind="stable")  # monotone in t
    assert np.all(np.diff(S[order]) >= 0)
    # every (x, y < S_x) exactly once, each entry carrying its query block's S, in the uniform
    # launch's order: slice 0 of every query block, then slice 1, …
    want = [(x, y, S[x]) for y in range(S.max()) for x in range(len(S)) if S[x] > y]
    assert [tuple(e) for e in ent] == want
    return S


@pytest.mark.parametrize("seed", range(6))
def test_random_counts(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    counts = rng.integers(0, [4, 20, 98, 3000, 1 << 22, 2][seed], n)
    check(counts, 512)
    check(counts, max(n, 512 - 37 * seed), smax=3 + seed)
    check(counts, n + seed, ntiles=5)


def test_equal_counts_give_the_uniform_slices():
    """196 query blocks, 512 slots: S = ⌊512 / 196⌋ = 2 for any common count above one."""
    for t in (2, 7, 98):
        assert check(np.full(196, t), 512).tolist() == [2] * 196
    assert check(np.full(196, 1), 512).tolist() == [1] * 196
    assert check(np.full(64, 40), 512).tolist() == [8] * 64  # 512 / 64, and the S_max clamp
    assert check(np.full(10, 40), 512).tolist() == [8] * 10


def test_zero_counts_give_one_slice():
    assert check(np.zeros(196, np.int64), 512).tolist() == [1] * 196
    assert check([0, 0, 9], 512, ntiles=5).tolist() == [1, 1, 5]


def test_one_query_block():
    assert check([0], 512).tolist() == [1]
    assert check([3], 512).tolist() == [3]
    assert check([50], 512).tolist() == [8]
    assert check([50], 512, ntiles=5).tolist() == [5]
    assert check([50], 1).tolist() == [1]
    assert check([50], 512, ntiles=1).tolist() == [1]


def test_budget_equal_to_n():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 30, 100)
    assert check(counts, 100).tolist() == [1] * 100
    assert rule(counts, 99) is None  # fewer slots than query blocks: no plan
    assert rule([], 10) is None


def test_cfg1_model_histogram():
    """The model's counts of the cfg1 pair (tools/nn_plan_model.py, bound 0.06²) at B = 512: 3
    query blocks with one slice, 102 with two, 71 with three, 20 with four — 500 blocks; the
    unseeded r² counts: 452 blocks."""
    counts = json.loads(GOLDEN.read_text())
    S = check(counts["0.06^2"], 512)
    assert dict(zip(*np.unique(S, return_counts=True))) == {1: 3, 2: 102, 3: 71, 4: 20}
    assert S.sum() == 500
    S = check(counts["r^2"], 512)
    assert dict(zip(*np.unique(S, return_counts=True))) == {1: 7, 2: 128, 3: 55, 4: 6}
