"""bench.py's plain run on the GPU: the headline alone, `--steps` timed steps, `--dump-outputs`.

A plain run (no `--full`) warms up W steps, times K steps once and prints the line; every other
section of the line is null.  `--dump-outputs DIR` leaves the last timed step's results as float64
.npy files, identical between two runs with the same arguments (seeded inputs)."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

from m3d.core import IcpLoop

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
NS, NT, ITERS, STEPS, WARMUP = 3001, 2777, 4, 3, 2  # odd sizes, more than one NN tile
FULL_ONLY = ("roofline", "ms_per_step_with_kernel_events", "icp_grid", "cfg1_strong", "cfg1_cold", "cfg3",
             "ransac", "ransac_api", "cfg4_synthetic", "cpu_baseline")


def run_plain(monkeypatch, capsys, out_dir):
    sys.path.insert(0, str(ROOT))
    import bench

    calls = []
    steps = IcpLoop.steps
    monkeypatch.setattr(IcpLoop, "steps", lambda self, n: (calls.append(n), steps(self, n))[1])
    monkeypatch.delenv("M3D_BENCH_FULL", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--ns", str(NS), "--nt", str(NT), "--icp-iters", str(ITERS),
                                      "--dump-outputs", str(out_dir)])
    bench.main()
    lines = [x for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), calls


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(monkeypatch, capsys, tmp_path):
    line, calls = run_plain(monkeypatch, capsys, tmp_path / "a")
    # the loop ran warm-up + timed steps and nothing else (no events pass, no grid leg)
    assert calls == [ITERS + 1] * (WARMUP + STEPS)
    assert line["full"] is False and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["higher_is_better"] is True and line["n_gpus"] == 1
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(ITERS / (line["ms_per_step"] * 1e-3), rel=1e-9)
    for k in FULL_ONLY:
        assert line[k] is None, k
    assert list(line)[-1] == "summary"

    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == {"transformation", "update", "fitness", "inlier_rmse", "num_correspondences",
                        "iterations", "correspondences", "points"}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20
    assert got["transformation"].shape == (4, 4) and got["points"].shape == (NS, 3)
    assert got["correspondences"].shape == (NS,) and got["iterations"][0] == ITERS
    assert got["fitness"][0] == line["check"]["icp_fitness"] > 0
    assert int((got["correspondences"] >= 0).sum()) == int(got["num_correspondences"][0])

    # the same arguments again: the same inputs, so the same arrays to the bit
    line2, _ = run_plain(monkeypatch, capsys, tmp_path / "b")
    for name, a in got.items():
        np.testing.assert_array_equal(np.load(tmp_path / "b" / f"{name}.npy"), a, err_msg=name)
