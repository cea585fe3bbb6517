"""GPU parity of the preprocessing / feature-matching path (prep.hip, feat.hip) against the CPU
oracle (oracle/prep_oracle.py; Open3D semantics restated, parity with Open3D itself unpinned).

Bars (stated):
* voxel down-sampling, hybrid neighbourhoods, feature correspondences: bit-exact (same fp64
  operations in the same order; ties by index on both sides);
* normals: within 1e-9 (the device's acos/cos may differ from the host libm by an ulp);
* FPFH: within 1e-12 on every point whose neighbourhood is edge-clean (oracle
  spfh_edge_sensitive), ≥ 99.5 % of all rows within 1e-6, every group sums to 100 (or 0);
* feature correspondences on the device's own FPFH: bit-exact vs the oracle on those features;
* feature RANSAC: same best hypothesis and validation count (Open3D 0.19's exit rule: the
  correspondence inlier ratio of each new best), transform within 1e-9, fitness and ratio exact,
  rmse within 1e-12 (the validation NN is the exact fp64 decision, nnkey.h), and the best's
  correspondence_set pair for pair.
"""
import numpy as np
import pytest

import prep_oracle as P
from m3d import prep, synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n,voxel,with_normals", [(1, 0.3, False), (7, 10.0, True), (5000, 0.3, True),
                                                  (60000, 0.3, False), (20000, 0.05, True)])
def test_voxel_down_sample_exact(n, voxel, with_normals):
    rng = np.random.default_rng(n)
    pts = rng.uniform(-5, 5, (n, 3)) + np.array([100.0, -50.0, 3.0])
    nrm = rng.normal(size=(n, 3)) if with_normals else None
    got, gn = prep.voxel_down_sample(pts, voxel, nrm)
    ref, rn = P.voxel_down_sample(pts, voxel, nrm)
    np.testing.assert_array_equal(got, ref)
    if with_normals:
        np.testing.assert_array_equal(gn, rn)


def test_voxel_down_sample_rejects_bad_voxel():
    with pytest.raises(ValueError):
        prep.voxel_down_sample(np.zeros((3, 3)), 0.0)
    with pytest.raises(ValueError):
        prep.voxel_down_sample(np.array([[0.0, 0, 0], [1e9, 0, 0]]), 1e-3)


@pytest.mark.parametrize("case,radii", [
    pytest.param(c, None, id=c) for c in ["surface", "duplicates", "plane", "offset", "dense"]] + [
    # 128 < k ≤ 256 (four list slots per lane): some lists full and the rest short and padded; the
    # first k of that form with no list full; ties by index across the 64-lane slot boundaries
    pytest.param("surface", [(1.5, 200)], id="surface-k200"),
    pytest.param("surface", [(1.0, 129)], id="surface-k129"),
    pytest.param("duplicates", [(1.5, 200)], id="duplicates-k200")])
def test_hybrid_search_exact(case, radii):
    """Lists equal the oracle's bit for bit.  "plane" and "dense" are dense enough for the
    two-stage search (prep.hip hybrid_fine_radius: a finer first grid, full search again when
    fewer than k points lie within its radius), "plane" at k = 30 with many such repeats.  The
    k > 128 cases by the oracle: surface-k200 21 % of the lists full, the rest 117 to 199 entries;
    surface-k129 no list full (at most 119); duplicates-k200 84 % full."""
    rng = np.random.default_rng(3)
    radii = radii or [(0.6, 30), (1.5, 100)]
    if case == "dense":
        pts, _ = synth.surface_points(60000, seed=7)
        radii = [(0.6, 30), (1.0, 100)]
    elif case == "surface":
        pts, _ = synth.surface_points(8000, seed=1)
    elif case == "duplicates":
        pts = np.repeat(rng.normal(size=(400, 3)), 5, axis=0)
    elif case == "plane":
        pts = np.c_[rng.uniform(-2, 2, (5000, 2)), np.zeros(5000)]
    else:
        pts = synth.surface_points(5000, seed=2)[0] + np.array([2e4, -1e4, 5e3])
    for radius, k in radii:
        gi, gd, gc = prep.hybrid_search(pts, radius, k)
        ri, rd, rc = P.hybrid_search(pts, radius, k)
        np.testing.assert_array_equal(gc, rc)
        np.testing.assert_array_equal(gi, ri)
        np.testing.assert_array_equal(gd, rd)


def test_normals_match_oracle():
    pts, true = synth.surface_points(6000, seed=4)
    got = prep.estimate_normals(pts, 0.6, 30)
    ref = P.estimate_normals(pts, 0.6, 30)
    np.testing.assert_allclose(got, ref, atol=1e-9)
    got = prep.estimate_normals(pts, 0.6, 30, normals=true)  # oriented like the file's normals
    assert np.all(np.sum(got * true, axis=1) > 0)
    # fewer than 3 neighbours → identity covariance → (0, 0, 1)
    lone = np.array([[0.0, 0, 0], [10.0, 0, 0], [20.0, 0, 0]])
    np.testing.assert_array_equal(prep.estimate_normals(lone, 1.0, 30), [[0, 0, 1]] * 3)


def test_fpfh_matches_oracle():
    """FPFH equals the CPU restatement (glibc acos/atan2) bit for bit on every row.  The swap
    test acos(|a1|) > acos(|a2|) of ComputePairFeatures is decided as correctly rounded acos
    values would (ddmath.h acos_gt); with the device libm's acos instead, near-tied tests (this
    cloud's radius-0.8 normals give neighbours near-identical normals: 86 ties within 1e-14 in
    236k pairs) went the other way on 0.5 % of the rows (round 5's bar: 40 % of rows exact).
    tools/fpfh_parity.py measures the same on cfg4's scans."""
    pts, _ = synth.surface_points(2500, seed=5)
    nrm = P.estimate_normals(pts, 0.8, 30)
    got = prep.compute_fpfh(pts, nrm, 2.0, 100)
    ref = P.compute_fpfh(pts, nrm, 2.0, 100)
    np.testing.assert_array_equal(got, ref)
    sums = got.reshape(-1, 3, 11).sum(axis=2)
    assert np.all((np.abs(sums - 200.0) < 1e-9) | (sums == 0.0))


def test_feature_correspondences_on_device_fpfh():
    """a5 downstream of the device's own FPFH: correspondences computed on the device features
    equal the oracle's correspondences on those same features, bit for bit (mutual filter on and
    off)."""
    src, _ = synth.surface_points(3000, seed=12)
    T = synth.random_rigid(4, rot_range=0.4, trans_range=0.5)
    tgt = synth.apply(T, synth.surface_points(3000, seed=13)[0])
    fs = prep.compute_fpfh(src, prep.estimate_normals(src, 0.6, 30), 1.5, 100)
    ft = prep.compute_fpfh(tgt, prep.estimate_normals(tgt, 0.6, 30), 1.5, 100)
    for mutual in (False, True):
        got = prep.feature_correspondences(fs, ft, mutual)
        ref = P.correspondences_from_features(fs, ft, mutual)
        np.testing.assert_array_equal(got, ref)


@pytest.mark.parametrize("mutual", [False, True])
def test_feature_correspondences_exact(mutual):
    pts, _ = synth.surface_points(3000, seed=6)
    nrm = P.estimate_normals(pts, 0.8, 30)
    f = P.compute_fpfh(pts, nrm, 2.0, 100)
    T = synth.random_rigid(2, rot_range=0.4, trans_range=0.5)
    rng = np.random.default_rng(0)
    perm = rng.permutation(len(pts))
    ft = f[perm] + rng.normal(scale=0.5, size=f.shape)
    got = prep.feature_correspondences(f, ft, mutual)
    ref = P.correspondences_from_features(f, ft, mutual)
    np.testing.assert_array_equal(got, ref)
    del T


def _oracle_pairs(src, tgt, T, max_corr):
    """GetRegistrationResultAndCorrespondences' correspondence_set for T (exact fp64 1-NN within
    max_corr, lowest index on ties), sorted by source index."""
    import icp_oracle

    _, _, corr, _ = icp_oracle.registration_result(icp_oracle.transform_points(T, src), tgt, max_corr)
    return np.asarray(corr, np.int64)


def _assert_same_result(got, ref, src, tgt, max_corr):
    assert got.validations == ref["validations"]
    assert got.best_index == ref["best_index"]
    assert got.fitness == ref["fitness"]
    assert abs(got.inlier_rmse - ref["inlier_rmse"]) <= 1e-12 * max(1.0, ref["inlier_rmse"])
    assert got.corres_ratio == ref["corres_ratio"]  # an integer count over nc on both sides
    np.testing.assert_allclose(got.transformation, ref["transformation"], atol=1e-9)
    # RegistrationResult.correspondence_set, pair for pair: against the oracle's NN under the
    # device's own T (the NN decision) and under the oracle's T (within 1e-9 of it)
    if ref["best_index"] >= 0:
        pairs = np.asarray(got.correspondence_set, np.int64)
        np.testing.assert_array_equal(pairs, _oracle_pairs(src, tgt, got.transformation, max_corr))
        np.testing.assert_array_equal(pairs, _oracle_pairs(src, tgt, ref["transformation"], max_corr))


def test_feature_ransac_matches_oracle():
    src, _ = synth.surface_points(4000, seed=8)
    T = synth.random_rigid(3, rot_range=0.5, trans_range=1.0)
    tgt = synth.apply(T, src) + np.random.default_rng(1).normal(scale=0.01, size=src.shape)
    rng = np.random.default_rng(2)
    corr = np.c_[np.arange(4000), np.arange(4000)]
    bad = rng.random(4000) < 0.6
    corr[bad, 1] = rng.integers(0, 4000, int(bad.sum()))
    kw = dict(max_iteration=300, confidence=0.999, edge_length=0.9, distance=0.45)
    got = prep.ransac_on_correspondences(src, tgt, corr, 0.45, seed=11, **kw)
    ref = P.ransac_feature(src, tgt, corr, 0.45, lambda h: P.native_rows(11, h, len(corr)), **kw)
    _assert_same_result(got, ref, src, tgt, 0.45)
    np.testing.assert_allclose(got.transformation, T, atol=2e-2)
    assert len(got.correspondence_set) == round(got.fitness * len(src))


@pytest.mark.parametrize("bad_ratio,iters,seed,edge,conf,nval",
                         [(0.5, 2000, 16, None, 1.0, 2000), (0.3, 2000, 6, 0.9, 0.999, 5),
                          (0.97, 2000, 5, None, 0.999, 1)])
def test_feature_ransac_batched_validation_matches_oracle(bad_ratio, iters, seed, edge, conf, nval):
    """Batched validation (validate_kernel, batches of 64 → 128 → …) against the sequential
    oracle, Open3D 0.19's exit rule (est_k from the new best's correspondence inlier ratio).
    Case 1: confidence 1.0 (est_k_d = +inf, "we always consume all the iterations") and a first
    hypothesis drawn from three inlier rows, so every later best has a ratio > 0: all 2000
    hypotheses are validated in growing batches, fitness ties decided by rmse.  Case 2: an early
    exit inside the first batch (ratio ≈ 0.65 → est_k = 17).  Case 3: a 97 %-outlier set whose
    first best has correspondence ratio 0: log(1 − 0) = 0, the estimate is −inf, and upstream's
    int conversion of it stops the loop (4 validations)."""
    src, _ = synth.surface_points(3000, seed=seed)
    T = synth.random_rigid(seed + 1, rot_range=0.5, trans_range=1.0)
    tgt = synth.apply(T, src) + np.random.default_rng(seed + 2).normal(scale=0.01, size=src.shape)
    rng = np.random.default_rng(seed + 3)
    corr = np.c_[np.arange(3000), np.arange(3000)]
    bad = rng.random(3000) < bad_ratio
    corr[bad, 1] = rng.integers(0, 3000, int(bad.sum()))
    kw = dict(max_iteration=iters, confidence=conf, edge_length=edge, distance=None)
    got = prep.ransac_on_correspondences(src, tgt, corr, 0.03, seed=seed, **kw)
    ref = P.ransac_feature(src, tgt, corr, 0.03, lambda h: P.native_rows(seed, h, len(corr)), **kw)
    assert ref["validations"] >= nval
    _assert_same_result(got, ref, src, tgt, 0.03)


def test_feature_ransac_exit_uses_corres_ratio_not_fitness():
    """The round-3 verdict's case: a well-overlapping pair (fitness ≈ 1 at the true pose) with 70 %
    outlier correspondences.  A fitness-based estimate (rounds 1–3) exits after a handful of
    validations; Open3D's correspondence-ratio estimate (≈ 0.3 → est_k ≈ 253) keeps going.  The
    device follows the corrected oracle, validation for validation."""
    pts, _ = synth.surface_points(1500, seed=7)
    T = synth.random_rigid(8, rot_range=0.5, trans_range=1.0)
    # 0.01 noise: rmse values are then real distances, not rounding noise (an exact copy makes
    # every good hypothesis's rmse ~1e-15, and "lower rmse wins" compares rounding orders)
    tgt = synth.apply(T, pts) + np.random.default_rng(10).normal(scale=0.01, size=pts.shape)
    rng = np.random.default_rng(9)
    corr = np.c_[np.arange(1500), np.arange(1500)]
    bad = rng.random(1500) < 0.7
    corr[bad, 1] = rng.integers(0, 1500, int(bad.sum()))
    kw = dict(max_iteration=400, confidence=0.999, edge_length=0.9, distance=0.45)
    rows = lambda h: P.native_rows(3, h, len(corr))  # noqa: E731
    ref = P.ransac_feature(pts, tgt, corr, 0.45, rows, **kw)
    old = P.ransac_feature(pts, tgt, corr, 0.45, rows, exit_rule="fitness", **kw)
    assert old["validations"] < 10 < ref["validations"]
    got = prep.ransac_on_correspondences(pts, tgt, corr, 0.45, seed=3, **kw)
    _assert_same_result(got, ref, pts, tgt, 0.45)
    assert got.validations != old["validations"]


def test_feature_ransac_empty_cases():
    pts, _ = synth.surface_points(100, seed=1)
    out = prep.ransac_on_correspondences(pts, pts, np.zeros((2, 2), np.int32), 0.45)
    assert out.fitness == 0.0 and out.best_index == -1
    np.testing.assert_array_equal(out.transformation, np.eye(4))


def test_ply_pipeline_registers_synthetic_scan(tmp_path):
    """Ply(path) → global_registration → refine_registration on a synthetic scan pair
    (cfg4's pipeline; the reference ships no scans)."""
    from m3d import plyio
    from matcher.icp import refine_registration
    from matcher.ransac import global_registration
    from ply import Ply

    pts, nrm = synth.surface_points(40000, seed=21)
    T = synth.random_rigid(22, rot_range=0.5, trans_range=0.5)
    plyio.write_ply(tmp_path / "src.ply", synth.apply(np.linalg.inv(T), pts), binary=True)
    plyio.write_ply(tmp_path / "tgt.ply", synth.surface_points(40000, seed=23)[0], binary=False)
    np.random.seed(0)
    src, tgt = Ply(tmp_path / "src.ply", 0.3), Ply(tmp_path / "tgt.ply", 0.3)
    assert src.pcd_fpfh.data.shape == (33, len(src.pcd_down.points))
    coarse = global_registration(src, tgt, 0.3, iteration=30000)
    assert coarse.fitness > 0.3
    fine = refine_registration(src, tgt, coarse.transformation, 0.3)
    np.testing.assert_allclose(fine.transformation, T, atol=5e-3)


def _ply_oracle(pts, nrm, v):
    """ply.py:106-120 on the oracle: voxel down-sample carrying the file normals (per-voxel
    mean), EstimateNormals(2v, 30) oriented by them, FPFH(5v, 100)."""
    down, dprev = P.voxel_down_sample(pts, v, nrm)
    dn = P.estimate_normals(down, 2 * v, 30, prev_normals=dprev)
    return down, dprev, dn, P.compute_fpfh(down, dn, 5 * v, 100), (P.hybrid_search(down, 5 * v, 100), dn)


def _fpfh_bar(got, ref, pts, nrm, nbrs):
    """test_fpfh_matches_oracle's two tiers."""
    idx, _, cnt = nbrs
    sens = P.spfh_edge_sensitive(pts, nrm, idx, cnt)
    clean = ~sens.copy()
    for i in range(len(pts)):
        if np.any(sens[idx[i, : int(cnt[i])]]):
            clean[i] = False
    assert clean.mean() >= 0.35, clean.mean()
    np.testing.assert_allclose(got[clean], ref[clean], rtol=1e-12, atol=1e-12)
    row_ok = np.all(np.abs(got - ref) <= 1e-6 * np.maximum(1.0, np.abs(ref)), axis=1)
    assert row_ok.mean() >= 0.995, row_ok.mean()


@pytest.mark.parametrize("flip", [False, True])
def test_ply_with_file_normals_follows_open3d(tmp_path, flip):
    """A PLY that carries nx/ny/nz: Open3D's VoxelDownSample averages the file normals into
    pcd_down, and EstimateNormals orients each new normal by that average (ply.py:80,106-112);
    the full-resolution normals follow the file's (ply.py:133).  pcd_down normals within 1e-9 of
    the oracle and FPFH at test_fpfh_matches_oracle's bars; with every file normal flipped, both
    normal sets flip and every normal agrees in sign with the (averaged) file normal."""
    from m3d import plyio
    from ply import Ply

    v = 0.5
    pts, nrm = synth.surface_points(20000, seed=21)
    if flip:
        nrm = -nrm
    plyio.write_ply(tmp_path / "n.ply", pts, nrm, binary=True)
    np.random.seed(3)
    ply = Ply(tmp_path / "n.ply", v)
    down, dprev, dn, fpfh, (nbrs, _) = _ply_oracle(pts, nrm, v)
    np.random.seed(3)
    noise = 0.05 * np.random.randn(*down.shape)            # ply.py:61-62, after the features
    np.testing.assert_array_equal(ply.pcd_down.points, down + noise)
    np.testing.assert_allclose(ply.pcd_down.normals, dn, atol=1e-9)
    assert np.all(np.sum(ply.pcd_down.normals * dprev, axis=1) >= 0.0)
    _fpfh_bar(ply.pcd_fpfh.data.T, fpfh, down, dn, nbrs)
    assert np.all(np.sum(ply.pcd.normals * nrm, axis=1) >= 0.0)
    # without file normals the estimate's sign is the eigen solver's; the file's sign wins here
    plain = P.estimate_normals(down, 2 * v, 30)
    s = np.sign(np.sum(plain * dprev, axis=1))
    np.testing.assert_allclose(ply.pcd_down.normals, plain * np.where(s == 0, 1.0, s)[:, None], atol=1e-9)
    assert (s < 0).mean() > 0.05  # the orientation step changes a visible share of the normals


def test_voxel_down_sample_skips_nan_normals():
    """AccumulatedPoint::AddPoint (Open3D geometry/DownSample.cpp) adds a normal only when none
    of its components is NaN, but divides by every point of the voxel."""
    pts = np.array([[0.0, 0, 0], [0.1, 0, 0], [5.0, 0, 0]])
    nrm = np.array([[0.0, 0, 1], [np.nan, 0, 0], [1.0, 0, 0]])
    got, gn = prep.voxel_down_sample(pts, 1.0, nrm)
    ref, rn = P.voxel_down_sample(pts, 1.0, nrm)
    np.testing.assert_array_equal(got, ref)
    np.testing.assert_array_equal(gn, rn)
    np.testing.assert_array_equal(gn, [[0.0, 0, 0.5], [1.0, 0, 0]])


@pytest.mark.parametrize("iteration", [30, 30000])
def test_cfg4_stl_pipeline(tmp_path, iteration):
    """cfg4 from STL: two tessellations of one surface (two "scans", source moved by T⁻¹) written
    as binary STL → convert_stl-ply.py:1-11 (m3d.plyio.convert_stl_to_ply: merged vertices →
    ASCII PLY) → Ply(path, 0.3) (ply.py:32-66) → matcher.register (= main.py:24-43:
    global_registration → refine_registration) on the GPU.  The reference ships no scans
    (3d_data/.gitignore), so the meshes are generated (m3d.synth.surface_mesh)."""
    from m3d import plyio
    from matcher import register
    from ply import Ply

    T = synth.random_rigid(31, rot_range=0.5, trans_range=0.5)
    v_src, f_src = synth.surface_mesh(180, 360, seed=1)
    v_tgt, f_tgt = synth.surface_mesh(200, 400, seed=2)
    plyio.write_stl(tmp_path / "src.stl", synth.apply(np.linalg.inv(T), v_src), f_src, binary=True)
    plyio.write_stl(tmp_path / "tgt.stl", v_tgt, f_tgt, binary=True)
    n_src = plyio.convert_stl_to_ply(tmp_path / "src.stl", tmp_path / "src.ply")
    n_tgt = plyio.convert_stl_to_ply(tmp_path / "tgt.stl", tmp_path / "tgt.ply")
    assert (n_src, n_tgt) == (len(v_src), len(v_tgt))  # shared STL corners merged back
    np.random.seed(0)
    src, tgt = Ply(tmp_path / "src.ply", 0.3), Ply(tmp_path / "tgt.ply", 0.3)
    assert set(src.stage_ms) >= {"read", "voxel_down_sample", "normals_down", "fpfh", "noise", "normals_full"}
    res = register(src, tgt, 0.3, iteration=iteration)
    np.testing.assert_allclose(res.transformation, T, atol=5e-3)
    assert res.fitness > 0.9


@pytest.mark.gpu
def test_host_text_io_before_any_device_call(tmp_path):
    """A fresh process whose first libm3d use is host-side (ASCII PLY write) must still see the
    device afterwards: libm3d.so has to bind to the HIP runtime torch brings (m3d/_lib.py)."""
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from m3d import plyio, synth\n"
        "from ply import Ply\n"
        "pts, _ = synth.surface_points(20000, seed=21)\n"
        "plyio.write_ply(%r, pts, binary=False)\n"
        "print(len(Ply(%r, 0.3).pcd_down.points))\n"
    ) % (str(root / "3d-matching_amd"), str(tmp_path / "a.ply"), str(tmp_path / "a.ply"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout.split()[-1]) > 0


def test_device_acos_cr_is_correctly_rounded():
    """The swap test's acos compiled for gfx950 (ddmath.h acos_cr through m3d_debug_acos_device)
    equals the correctly rounded acos (200-bit mpmath) on 20,000 arguments — uniform, near 1,
    near 0 — and the host copy bit for bit.  The device libm's own acos is reported beside it:
    it agrees with glibc's on most arguments but not all, which is why the swap test does not
    use it."""
    import ctypes as C
    import math
    import random

    import torch

    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 200
    from m3d.core import context, ptr, stream_handle

    rnd = random.Random(11)
    u = np.array([[r, 1 - r * 1e-6, 1 - rnd.random() ** 8, r * 1e-9, 1 - 2.0 ** -53 * (1 + k % 50)][k % 5]
                  for k, r in ((k, rnd.random()) for k in range(20000))])
    ctx = context()
    ud = torch.from_numpy(u).cuda()
    outs = []
    for mode in (0, 1):
        od = torch.empty_like(ud)
        ctx.check(ctx.lib.m3d_debug_acos_device(ctx.h, ptr(ud), len(u), ptr(od), mode, stream_handle()),
                  "acos_device")
        outs.append(od.cpu().numpy())
    ref = np.array([float(mpmath.acos(mpmath.mpf(x))) for x in u])
    np.testing.assert_array_equal(outs[0], ref)
    host = np.empty_like(u)
    ctx.lib.m3d_debug_acos_cr(u.ctypes.data_as(C.c_void_p), len(u), host.ctypes.data_as(C.c_void_p))
    np.testing.assert_array_equal(outs[0], host)
    glibc = np.array([math.acos(x) for x in u])
    print(f"device libm acos != glibc: {int((outs[1] != glibc).sum())}, != CR: {int((outs[1] != ref).sum())}; "
          f"glibc != CR: {int((glibc != ref).sum())} of {len(u)}")
