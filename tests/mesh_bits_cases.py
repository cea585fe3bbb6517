"""The fixed cases whose raw output bits tests/golden/mesh_icp_bits.npz records, and the calls that
produce them: m3d_mesh_icp_run, m3d_mesh_icp_terms and m3d_mesh_closest (through m3d.mesh).

The fixture was recorded once (tools/gen_mesh_bits.py) from the build that still had a solve kernel,
a host-built state and two copies of the triangle sweep and box walk of its own in mesh_icp.hip;
test_gpu_mesh_icp.py asserts that the present build returns the same bits.

Inputs are made from an integer hash and from +, −, ·, / on float64 only (no random generator, no
libm call, no matrix product), so every machine and numpy version makes the same bits.

Shapes — the smallest at which the kernels take another path:
  triangles 1 (one grid cell: every point's box is the whole grid), TILE − 1, TILE, TILE + 1
      (TILE = kMeshBruteTile, the brute kernels' LDS tile);
  points 0, 1, 63, 64, 65 (a wave), SIDE + 1 (SIDE = kSideBlock, the terms pass's block; the scan
      kernels' block has the same size);
  triangle counts vary at 65 points, point counts at TILE + 1 triangles.
Every case runs on the brute-force path, the grid path and the grid path with seeds, which the
contract says return the same bits: the fixture holds them once, every variant is compared with it.
The loop cycles the kernel (L2, Tukey with k), the init (identity, within 1e-12 of it — not applied
to the points —, a rotation with a translation) and max_iteration (0, 30) over those shapes, and
runs all twelve combinations at TILE + 1 triangles and 65 points.  The distance query has one NaN
point.  (A NaN in a source cloud would first pass through the cloud's and the Morton grid's
construction, which this fixture is not about; the numpy restatement covers a NaN point of the loop.)
"""
import numpy as np

TILE = 256  # kMeshBruteTile (m3d_mesh_brute_tile)
SIDE = 256  # kSideBlock
TRIANGLES = (1, TILE - 1, TILE, TILE + 1)
POINTS = (0, 1, 63, 64, 65, SIDE + 1)
SHAPES = [(F, 65) for F in TRIANGLES] + [(TILE + 1, n) for n in POINTS if n != 65]
VARIANTS = (("brute", False), ("grid", False), ("grid", True))
TUKEY_K = 0.05

_C, _S = 0.9987502603949663, 0.04997916927067833  # cos, sin of 0.05 as literals
INITS = {
    "identity": np.eye(4),
    "near": np.array([[1.0, 5e-13, 0.0, -5e-13], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 5e-13], [0.0, 0.0, 0.0, 1.0]]),
    "rotation": np.array([[_C, -_S, 0.0, 0.01], [_S, _C, 0.0, -0.02], [0.0, 0.0, 1.0, 0.015], [0.0, 0.0, 0.0, 1.0]]),
}
_M = (1 << 64) - 1


def u01(shape, seed):
    """Uniform [0, 1) doubles of `shape` from splitmix64 of (seed, index): integer arithmetic only."""
    n = int(np.prod(shape))
    z = np.arange(1, n + 1, dtype=np.uint64) + np.uint64((seed * 0x632BE59BD9B4E019) & _M)
    z = z * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(shape)


def mesh_of(F):
    """F separate triangles in the unit cube, edges up to 0.3."""
    c = u01((F, 1, 3), 1000 + F)
    v = (c + (u01((F, 3, 3), 2000 + F) - 0.5) * 0.3).reshape(-1, 3)
    return np.ascontiguousarray(v), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def points_of(F, n):
    """Even points within 0.01 of a triangle, odd ones anywhere in [−0.2, 1.2]³."""
    v, f = mesh_of(F)
    a, b, c = (v[f[:, k]] for k in range(3))
    t = np.minimum((u01((n,), 3000 + F) * F).astype(np.int64), F - 1)
    w1 = u01((n, 1), 4000 + F)
    w2 = u01((n, 1), 5000 + F) * (1.0 - w1)
    near = ((1.0 - w1 - w2) * a[t] + w1 * b[t]) + w2 * c[t] + (u01((n, 3), 6000 + F) - 0.5) * 0.02
    box = u01((n, 3), 7000 + F) * 1.4 - 0.2
    return np.ascontiguousarray(np.where((np.arange(n) % 2 == 0)[:, None], near, box))


def seeds_of(F, n):
    """Seed triangles in [−1, F]: none, every triangle, and one index past the end."""
    return ((u01((n,), 8000 + F) * (F + 2)).astype(np.int64) - 1).astype(np.int32)


def radius_of(F):
    return 0.5 if F == 1 else 0.15


def run_cases():
    """→ [(key, F, n, kernel name, init name, max_iteration)]"""
    out = []
    for i, (F, n) in enumerate(SHAPES):
        out.append((f"run/F{F}_n{n}", F, n, ("l2", "tukey")[i % 2], ("identity", "near", "rotation")[i % 3],
                    0 if i % 4 == 1 else 30))
    for kern in ("l2", "tukey"):
        for init in INITS:
            for it in (0, 30):
                out.append((f"run/all_{kern}_{init}_{it}", TILE + 1, 65, kern, init, it))
    return out


def terms_cases():
    return [(f"terms/F{F}_n{n}", F, n, ("tukey", "l2")[i % 2], ("rotation", "identity", "near")[i % 3])
            for i, (F, n) in enumerate(SHAPES)]


def closest_cases():
    return [(f"closest/F{F}_n{n}", F, n, i % 2 == 0) for i, (F, n) in enumerate(SHAPES)]


def _loss(name):
    import matcher

    return matcher.TukeyLoss(TUKEY_K) if name == "tukey" else matcher.L2Loss()


def record(call):
    """Run every case of `call` ("run" | "terms" | "closest") on every variant → yields
    (key, variant name, {field: array}); the arrays hold the call's raw bits."""
    import m3d.mesh as M
    from m3d.core import Cloud

    if call == "run":
        for key, F, n, kern, init, it in run_cases():
            mesh, cloud = M.TriangleMesh(*mesh_of(F)), Cloud(points_of(F, n))
            for path, seed in VARIANTS:
                o = M.icp_to_mesh(cloud, mesh, radius_of(F), init=INITS[init], max_iteration=it, kernel=_loss(kern),
                                  path=path, seed=seed)
                tri = np.full(n, -1, np.int32)
                tri[o.correspondence_set[:, 0]] = o.correspondence_set[:, 1]
                yield key, f"{path}{' seeded' if seed else ''}", {
                    "T": o.transformation, "update": o.update, "fit_rmse": np.array([o.fitness, o.inlier_rmse]),
                    "counts": np.array([o.num_correspondences, o.iterations, int(o.converged)], np.int64), "tri": tri}
    elif call == "terms":
        for key, F, n, kern, init in terms_cases():
            mesh, cloud = M.TriangleMesh(*mesh_of(F)), Cloud(points_of(F, n))
            for path, seed in VARIANTS:
                s, t, d = M.icp_to_mesh_terms(cloud, mesh, INITS[init], radius_of(F), kernel=_loss(kern), path=path,
                                              seed_triangles=seeds_of(F, n) if seed else None)
                yield key, f"{path}{' seeded' if seed else ''}", {"sums": s, "tri": t, "d2": d}
    else:
        for key, F, n, moved in closest_cases():
            mesh, q = M.TriangleMesh(*mesh_of(F)), points_of(F, n)
            if n > 7:
                q[7, 1] = np.nan
            for path in ("brute", "grid"):
                o = M.closest_points(mesh, q, INITS["rotation"] if moved else None, path=path)
                yield key, path, {k: o[k] for k in ("d2", "triangle", "point", "uv", "region")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
