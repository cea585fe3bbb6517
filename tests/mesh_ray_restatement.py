"""The ray-casting contract of csrc/mesh_ray.h restated in numpy (fp64, one operation at a time;
numpy does not fuse a product into a sum).

A ray is (o, d), six doubles; the test is the watertight test of Woop, Benthin and Wald (2013):
  per ray       kz = the axis of the largest |d| (the lowest axis wins a tie), kx = (kz+1)%3,
                ky = (kx+1)%3, swapped when d[kz] < 0; Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz].
  per triangle  A = a − o (B, C alike); Ax = A[kx] − Sx*A[kz], Ay = A[ky] − Sy*A[kz];
                U = Cx*By − Cy*Bx, V = Ax*Cy − Ay*Cx, W = Bx*Ay − By*Ax;
                miss if (U<0 || V<0 || W<0) && (U>0 || V>0 || W>0); det = (U+V)+W, miss if det == 0;
                Az = Sz*A[kz]; t = ((U*Az + V*Bz) + W*Cz) / det; hit iff tnear ≤ t ≤ tfar (NaN misses);
                (u, v) = (V/det, W/det): point ≈ (1−u−v)·a + u·b + v·c.
A ray with a component that is not finite or with d == 0 hits nothing; unusable triangles
(mesh_restatement.usable) are skipped.  First hit: the smallest (t, triangle); a miss gives t = +inf,
triangle −1, NaN uv.  Count: the usable triangles hit, int32.
"""
import numpy as np

from mesh_restatement import usable

CHUNK_PAIRS = 1 << 21  # (ray, triangle) pairs evaluated at a time


def _rays(rays):
    r = np.asarray(rays, np.float64)
    assert r.shape[-1] == 6
    return r.reshape(-1, 6), r.shape[:-1]


def ray_tri(rays, a, b, c, tnear=0.0, tfar=np.inf):
    """Rays (n, 6) against triangles a, b, c (F, 3) each → dict of (n, F) arrays: ``hit``, ``t``,
    ``u``, ``v`` and the three edge values ``U``, ``V``, ``W``."""
    rays = np.asarray(rays, np.float64).reshape(-1, 6)
    a, b, c = (np.asarray(x, np.float64).reshape(-1, 3) for x in (a, b, c))
    o, d = rays[:, :3], rays[:, 3:]
    n = len(rays)
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        ok = np.isfinite(rays).all(axis=1) & ~(d == 0.0).all(axis=1)
        kz = np.argmax(np.where(np.isnan(d), 0.0, np.abs(d)), axis=1)  # the first of equal maxima: the lowest axis
        kx = (kz + 1) % 3
        ky = (kx + 1) % 3
        neg = d[rows, kz] < 0.0
        kx, ky = np.where(neg, ky, kx), np.where(neg, kx, ky)
        dz = d[rows, kz]
        Sx, Sy, Sz = d[rows, kx] / dz, d[rows, ky] / dz, 1.0 / dz
        ox, oy, oz = o[rows, kx], o[rows, ky], o[rows, kz]

        def sheared(p):  # (F, 3) → the (n, F) sheared x, y and the raw z difference
            Pz = p[:, kz].T - oz[:, None]
            Px = (p[:, kx].T - ox[:, None]) - Sx[:, None] * Pz
            Py = (p[:, ky].T - oy[:, None]) - Sy[:, None] * Pz
            return Px, Py, Pz

        Ax, Ay, Akz = sheared(a)
        Bx, By, Bkz = sheared(b)
        Cx, Cy, Ckz = sheared(c)
        U = Cx * By - Cy * Bx
        V = Ax * Cy - Ay * Cx
        W = Bx * Ay - By * Ax
        miss = ((U < 0) | (V < 0) | (W < 0)) & ((U > 0) | (V > 0) | (W > 0))
        det = (U + V) + W
        miss |= det == 0.0
        Az, Bz, Cz = Sz[:, None] * Akz, Sz[:, None] * Bkz, Sz[:, None] * Ckz
        t = ((U * Az + V * Bz) + W * Cz) / det
        hit = ~miss & (tnear <= t) & (t <= tfar) & ok[:, None]
        u, v = V / det, W / det
    return {"hit": hit, "t": t, "u": u, "v": v, "U": U, "V": V, "W": W}


def _mesh(vertices, triangles):
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(triangles).reshape(-1, 3)
    ok = usable(v, f)
    if not ok.any():
        raise ValueError("the mesh has no usable triangle")
    idx = np.nonzero(ok)[0]
    return v[f[idx, 0]], v[f[idx, 1]], v[f[idx, 2]], idx


def cast_and_count(vertices, triangles, rays, tnear=0.0, tfar=np.inf):
    """One evaluation of every (ray, usable triangle) pair → (the dict m3d.raycast.cast_rays
    returns, the int32 counts m3d.raycast.count_intersections returns); leading shape kept."""
    a, b, c, idx = _mesh(vertices, triangles)
    r, lead = _rays(rays)
    n = len(r)
    t_hit = np.full(n, np.inf)
    tri = np.full(n, -1, np.int32)
    uv = np.full((n, 2), np.nan)
    count = np.zeros(n, np.int32)
    step = max(1, CHUNK_PAIRS // len(idx))
    for i0 in range(0, n, step):
        x = ray_tri(r[i0:i0 + step], a, b, c, tnear, tfar)
        t = np.where(x["hit"], x["t"], np.inf)
        # the smallest t, the lowest index among equals (argmin takes the first); a hit at t = +inf
        # still beats no hit
        j = np.argmin(t, axis=1)
        rows = np.arange(len(j))
        j = np.where(x["hit"][rows, j], j, np.argmax(x["hit"], axis=1))
        got = x["hit"][rows, j]
        sl = slice(i0, i0 + len(j))
        t_hit[sl] = np.where(got, x["t"][rows, j], np.inf)
        tri[sl] = np.where(got, idx[j], -1)
        uv[sl, 0] = np.where(got, x["u"][rows, j], np.nan)
        uv[sl, 1] = np.where(got, x["v"][rows, j], np.nan)
        count[sl] = x["hit"].sum(axis=1)
    first = {"t_hit": t_hit.reshape(lead), "triangle": tri.reshape(lead), "uv": uv.reshape(lead + (2,))}
    return first, count.reshape(lead)


def cast_rays(vertices, triangles, rays, tnear=0.0, tfar=np.inf):
    """The first hit of every ray → the dict m3d.raycast.cast_rays returns."""
    return cast_and_count(vertices, triangles, rays, tnear, tfar)[0]


def count_intersections(vertices, triangles, rays, tnear=0.0, tfar=np.inf):
    """The number of usable triangles every ray hits, int32."""
    return cast_and_count(vertices, triangles, rays, tnear, tfar)[1]


def edge_values(vertices, triangles, rays):
    """(n, F', 3) the edge values U, V, W of every ray against every usable triangle."""
    a, b, c, _ = _mesh(vertices, triangles)
    x = ray_tri(_rays(rays)[0], a, b, c, -np.inf, np.inf)
    return np.stack([x["U"], x["V"], x["W"]], axis=2)


_M64 = 0xFFFFFFFFFFFFFFFF


def _sample_key(seed, i):
    """sampler.h sample_base(seed, i) in Python integers."""
    z = ((seed & _M64) ^ ((i * 0x9E3779B97F4A7C15) & _M64)) + 0x9E3779B97F4A7C15 & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def occupancy_directions(nsamples):
    """(nsamples, 3) the fixed directions of compute_occupancy: component k of sample s is 2u − 1
    with u = (key >> 11)·2^-53, key = sample_base(0x6f6363, 3s + k)."""
    out = np.empty((nsamples, 3))
    for s in range(nsamples):
        for k in range(3):
            out[s, k] = 2.0 * ((_sample_key(0x6F6363, 3 * s + k) >> 11) * 2.0 ** -53) - 1.0
    return out


def icosphere(subdivisions=3):
    """A closed unit sphere mesh: an icosahedron subdivided `subdivisions` times (20·4^s triangles;
    3 → 1280), every vertex on the unit sphere, outward orientation, edges shared exactly."""
    p = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, p, 0), (1, p, 0), (-1, -p, 0), (1, -p, 0), (0, -1, p), (0, 1, p), (0, -1, -p), (0, 1, -p),
         (p, 0, -1), (p, 0, 1), (-p, 0, -1), (-p, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10),
         (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid = {}

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[key[0]] + v[key[1]]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]

        f = [t for a, b, c in f for t in ((a, m(a, b), m(c, a)), (b, m(b, c), m(a, b)), (c, m(c, a), m(b, c)),
                                          (m(a, b), m(b, c), m(c, a)))]
    return np.array(v), np.array(f, np.int32)


CUBE_V = np.array([(x, y, z) for z in (0.0, 1.0) for y in (0.0, 1.0) for x in (0.0, 1.0)])
# twelve triangles, outward, each face split along the diagonal through its lowest vertex
CUBE_F = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3],
                   [0, 4, 6], [0, 6, 2], [1, 3, 7], [1, 7, 5]], np.int32)


# ---- the one-triangle truth table the CPU and GPU tests share.  Every number is dyadic, so each
# step of the test is exact and the expected t is known without running anything.
TRI_V = np.array([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)])


def _perm(x, axis):
    """Coordinates rotated so that the triangle's normal (z) lies along `axis`."""
    x = np.asarray(x, np.float64)
    return np.roll(x.reshape(-1, 3), axis - 2, axis=1).reshape(x.shape)


def truth_table():
    """→ list of (label, vertices (3, 3), ray (6,), tnear, tfar, hit, t): one ray against one
    triangle, with the answer worked out by hand."""
    inf, nan = np.inf, np.nan
    down = (0.0, 0.0, -1.0)
    T = TRI_V
    cases = [
        ("interior", T, (0.25, 0.25, 1.0) + down, 0.0, inf, True, 1.0),
        ("edge ab", T, (0.5, 0.0, 1.0) + down, 0.0, inf, True, 1.0),
        ("edge ac", T, (0.0, 0.5, 1.0) + down, 0.0, inf, True, 1.0),
        ("edge bc", T, (0.5, 0.5, 1.0) + down, 0.0, inf, True, 1.0),
        ("vertex a", T, (0.0, 0.0, 1.0) + down, 0.0, inf, True, 1.0),
        ("vertex b", T, (1.0, 0.0, 2.0) + down, 0.0, inf, True, 2.0),
        ("just outside", T, (0.5, -2.0 ** -40, 1.0) + down, 0.0, inf, False, None),
        ("parallel above", T, (0.25, 0.25, 1.0, 1.0, 0.0, 0.0), 0.0, inf, False, None),
        ("in the plane (det == 0)", T, (-1.0, 0.25, 0.0, 1.0, 0.0, 0.0), 0.0, inf, False, None),
        ("behind the origin", T, (0.25, 0.25, 1.0, 0.0, 0.0, 1.0), 0.0, inf, False, None),
        ("behind, tnear = -2", T, (0.25, 0.25, 1.0, 0.0, 0.0, 1.0), -2.0, inf, True, -1.0),
        ("origin on the triangle", T, (0.25, 0.25, 0.0) + down, 0.0, inf, True, 0.0),
        ("flipped orientation", T[[0, 2, 1]], (0.25, 0.25, 1.0) + down, 0.0, inf, True, 1.0),
        ("from below", T, (0.25, 0.25, -1.0, 0.0, 0.0, 1.0), 0.0, inf, True, 1.0),
        ("direction of length 4", T, (0.25, 0.25, 1.0, 0.0, 0.0, -4.0), 0.0, inf, True, 0.25),
        ("d == 0", T, (0.25, 0.25, 1.0, 0.0, 0.0, 0.0), 0.0, inf, False, None),
        ("NaN origin", T, (nan, 0.25, 1.0) + down, 0.0, inf, False, None),
        ("NaN direction", T, (0.25, 0.25, 1.0, 0.0, nan, -1.0), 0.0, inf, False, None),
        ("inf direction", T, (0.25, 0.25, 1.0, 0.0, 0.0, -inf), 0.0, inf, False, None),
        ("inf origin", T, (0.25, 0.25, inf) + down, 0.0, inf, False, None),
        ("tfar == t", T, (0.25, 0.25, 1.0) + down, 0.0, 1.0, True, 1.0),
        ("tfar one ulp below t", T, (0.25, 0.25, 1.0) + down, 0.0, np.nextafter(1.0, 0.0), False, None),
        ("tnear == t", T, (0.25, 0.25, 1.0) + down, 1.0, inf, True, 1.0),
        ("tnear one ulp above t", T, (0.25, 0.25, 1.0) + down, np.nextafter(1.0, 2.0), inf, False, None),
        ("tnear > tfar", T, (0.25, 0.25, 1.0) + down, 2.0, 0.5, False, None),
    ]
    # every dominant axis with each sign, straight and slanted (Sx, Sy != 0: the kx / ky swap shows)
    for axis in range(3):
        for sign in (1.0, -1.0):
            tri = _perm(T, axis)
            for d in ((0.0, 0.0, -sign), (0.25, 0.5, -sign), (-0.5, 0.125, -2.0 * sign)):
                hitp = np.array((0.25, 0.5, 0.0))
                o = hitp - np.array(d)
                ray = np.concatenate([_perm(o, axis), _perm(d, axis)])
                cases.append((f"axis {axis} sign {sign:+.0f} d {d}", tri, tuple(ray), 0.0, inf, True, 1.0))
                miss = np.concatenate([_perm(o + (1.0, 0.0, 0.0), axis), _perm(d, axis)])
                cases.append((f"axis {axis} sign {sign:+.0f} d {d} beside", tri, tuple(miss), 0.0, inf, False, None))
    return [(lab, np.asarray(v, np.float64), np.asarray(r, np.float64), tn, tf, hit, t)
            for lab, v, r, tn, tf, hit, t in cases]
