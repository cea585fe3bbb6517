"""The point-to-mesh contract of csrc/mesh.hip restated in numpy (fp64, one operation at a time;
numpy does not fuse a product into a sum).

For a query p (optionally q64_of(T, p): ((T00·x + T01·y) + T02·z) + T03, …) and the triangles
(a, b, c) of a mesh: Ericson's closest point on a triangle, the seven Voronoi regions tested in the
order below, every dot product (x0*y0 + x1*y1) + x2*y2; d² = (dx·dx + dy·dy) + dz·dz with
d = point − p; the winner the smallest (d², triangle index) over the usable triangles (nine finite
coordinates, ab × ac not three exact zeros) whose d² is not NaN.  Region codes: 0 1 2 vertex a b c,
3 4 5 edge ab ac bc, 6 face.  uv = (v, w) with point ≈ (1−v−w)·a + v·b + w·c.
"""
import numpy as np

# the unit triangle the CPU and GPU tests share
A, B, Cc = (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)
TRI_V = np.array([A, B, Cc])
TRI_F = np.array([[0, 1, 2]])

# one query per Voronoi region of the triangle above, every number dyadic so each step is exact:
# (query, region, closest point, (v, w), d²)
REGION_CASES = [
    ((-1.0, -1.0, 0.0), 0, (0.0, 0.0, 0.0), (0.0, 0.0), 2.0),
    ((2.0, -0.5, 0.0), 1, (1.0, 0.0, 0.0), (1.0, 0.0), 1.25),
    ((-0.5, 2.0, 0.0), 2, (0.0, 1.0, 0.0), (0.0, 1.0), 1.25),
    ((0.5, -1.0, 2.0), 3, (0.5, 0.0, 0.0), (0.5, 0.0), 5.0),
    ((-1.0, 0.5, 0.0), 4, (0.0, 0.5, 0.0), (0.0, 0.5), 1.0),
    ((1.0, 1.0, 0.0), 5, (0.5, 0.5, 0.0), (0.5, 0.5), 0.5),
    ((0.25, 0.25, 3.0), 6, (0.25, 0.25, 0.0), (0.25, 0.25), 9.0),
]
# on a vertex, on an edge, in the face plane: d² is exactly zero
ZERO_CASES = [((1.0, 0.0, 0.0), 1), ((0.5, 0.0, 0.0), 3), ((0.25, 0.5, 0.0), 6)]


def q64_of(T, p):
    """The transformed queries in the library's operation order."""
    T = np.asarray(T, np.float64).reshape(4, 4)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    return np.stack([((T[k, 0] * p[:, 0] + T[k, 1] * p[:, 1]) + T[k, 2] * p[:, 2]) + T[k, 3] for k in range(3)],
                    axis=1)


def _dot(x, y):
    return (x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]


def closest_on_triangle(p, a, b, c):
    """closest(p, (a, b, c)) for queries p (n, 3) → (d2 (n,), point (n, 3), uv (n, 2), region (n,)).
    Every branch is evaluated for every query and the FIRST region whose test holds is taken, which
    is the device's early return."""
    p = np.asarray(p, np.float64).reshape(-1, 3)
    a, b, c = (np.asarray(x, np.float64).reshape(3) for x in (a, b, c))
    n = len(p)
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        zero, one = np.zeros(n), np.ones(n)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        s = (va + vb) + vc
        v_f, w_f = vb / s, vc / s
        cb = c - b
        cases = [
            ((d1 <= 0) & (d2 <= 0), np.broadcast_to(a, (n, 3)), zero, zero),
            ((d3 >= 0) & (d4 <= d3), np.broadcast_to(b, (n, 3)), one, zero),
            ((vc <= 0) & (d1 >= 0) & (d3 <= 0), a + ab * v_ab[:, None], v_ab, zero),
            ((d6 >= 0) & (d5 <= d6), np.broadcast_to(c, (n, 3)), zero, one),
            ((vb <= 0) & (d2 >= 0) & (d6 <= 0), a + ac * w_ac[:, None], zero, w_ac),
            ((va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0), b + cb * w_bc[:, None], 1.0 - w_bc, w_bc),
            (np.ones(n, bool), (a + ab * v_f[:, None]) + ac * w_f[:, None], v_f, w_f),
        ]
        codes = (0, 1, 3, 2, 4, 5, 6)  # the order of the tests: A, B, AB, C, AC, BC, face
        point = np.empty((n, 3))
        uv = np.empty((n, 2))
        region = np.full(n, -1, np.int64)
        for (cond, pt, v, w), code in zip(cases, codes):
            take = cond & (region < 0)
            point[take] = pt[take]
            uv[take, 0] = v[take]
            uv[take, 1] = w[take]
            region[take] = code
        d = point - p
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    return dd, point, uv, region.astype(np.uint8)


def usable(vertices, triangles):
    """(F,) bool: the triangles the search considers."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        cx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        cy = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        cz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
    fin = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    return fin & ~((cx == 0) & (cy == 0) & (cz == 0))


def per_triangle_d2(vertices, triangles, points, transformation=None):
    """(F, n) the d² of every query against every triangle (NaN rows for skipped triangles)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    q = np.asarray(points, np.float64).reshape(-1, 3)
    if transformation is not None:
        q = q64_of(transformation, q)
    ok = usable(v, t)
    out = np.full((len(t), len(q)), np.nan)
    for f in np.nonzero(ok)[0]:
        out[f] = closest_on_triangle(q, v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])[0]
    return out


def closest_points(vertices, triangles, points, transformation=None):
    """The whole contract → the dict m3d.mesh.closest_points returns.  ValueError for a mesh
    without a usable triangle."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    q = np.asarray(points, np.float64).reshape(-1, 3)
    if transformation is not None:
        q = q64_of(transformation, q)
    ok = usable(v, t)
    if not ok.any():
        raise ValueError("the mesh has no usable triangle")
    n = len(q)
    bd = np.full(n, np.inf)
    bt = np.full(n, -1, np.int32)
    bp = np.full((n, 3), np.nan)
    buv = np.full((n, 2), np.nan)
    br = np.full(n, 255, np.uint8)
    for f in np.nonzero(ok)[0]:  # ascending index: a strict < keeps the lower index on a tie
        d2, pt, uv, reg = closest_on_triangle(q, v[t[f, 0]], v[t[f, 1]], v[t[f, 2]])
        with np.errstate(invalid="ignore"):
            better = ~np.isnan(d2) & ((bt < 0) | (d2 < bd))
        bd[better], bt[better], bp[better], buv[better], br[better] = d2[better], f, pt[better], uv[better], reg[better]
    return {"d2": bd, "triangle": bt, "point": bp, "uv": buv, "region": br}
