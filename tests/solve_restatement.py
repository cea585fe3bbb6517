"""Pure-Python restatement of the ICP device solve's device-only arithmetic (linalg.h sincos_small,
vec6_to_matrix_sc, matmul4_affine; icp.hip solve_state's bookkeeping) and its high-precision
references.  No GPU, no library: every function below computes in Python floats — IEEE binary64,
one correctly rounded operation per Python operator — in linalg.h's operation order, so its result
is what the gfx950 compile (built with -ffp-contract=off) must give bit for bit.  The mp_*
references work at 200 bits (mpmath)."""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -53  # unit roundoff of binary64


def fma(a, b, c):
    """a·b + c with one rounding (this interpreter has no math.fma): exact in rationals, then
    float(Fraction), which rounds to nearest even, subnormals included."""
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sincos_small(a):
    """linalg.h sincos_small: the two Horner chains in z = a², the same constants as the same
    double expressions, in the same order → (sin, cos)."""
    z = a * a
    ps = 1.0 / 355687428096000.0  # 1/17!
    ps = fma(ps, z, -1.0 / 1307674368000.0)
    ps = fma(ps, z, 1.0 / 6227020800.0)
    ps = fma(ps, z, -1.0 / 39916800.0)
    ps = fma(ps, z, 1.0 / 362880.0)
    ps = fma(ps, z, -1.0 / 5040.0)
    ps = fma(ps, z, 1.0 / 120.0)
    ps = fma(ps, z, -1.0 / 6.0)
    pc = 1.0 / 6402373705728000.0  # 1/18!
    pc = fma(pc, z, -1.0 / 20922789888000.0)
    pc = fma(pc, z, 1.0 / 87178291200.0)
    pc = fma(pc, z, -1.0 / 479001600.0)
    pc = fma(pc, z, 1.0 / 3628800.0)
    pc = fma(pc, z, -1.0 / 40320.0)
    pc = fma(pc, z, 1.0 / 720.0)
    pc = fma(pc, z, -1.0 / 24.0)
    pc = fma(pc, z, 0.5)
    return fma(a * z, ps, a), fma(-z, pc, 1.0)


def vec6_to_matrix_sc(x, ca, sa, cb, sb, cc, sc):
    """linalg.h vec6_to_matrix_sc: R = Rz·Ry·Rx as two 3×3 products, each entry (p0 + p1) + p2 with
    the factors that are exactly 0 or 1 written out, t = x[3..5] → 4×4 float64."""
    rx = [1.0, 0.0, 0.0, 0.0, ca, -sa, 0.0, sa, ca]
    ry = [cb, 0.0, sb, 0.0, 1.0, 0.0, -sb, 0.0, cb]
    rz = [cc, -sc, 0.0, sc, cc, 0.0, 0.0, 0.0, 1.0]
    zy = [0.0] * 9
    for i in range(3):
        for j in range(3):
            zy[i * 3 + j] = rz[i * 3 + 0] * ry[0 * 3 + j] + rz[i * 3 + 1] * ry[1 * 3 + j] + rz[i * 3 + 2] * ry[2 * 3 + j]
    T = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            T[i, j] = zy[i * 3 + 0] * rx[0 * 3 + j] + zy[i * 3 + 1] * rx[1 * 3 + j] + zy[i * 3 + 2] * rx[2 * 3 + j]
        T[i, 3] = float(x[3 + i])
    T[3, 3] = 1.0
    return T


def update_small(x):
    """vec6_to_matrix_wave's small-angle branch (max |x[0..2]| ≤ 0.5) for the solution x."""
    (sa, ca), (sb, cb), (sc, cc) = (sincos_small(float(x[k])) for k in range(3))
    return vec6_to_matrix_sc(x, ca, sa, cb, sb, cc, sc)


def matmul4_affine(A, B):
    """linalg.h matmul4_affine: C = A·B for affine 4×4, the sums left to right."""
    A = [[float(v) for v in r] for r in np.asarray(A)]
    B = [[float(v) for v in r] for r in np.asarray(B)]
    C = np.zeros((4, 4))
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j]
        C[i, 3] = A[i][0] * B[0][3] + A[i][1] * B[1][3] + A[i][2] * B[2][3] + A[i][3]
    C[3, 3] = 1.0
    return C


def p2p_translation(R, mp, mq, c):
    """solve_state's point-to-point translation in its order: t = (mq + c) − ((R0·w0 + R1·w1) +
    R2·w2), w = mp + c (mp, mq: the centred first moments over the count, c the source's centre)."""
    w = [float(mp[k]) + float(c[k]) for k in range(3)]
    return np.array([(float(mq[a]) + float(c[a])) -
                     (float(R[a][0]) * w[0] + float(R[a][1]) * w[1] + float(R[a][2]) * w[2]) for a in range(3)])


def new_state():
    """IcpState's bookkeeping fields after a reset (icp.hip reset_eval)."""
    return dict(evals=0, iters=0, done=0, converged=0, fitness=0.0, rmse=0.0, prev_fitness=0.0, prev_rmse=0.0,
                count=0)


def solve_bookkeeping(state, sums, params):
    """icp.hip solve_state without the algebra: fitness, rmse, the stop rule, iters, evals, done →
    (the new state, whether this evaluation applies an update).  params: relative_fitness,
    relative_rmse, max_iteration, ns (the fitness denominator: the source count, or
    set_source_total's).  A finished loop's solve changes nothing (solve_kernel returns)."""
    s = dict(state)
    if s["done"]:
        return s, False
    count = float(sums[28])
    fit = count / float(params["ns"]) if count > 0.0 else 0.0
    rmse = math.sqrt(float(sums[29]) / count) if count > 0.0 else 0.0
    stop = False
    if (s["evals"] > 0 and abs(s["prev_fitness"] - fit) < params["relative_fitness"]
            and abs(s["prev_rmse"] - rmse) < params["relative_rmse"]):
        s["converged"] = 1
        stop = True
    elif s["iters"] >= params["max_iteration"]:
        stop = True
    s["fitness"] = s["prev_fitness"] = fit
    s["rmse"] = s["prev_rmse"] = rmse
    s["count"] = int(count)
    s["evals"] += 1
    if stop:
        s["done"] = 1
        return s, False
    s["iters"] += 1
    return s, True


# ------------------------------------------------------------------------------- mp references
def _mp():
    import mpmath

    mpmath.mp.prec = 200
    return mpmath


def mp_solve(A, b):
    """x of A x = b by LU at 200 bits → a list of mpf."""
    mp = _mp()
    x = mp.lu_solve(mp.matrix([[mp.mpf(float(v)) for v in r] for r in np.asarray(A)]),
                    mp.matrix([mp.mpf(float(v)) for v in b]))
    return [x[k] for k in range(len(b))]


def mp_sincos(a):
    mp = _mp()
    return mp.sin(mp.mpf(a)), mp.cos(mp.mpf(a))


def ulps(got, ref):
    """|got − ref| in units of ref's last place as a binary64 (ref: mpf, not zero)."""
    mp = _mp()
    e = mp.frexp(ref)[1]  # |ref| in [2^(e−1), 2^e)
    ulp = mp.ldexp(mp.mpf(1), max(e - 53, -1074))
    return float(abs(mp.mpf(got) - ref) / ulp)


def mp_vec6_rotation(x):
    """Rz(x2)·Ry(x1)·Rx(x0) at 200 bits → mp 3×3."""
    mp = _mp()
    (sa, ca), (sb, cb), (sc, cc) = (mp_sincos(float(x[k])) for k in range(3))
    rx = mp.matrix([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = mp.matrix([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rz = mp.matrix([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz * ry * rx


def mp_max_abs_diff(M, ref):
    """max |M − ref| over a float64 array M and an mp matrix ref of the same shape → float."""
    mp = _mp()
    M = np.asarray(M)
    return float(max(abs(mp.mpf(float(M[i, j])) - ref[i, j]) for i in range(M.shape[0]) for j in range(M.shape[1])))


def mp_rotation_from_cov(H):
    """The proper rotation of rotation_from_cov's convention at 200 bits: H = Σ p qᵀ = U Σ Vᵀ
    (p source, q target), R = V·diag(1, 1, det(V Uᵀ))·Uᵀ maps source to target → mp 3×3."""
    mp = _mp()
    Hm = mp.matrix([[mp.mpf(float(v)) for v in r] for r in np.asarray(H).reshape(3, 3)])
    Um, _, Vt = mp.svd_r(Hm)  # H = Um·diag(S)·Vt, S descending
    V = Vt.T
    d = mp.det(V * Um.T)
    return V * mp.diag([1, 1, 1 if d > 0 else -1]) * Um.T
