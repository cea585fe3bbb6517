"""Fast Global Registration restated in numpy: fp64, the exact expression order of csrc/fgr.hip
(the contract is in include/m3d.h; the sum order in DESIGN.md §3.17).

Every operation is rounded on its own (numpy does not contract a·b + c), the sampler is
feat.hip's counter sampler, the solve is linalg.h's rule (unpivoted LDLᵀ while every pivot is safe,
else the pivoted one) transcribed operation for operation.  Against the device only libm's sin /
cos in vec6_to_matrix can differ (the device's are its own), so everything up to and including one
terms pass is bit-equal and the loop's trajectory agrees to a few ulps per iteration.

What a run records for the tests' preconditions: the smallest relative gap of the tuple
comparisons the sequential loop evaluated, the trial index of every accepted trial, and per
iteration par and whether the unpivoted solve held.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

SEG = 384    # m3d_internal.h kFgrSegRows
LANES = 64
MASK64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------- the sum order
def _tree(v):
    """The xor butterfly 32, 16, 8, 4, 2, 1 over axis 0 (64 entries)."""
    h = LANES // 2
    while h:
        v = v[:h] + v[h:]
        h //= 2
    return v[0]


def device_sum(x):
    """Σ over axis 0 in the device's order, a function of the count alone: segments of 384
    elements, lane l of 64 adding its six elements l + 64·k sequentially onto +0.0, a butterfly;
    then lane g adding the segment sums g, g + 64, … sequentially onto +0.0, a butterfly."""
    x = np.asarray(x, np.float64)
    n, tail = x.shape[0], x.shape[1:]
    if n == 0:
        return np.zeros(tail)
    nseg = -(-n // SEG)
    pad = np.zeros((nseg * SEG,) + tail)
    pad[:n] = x
    pad = pad.reshape((nseg, SEG // LANES, LANES) + tail)
    acc = np.zeros((nseg, LANES) + tail)
    for k in range(SEG // LANES):
        acc = acc + pad[:, k]
    seg = _tree(np.moveaxis(acc, 1, 0))             # (nseg,) + tail
    m = -(-nseg // LANES)
    pad2 = np.zeros((m * LANES,) + tail)
    pad2[:nseg] = seg
    pad2 = pad2.reshape((m, LANES) + tail)
    acc2 = np.zeros((LANES,) + tail)
    for j in range(m):
        acc2 = acc2 + pad2[j]
    return _tree(acc2)


def sequential_sum(x):
    x = np.asarray(x, np.float64)
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:])
    return np.cumsum(x, axis=0)[-1]


# ------------------------------------------------------------------------------- the sampler
def _splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(PHI)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def trial_rows(seed, h, n):
    """Rows of trials h (array): (len(h), 3) int64, three draws with replacement."""
    h = np.asarray(h, np.uint64)
    with np.errstate(over="ignore"):
        base = _splitmix64(np.uint64(seed & MASK64) ^ (h * np.uint64(PHI)))
        cols = [((_splitmix64(base + np.uint64(k)) >> np.uint64(32)) * np.uint64(n)) >> np.uint64(32) for k in range(3)]
    return np.stack(cols, axis=1).astype(np.int64)


# ------------------------------------------------------------------------------- normalise
@dataclass
class Normalised:
    mean_src: np.ndarray
    mean_tgt: np.ndarray
    scale: float
    g: float
    par0: float


def _norms(P):
    return np.sqrt((P[:, 0] * P[:, 0] + P[:, 1] * P[:, 1]) + P[:, 2] * P[:, 2])


def normalise(S, G, use_absolute_scale=False, sum=device_sum):
    S, G = np.asarray(S, np.float64).reshape(-1, 3), np.asarray(G, np.float64).reshape(-1, 3)
    m0, m1 = sum(S) / float(len(S)), sum(G) / float(len(G))
    scale = float(max(_norms(S - m0).max(), _norms(G - m1).max()))
    g, par0 = (1.0, scale) if use_absolute_scale else (scale, 1.0)
    return Normalised(m0, m1, scale, g, par0)


def gather(S, G, rows, nz):
    """The rows' normalised pairs: (S[i] − m0) / g, (G[j] − m1) / g."""
    rows = np.asarray(rows, np.int64).reshape(-1, 2)
    return (S[rows[:, 0]] - nz.mean_src) / nz.g, (G[rows[:, 1]] - nz.mean_tgt) / nz.g


# ------------------------------------------------------------------------------- tuple test
@dataclass
class Tuples:
    rows: np.ndarray       # (3·tuples,) row numbers of the input set
    tuples: int
    trials: int
    accepted: np.ndarray   # trial index of every accepted trial the sequential loop reached
    min_gap: float         # smallest relative gap of the comparisons it evaluated (inf: none)


def _edges(a, r):
    out = []
    for k in range(3):
        d = a[r[:, k]] - a[r[:, (k + 1) % 3]]
        out.append(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))
    return out


def _gap(a, b):
    """Relative gap of the comparison a < b; inf where both are exactly zero (0 < 0 is exact)."""
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(m == 0.0, np.inf, np.abs(a - b) / m)


def tuple_test(pr, qr, seed, tuple_scale, maximum_tuple_count, chunk=1 << 16):
    n = len(pr)
    cap = max(int(maximum_tuple_count), 1)
    total = 100 * n
    acc, min_gap, trials = [], np.inf, total
    have = 0
    for h0 in range(0, total, chunk):
        h = np.arange(h0, min(h0 + chunk, total), dtype=np.int64)
        r = trial_rows(seed, h, n)
        li, lj = _edges(pr, r), _edges(qr, r)
        ok = np.ones(len(h), bool)
        gaps = np.full(len(h), np.inf)
        for k in range(3):
            lo, hi = li[k] * tuple_scale, li[k] / tuple_scale
            ok &= (lo < lj[k]) & (lj[k] < hi)
            gaps = np.minimum(gaps, np.minimum(_gap(lo, lj[k]), _gap(lj[k], hi)))
        hit = np.flatnonzero(ok)
        if have + len(hit) >= cap:
            last = hit[cap - have - 1]
            acc.append(h[hit[: cap - have]])
            min_gap = min(min_gap, float(gaps[: last + 1].min()))
            trials = int(h[last]) + 1
            have = cap
            break
        acc.append(h[hit])
        have += len(hit)
        if len(h):
            min_gap = min(min_gap, float(gaps.min()))
    accepted = np.concatenate(acc) if acc else np.zeros(0, np.int64)
    rows = trial_rows(seed, accepted, n).reshape(-1) if len(accepted) else np.zeros(0, np.int64)
    return Tuples(rows, len(accepted), trials, accepted, min_gap)


# ------------------------------------------------------------------------------- the loop
def row_terms(p, q, par):
    """(n, 16): the distinct per-row terms of Σ s·J Jᵀ and Σ s·J r (fgr.hip row_terms)."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    r = p - q
    rx, ry, rz = r[:, 0], r[:, 1], r[:, 2]
    rr = (rx * rx + ry * ry) + rz * rz
    w = par / (rr + par)
    s = w * w
    return np.stack([s * (y * y + z * z), s * (x * y), s * (x * z), s * (x * x + z * z), s * (y * z),
                     s * (x * x + y * y), s * x, s * y, s * z, s,
                     s * (z * ry - y * rz), s * (x * rz - z * rx), s * (y * rx - x * ry),
                     s * rx, s * ry, s * rz], axis=1)


def expand_sums(S):
    """The 21 upper-triangle entries of JᵀJ (row-major) and the 6 of Jᵀr; a negative is 0 − S."""
    z = 0.0
    return np.array([S[0], z - S[1], z - S[2], z, z - S[8], S[7],
                     S[3], z - S[4], S[8], z, z - S[6],
                     S[5], z - S[7], S[6], z,
                     S[9], z, z, S[9], z, S[9],
                     S[10], S[11], S[12], z - S[13], z - S[14], z - S[15]], np.float64)


def terms27(p, q, par, sum=device_sum):
    return expand_sums(sum(row_terms(np.asarray(p, np.float64), np.asarray(q, np.float64), float(par))))


def ldlt6_solve_spd(A, b):
    """linalg.h ldlt6_solve_spd: (ok, x)."""
    M = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    dmax = 0.0
    for i in range(6):
        dmax = max(dmax, M[i][i]) if M[i][i] == M[i][i] else dmax  # fmax ignores a NaN
    lo = 1e-9 * dmax
    ok = dmax > 0.0 and math.isfinite(dmax)
    D, Di = [0.0] * 6, [0.0] * 6
    with np.errstate(all="ignore"):
        for k in range(6):
            D[k] = M[k][k]
            ok = ok and D[k] > lo
            Di[k] = float(np.float64(1.0) / np.float64(D[k]))
            for i in range(k + 1, 6):
                c = M[i][k]
                M[i][k] = c * Di[k]
                for j in range(k + 1, i + 1):
                    M[i][j] -= c * M[j][k]
    if not ok:
        return False, None
    y, x = [0.0] * 6, [0.0] * 6
    for i in range(6):
        s = float(b[i])
        for j in range(i):
            s -= M[i][j] * y[j]
        y[i] = s
    for i in range(5, -1, -1):
        s = y[i] * Di[i]
        for j in range(i + 1, 6):
            s -= M[j][i] * x[j]
        x[i] = s
    return True, x


def ldlt6_solve(A, b):
    """linalg.h ldlt6_solve (Eigen::LDLT's diagonal pivoting; a zero pivot gives a zero component)."""
    M = [[float(A[i][j]) for j in range(6)] for i in range(6)]
    L = [[1.0 if i == j else 0.0 for j in range(6)] for i in range(6)]
    D, y, perm = [0.0] * 6, [0.0] * 6, list(range(6))
    tiny = 2.2250738585072014e-308
    with np.errstate(all="ignore"):
        for k in range(6):
            p, best = k, abs(M[k][k])
            for i in range(k + 1, 6):
                if abs(M[i][i]) > best:
                    best, p = abs(M[i][i]), i
            if p != k:
                M[k], M[p] = M[p], M[k]
                for i in range(6):
                    M[i][k], M[i][p] = M[i][p], M[i][k]
                for j in range(k):
                    L[k][j], L[p][j] = L[p][j], L[k][j]
                perm[k], perm[p] = perm[p], perm[k]
            D[k] = M[k][k]
            ok = abs(D[k]) > tiny
            for i in range(k + 1, 6):
                L[i][k] = float(np.float64(M[i][k]) / np.float64(D[k])) if ok else 0.0
            for i in range(k + 1, 6):
                for j in range(k + 1, 6):
                    M[i][j] -= L[i][k] * M[k][j]
        for i in range(6):
            s = float(b[perm[i]])
            for j in range(i):
                s -= L[i][j] * y[j]
            y[i] = s
        for i in range(6):
            y[i] = float(np.float64(y[i]) / np.float64(D[i])) if abs(D[i]) > tiny else 0.0
        for i in range(5, -1, -1):
            s = y[i]
            for j in range(i + 1, 6):
                s -= L[j][i] * y[j]
            y[i] = s
    x = [0.0] * 6
    for i in range(6):
        x[perm[i]] = y[i]
    return x


def vec6_to_matrix(x):
    """linalg.h vec6_to_matrix_sc with libm's sin / cos."""
    ca, sa, cb, sb, cc, sc = math.cos(x[0]), math.sin(x[0]), math.cos(x[1]), math.sin(x[1]), math.cos(x[2]), math.sin(x[2])
    rx = [1.0, 0.0, 0.0, 0.0, ca, -sa, 0.0, sa, ca]
    ry = [cb, 0.0, sb, 0.0, 1.0, 0.0, -sb, 0.0, cb]
    rz = [cc, -sc, 0.0, sc, cc, 0.0, 0.0, 0.0, 1.0]
    zy = [rz[i * 3] * ry[j] + rz[i * 3 + 1] * ry[3 + j] + rz[i * 3 + 2] * ry[6 + j] for i in range(3) for j in range(3)]
    T = np.eye(4)
    for i in range(3):
        for j in range(3):
            T[i, j] = zy[i * 3] * rx[j] + zy[i * 3 + 1] * rx[3 + j] + zy[i * 3 + 2] * rx[6 + j]
        T[i, 3] = x[3 + i]
    return T


def matmul4_affine(A, B):
    C = np.eye(4)
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
        C[i, 3] = A[i, 0] * B[0, 3] + A[i, 1] * B[1, 3] + A[i, 2] * B[2, 3] + A[i, 3]
    return C


def solve_delta(S16):
    """(δ, spd_held): JᵀJ x = −Jᵀr by the ICP tail's rule; a non-finite δ is the identity."""
    e = expand_sums(S16)
    A = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for c in range(a, 6):
            A[a, c] = A[c, a] = e[k]
            k += 1
    b = [0.0 - e[21 + a] for a in range(6)]
    ok, x = ldlt6_solve_spd(A, b)
    if not ok:
        x = ldlt6_solve(A, b)
    try:
        d = vec6_to_matrix(x)
    except (ValueError, OverflowError):  # libm refuses inf / nan
        d = np.full((4, 4), np.nan)
    if not np.isfinite(d).all():
        d = np.eye(4)
    return d, ok


def move_points(d, q):
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    return np.stack([((d[i, 0] * x + d[i, 1] * y) + d[i, 2] * z) + d[i, 3] for i in range(3)], axis=1)


@dataclass
class Loop:
    T: np.ndarray
    par: float
    pars: list = field(default_factory=list)       # par used by each iteration
    spd: list = field(default_factory=list)        # the unpivoted solve held


def loop(p, q, par0, iteration_number=64, decrease_mu=False, maximum_correspondence_distance=0.025,
         division_factor=1.4, sum=device_sum):
    p, q = np.asarray(p, np.float64).reshape(-1, 3), np.asarray(q, np.float64).reshape(-1, 3).copy()
    out = Loop(np.eye(4), float(par0))
    if len(p) < 10:
        return out
    par = float(par0)
    with np.errstate(all="ignore"):
        for itr in range(int(iteration_number)):
            d, ok = solve_delta(sum(row_terms(p, q, par)))
            out.pars.append(par)
            out.spd.append(ok)
            out.T = matmul4_affine(d, out.T)
            q = move_points(d, q)
            if decrease_mu and itr % 4 == 0 and par > maximum_correspondence_distance:
                par = par / division_factor
    out.par = par
    return out


# ------------------------------------------------------------------------------- the pipeline
@dataclass
class Option:
    division_factor: float = 1.4
    use_absolute_scale: bool = False
    decrease_mu: bool = False
    maximum_correspondence_distance: float = 0.025
    iteration_number: int = 64
    tuple_scale: float = 0.95
    maximum_tuple_count: int = 1000
    tuple_test: bool = True
    seed: int | None = None


@dataclass
class Result:
    T: np.ndarray            # source → target, original scale
    T_norm: np.ndarray
    par_final: float
    rows: np.ndarray         # (n_rows, 2) the row set optimised over
    tuples: int
    trials: int
    nz: Normalised
    tup: Tuples | None
    lp: Loop


def original_scale(T, nz):
    """O = (R, ((−R·m1) + g·t) + m0) and the returned O⁻¹ = (Rᵀ, −Rᵀ·o) (api_prep.cpp's order)."""
    m0, m1 = nz.mean_src, nz.mean_tgt
    o = [((0.0 - ((T[i, 0] * m1[0] + T[i, 1] * m1[1]) + T[i, 2] * m1[2])) + nz.g * T[i, 3]) + m0[i] for i in range(3)]
    out = np.eye(4)
    for i in range(3):
        for j in range(3):
            out[i, j] = T[j, i]
        out[i, 3] = 0.0 - ((T[0, i] * o[0] + T[1, i] * o[1]) + T[2, i] * o[2])
    return out


def fgr(S, G, corres, option=None, sum=device_sum):
    """Steps 2–5 on the rows `corres` (n, 2)."""
    o = option or Option()
    S, G = np.asarray(S, np.float64).reshape(-1, 3), np.asarray(G, np.float64).reshape(-1, 3)
    corres = np.asarray(corres, np.int64).reshape(-1, 2)
    nz = normalise(S, G, o.use_absolute_scale, sum)
    with np.errstate(all="ignore"):
        pr, qr = gather(S, G, corres, nz)
        tup = None
        rows = corres
        if o.tuple_test:
            if len(corres):
                tup = tuple_test(pr, qr, 0 if o.seed is None else int(o.seed), o.tuple_scale, o.maximum_tuple_count)
            else:
                tup = Tuples(np.zeros(0, np.int64), 0, 0, np.zeros(0, np.int64), np.inf)
            rows = corres[tup.rows]
            pr, qr = pr[tup.rows], qr[tup.rows]
    lp = loop(pr, qr, nz.par0, o.iteration_number, o.decrease_mu, o.maximum_correspondence_distance,
              o.division_factor, sum)
    return Result(original_scale(lp.T, nz), lp.T, lp.par, rows, tup.tuples if tup else 0, tup.trials if tup else 0,
                  nz, tup, lp)


# ------------------------------------------------------------------------------- test scenes
def rotation(rx, ry, rz):
    return vec6_to_matrix([rx, ry, rz, 0.0, 0.0, 0.0])[:3, :3]


def scene(n=600, wrong=0.5, sigma=0.01, seed=1, nt_extra=0, pose=(0.3, -0.2, 0.4, 0.5, -0.3, 0.2)):
    """A source of n points in the unit ball's box, the target its posed copy (+ σ noise, + nt_extra
    unrelated points in front, so ns ≠ nt and j ≠ i), n rows of which a share `wrong` point at a
    random target.  Returns S, G, rows, T (source → target)."""
    rng = np.random.default_rng(seed)
    S = rng.uniform(-1.0, 1.0, (n, 3))
    T = np.eye(4)
    T[:3, :3] = rotation(*pose[:3])
    T[:3, 3] = pose[3:]
    G = S @ T[:3, :3].T + T[:3, 3] + rng.normal(0.0, sigma, (n, 3))
    if nt_extra:
        G = np.vstack([rng.uniform(-1.0, 1.0, (nt_extra, 3)), G])
    j = np.arange(n) + nt_extra
    bad = rng.random(n) < wrong
    j[bad] = rng.integers(0, len(G), int(bad.sum()))
    rows = np.column_stack([np.arange(n), j]).astype(np.int32)
    for a in (S, G, rows, T):
        a.setflags(write=False)
    return S, G, rows, T
