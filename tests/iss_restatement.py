"""CPU restatement of ISS keypoints (numpy only) and the seeded inputs its tests share.

The contract of include/m3d.h (Open3D 0.19 ``ComputeISSKeypoints``):

* sets: brute force, d² = (dx·dx + dy·dy) + dz·dz in fp64 (``clean_restatement.d2_rows``), strict
  ``<`` against the squared radius, the point itself included;
* radii: a zero radius replaces both by 6 and 4 times the model resolution, the sequential fp64 sum
  of sqrt(d² to the nearest other point) in index order, divided by n;
* covariance of S(i) centred on the query, d = pⱼ − pᵢ in fp64, the sums in EXTENDED precision
  (``np.longdouble`` with a 64-bit mantissa, otherwise ``fractions.Fraction``), rounded to fp64 once;
  ``np.linalg.eigvalsh`` of that;
* the saliency and non-maximum rules as written there, the same-set rule with TRUE set equality.

Beside the result, ``solve`` says which decisions a correct fp64 implementation may take either
way (``undecided``), with τᵢ = 1e-12·λ2(i).  A sequential fp64 sum of ``count`` products and a
backward-stable eigen-solve are off by at most about (count + 30)·2⁻⁵³·(trace + |m|²), which is
≤ 1e-13·λ2 for counts up to 100 (the measured order-to-order spread of the centred sums is
2.1e-15·λ2); 1e-12 leaves a factor 10 over that bound.

* a saliency test is undecided if |λ1 − γ21·λ2| ≤ 4τ, |λ0 − γ32·λ1| ≤ 4τ or |λ0| ≤ τ;
* a candidate i (third > 0) is undecided if some j ∈ N(i) has S(j) ≠ S(i) and either both are
  salient and |third[j] − third[i]| ≤ τᵢ + τⱼ, or j's saliency is undecided and
  λ0(j) ≥ third[i] − τᵢ − τⱼ.

The fixtures and parameter rows below are chosen so that ``undecided`` is empty
(tests/test_iss_cpu.py asserts it); a row that is not is given another seed or other parameters,
never another τ.
"""
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import clean_restatement as C

TAU = 1e-12
DEFAULT = (0.0, 0.0, 0.975, 0.975, 5)
ROWS = [DEFAULT, (0.2, 0.12, 0.6, 0.3, 20), (0.15, 0.2, 0.8, 0.1, 5), (0.1, 0.1, 0.975, 0.975, 12)]


def bumpy(seed, n):
    """A height field over [−1, 1]²: twelve Gaussian bumps and 0.002 of noise, around C.CENTRE."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-1.0, 1.0, (n, 2))
    centres = rng.uniform(-1.0, 1.0, (12, 2))
    heights = rng.uniform(0.1, 0.3, 12)
    widths = rng.uniform(0.08, 0.2, 12)
    z = np.zeros(n)
    for c, h, w in zip(centres, heights, widths):
        z = z + h * np.exp(-((xy - c) ** 2).sum(1) / (2.0 * w * w))
    z = z + 0.002 * rng.standard_normal(n)
    return np.ascontiguousarray(np.column_stack([xy, z]) + C.CENTRE)


FIXTURES = {
    "A": lambda: C.points("A"),
    "C": lambda: C.points("C"),
    "bumpy11": lambda: bumpy(11, 2500),
    "bumpy12_far": lambda: bumpy(12, 2000) + 500.0,
}
# fixture → the parameter rows it runs with (every fixture the defaults)
USED = {"A": [0, 1, 2, 3], "C": [0], "bumpy11": [0, 1, 2, 3], "bumpy12_far": [0]}


@lru_cache(maxsize=None)
def points(name):
    P = np.ascontiguousarray(FIXTURES[name]())
    P.setflags(write=False)
    return P


def in_radius(P, r):
    """n×n bool: d²(i, j) < r·r."""
    r2 = r * r
    M = np.empty((len(P), len(P)), bool)
    for i0 in range(0, len(P), 512):
        M[i0:i0 + 512] = C.d2_rows(P, np.arange(i0, min(i0 + 512, len(P)))) < r2
    return M


def nearest_other(P):
    """sqrt(d²) to the nearest other point (KDTreeFlann::SearchKNN(2), entry 1); n = 1: 0."""
    n = len(P)
    out = np.zeros(n)
    if n < 2:
        return out
    for i0 in range(0, n, 512):
        rows = np.arange(i0, min(i0 + 512, n))
        D = C.d2_rows(P, rows)
        D[np.arange(len(rows)), rows] = np.inf
        out[rows] = np.sqrt(D.min(1))
    return out


def model_resolution(P):
    """ComputeModelResolution: the sequential sum in index order, / n."""
    if len(P) == 0:
        return 0.0
    s = 0.0
    for v in nearest_other(P):
        s += float(v)
    return s / len(P)


def extended_ok():
    return np.finfo(np.longdouble).nmant >= 63


def cov_extended(d):
    """Covariance of the rows of d (fp64 differences to the query) about their mean, the sums in
    np.longdouble → 3×3 fp64."""
    assert extended_ok()
    x = d.astype(np.longdouble)
    k = np.longdouble(len(d))
    m = x.sum(0) / k
    S2 = x.T @ x
    return np.asarray(S2 / k - np.outer(m, m), np.float64)


def cov_fraction(d):
    """The same in exact rational arithmetic → 3×3 fp64 (each entry rounded once)."""
    k = len(d)
    F = [[Fraction(float(v)) for v in row] for row in d]
    s1 = [sum(r[a] for r in F) for a in range(3)]
    out = np.empty((3, 3))
    for a in range(3):
        for b in range(3):
            s2 = sum(r[a] * r[b] for r in F)
            out[a, b] = float(s2 / k - (s1[a] / k) * (s1[b] / k))
    return out


def covariance(d):
    return cov_extended(d) if extended_ok() else cov_fraction(d)


def set_ids(M):
    """An integer per row of the bool matrix M, equal exactly when the rows (the sets) are equal."""
    seen = {}
    return np.array([seen.setdefault(row.tobytes(), len(seen)) for row in np.packbits(M, axis=1)], np.int64)


def solve(P, rs, rn, g21, g32, mn):
    P = np.ascontiguousarray(P, np.float64)
    n = len(P)
    res = 0.0
    if rs == 0.0 or rn == 0.0:
        res = model_resolution(P)
        rs, rn = 6.0 * res, 4.0 * res
    out = SimpleNamespace(points=P, salient_radius=rs, non_max_radius=rn, resolution=res,
                          keypoints=np.zeros(0, np.int64), third=np.zeros(n), e1=np.zeros(n),
                          counts=np.zeros(n, np.int32), salient=np.zeros(n, bool), sal_undecided=np.zeros(n, bool),
                          same_set_keypoints=0, undecided=np.zeros(0, np.int64), num_salient=0, num_counted=0)
    if n == 0 or rs == 0.0 or rn == 0.0:
        return out
    S = in_radius(P, rs)
    N = S if rn == rs else in_radius(P, rn)
    counts = S.sum(1).astype(np.int32)
    sid = set_ids(S)
    lam = np.zeros((n, 3))
    third = np.zeros(n)
    salient = np.zeros(n, bool)
    sal_und = np.zeros(n, bool)
    by_set = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(n):
            if counts[i] < mn:
                continue
            Cm = covariance(P[np.flatnonzero(S[i])] - P[i])
            if (np.abs(Cm) <= 1e-12).all():  # Eigen's isZero
                continue
            l0, l1, l2 = np.linalg.eigvalsh(Cm)
            lam[i] = l0, l1, l2
            salient[i] = bool(l1 / l2 < g21 and l0 / l1 < g32)
            third[i] = l0 if salient[i] else 0.0
            t = TAU * l2
            sal_und[i] = abs(l1 - g21 * l2) <= 4 * t or abs(l0 - g32 * l1) <= 4 * t or abs(l0) <= t
    tau = TAU * lam[:, 2]
    cand = np.flatnonzero(third > 0.0)
    nn = N.sum(1)
    key, und, same = [], set(np.flatnonzero(sal_und).tolist()), 0
    for i in cand:
        nb = np.flatnonzero(N[i])
        other = nb[sid[nb] != sid[i]]
        if nn[i] >= mn and not (third[other] > third[i]).any():
            key.append(i)
            same += int(((sid[nb] == sid[i]) & (nb != i)).any())
        tt = tau[i] + tau[other]
        close = (third[other] > 0.0) & (np.abs(third[other] - third[i]) <= tt)
        loose = sal_und[other] & (lam[other, 0] >= third[i] - tt)
        if close.any() or loose.any():
            und.add(int(i))
    out.keypoints = np.array(key, np.int64)
    out.third, out.e1, out.counts, out.salient, out.sal_undecided = third, lam[:, 2].copy(), counts, salient, sal_und
    out.same_set_keypoints, out.undecided = same, np.array(sorted(und), np.int64)
    out.num_salient = int((third > 0.0).sum())
    out.num_counted = int((counts >= mn).sum())
    return out


@lru_cache(maxsize=None)
def case(name, row):
    """solve() of a fixture with ROWS[row] (computed once per session, never modified)."""
    return solve(points(name), *ROWS[row])
