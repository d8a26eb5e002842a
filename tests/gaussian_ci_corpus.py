"""Gaussian conditional-independence tests (include/dvs_gaussian_ci.h; csrc/dvs_gaussian_ci.h): the cases, the numpy / Python
restatement of the header's definitions, the mpmath references and the checks that tests/test_emu_gaussian_ci.py and
tests/test_gpu_gaussian_ci.py run unchanged through the C ABI on their own back end (tests/scoring_corpus.py: EmuBackend,
GpuBackend).  The data sets, the exact moments and ``Reference`` (determinants, norms, the ln det bound) are those of
tests/gaussian_corpus.py; PC-stable and MMPC are restated by tests/pc_corpus.py (pc_ref, orient_ref) and tests/local_corpus.py
(mmpc_ref) over the restated tests.

References
  r, 1 - r^2   mpmath at 60 digits on the exact moments (gaussian_corpus.ExactMoments): r = -P_xy / sqrt(P_xx P_yy) with P the
               inverse of C[Z, x, y], and 1 - r^2 a second way, det C[Zxy] det C[Z] / (det C[Zx] det C[Zy]); the two routes are
               asserted to agree to 40 digits.  No Cholesky factor.
  statistics   the header's three formulae in mpmath.
  p-values     mpmath.betainc(df / 2, 1 / 2, 0, 1 - r^2, regularized=True) for cor (above 1 - r^2 = 1 / 2 as 1 - betainc(1 / 2,
               df / 2, 0, r^2) while that keeps 40 digits and by a positive series otherwise: mp_beta_tail), mpmath.erfc for zf and mi-g.

Tolerances.  None is fitted to a kernel's output.  u = 2^-53.
  1 - r^2      The computed squared pivot of the last row is exp(ln det^ C[Zxy] - ln det^ C[Zx]) and the computed q = l l + d_y^2
               is, within 2 u, the pivot y has in the factor of C[Z, y] (its row's first k entries come from the same operations),
               exp(ln det^ C[Zy] - ln det^ C[Z]).  With b(.) gaussian_corpus' bound on a computed ln det (Higham Thm 10.3 on the
               computed moments, kappa and the pivots from the mpmath reference, the input condition eta < 1/4 asserted):
                   |ln (1 - r^2)^ - ln (1 - r^2)| <= b(Zxy) + b(Zx) + b(Zy) + b(Z) + 4 u =: B.
  r            The computed factor is the exact factor of A + G, A = C[Zxy], ||G||_2 <= F (the same theorem, F3 of
               gaussian_corpus, which also covers the moments' error), so l / sqrt(l l + d_y^2) is exactly the partial
               correlation of A + G.  With P = A^-1, ||dP||_2 <= eta / (1 - eta) / sigma_min, eta = F / sigma_min, every entry
               of dP is below that, and P_xx, P_yy >= 1 / ||A||_2, so each of e_xy / sqrt(P_xx P_yy), e_xx / P_xx, e_yy / P_yy is
               at most tau = kappa eta / (1 - eta), and
                   |r^ - r| <= (|r| + tau) / (1 - tau) - |r| <= 2 tau / (1 - tau);   the four roundings after it add 4 u |r|.
               =: D (tau < 1e-3 asserted: the condition on the inputs).
  statistic    cor   t = r sqrt(df / (1 - r^2)):  |dt| <= 1.01 (sqrt(df / (1 - r^2)) D + |t| expm1(B / 2)) + 4 u |t|
               zf    z = atanh(r) sqrt(df), d atanh / dr = 1 / (1 - r^2) <= 1 / ((1 - r^2) - 2 D) on the interval (D < (1 - r^2) / 4
                     asserted):  |dz| <= sqrt(df) (D / ((1 - r^2) - 2 D) + 6 u (1 + |atanh r|))
               mi-g  s = -m ln(1 - r^2):  |ds| <= m (B + 2 u) + 4 u |s|
  p-value      p is monotone in |statistic|, so its change over the statistic's interval is the larger of |p(|s| - b) - p(s)|
               and |p(|s| + b) - p(s)|, both from mpmath: the statistic's bound times the p-value's condition number without the
               first-order remainder.  On top, the evaluation error of the tail: TAIL_RTOL[type] times p, measured as the error
               of the *restatement* (Python floats, math.lgamma / math.erfc / math.log) against mpmath at the exact statistic
               (tail_grid_error) over df in {1, 2, 3, 10, 126, 387, 5000} and r^2 from 1e-12 to 1 - 1e-9; the restatement is
               held to the measured value, the builds (the emulator's libm, the device's lgamma / erfc / log) to 4 times it,
               the factor and the reason of tests/pc_corpus.py.  Below 2^-1022 a p-value carries no relative error: that much is
               allowed absolutely, so such values compare as 0.
  guards       PC-stable and MMPC are compared exactly, after the restatement's own decisions are shown to be clear of the
               tolerance: every |p - alpha| / alpha and every max-min selection gap above GUARD_FACTOR * 4 * TAIL_RTOL.
Measured here (the restatement on the CPU; DESIGN.md §30 repeats them): TAIL_MEASURED.  On the pool of this file the largest
condition number of a C[Zxy] is 2.4e2, the restatement's largest statistic error / bound 1.2e-3 and p error / bound 5.3e-2."""
import ctypes
import functools
import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from dags_vae_search_amd import _lib as dl
from tests import gaussian_corpus as gc
from tests import local_corpus as lc
from tests import pc_corpus as pc

U64 = np.uint64
U = gc.U
NAN = gc.NAN
SENTINEL = gc.SENTINEL
TYPES = ("cor", "zf", "mi-g")
MAX_COND = dl.GCI_MAX_COND
P_FLOOR = 2.0 ** -1022
DPS_TAIL = 55                              # digits mp_beta_series sums to
ALPHA = 0.05
GUARD_FACTOR = 100
DATA_SHAPES = ((5, 129), (17, 389), (48, 389))
T_VALUES = (1, 63, 64, 65, 200)
E2E_SHAPES = ((5, 129), (8, 389), (17, 389))
# The largest relative error of the restatement's p-value against mpmath over the grid TAIL_DF x TAIL_R2 x both signs (336
# points a type), as measured on the CPU: tail_grid_error, which tests/test_gaussian_ci_ref.py runs again and holds to
# TAIL_RTOL, the measurement rounded up to two digits.  cor's is lgamma's (include/dvs_gaussian_ci.h): at df = 65 536, off the
# grid, the same measurement gives 3.55e-11.  zf's and mi-g's are the one rounding of the erfc argument times the statistic:
# p = 1e-300 has |z| = 37 and z^2 u = 1.5e-13.
TAIL_MEASURED = {"cor": 1.572e-12, "zf": 1.461e-13, "mi-g": 5.057e-14}
TAIL_RTOL = {"cor": 1.6e-12, "zf": 1.5e-13, "mi-g": 5.1e-14}
BUILD_FACTOR = 4
TAIL_DF = (1, 2, 3, 10, 126, 387, 5000)
TAIL_R2 = tuple([10.0 ** -e for e in range(12, 0, -1)] + [0.25, 0.5, 0.75] + [1.0 - 10.0 ** -e for e in range(1, 10)])


def type_id(typ):
    return dl.GCI_TYPES[typ]


# ---------------------------------------------------------------------------------------------------------------------
# The restatement of include/dvs_gaussian_ci.h in Python floats (every operation one rounding, in the header's order)
# ---------------------------------------------------------------------------------------------------------------------
def restated_beta_i(a, b, x, xc):
    if not x > 0.0:
        return 0.0
    if not xc > 0.0:
        return 1.0
    lead = math.exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log(xc))
    mirror = not x < (a + 1.0) / (a + b + 2.0)
    if mirror:
        a, b, x = b, a, xc
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < tiny:
        d = tiny
    d = 1.0 / d
    h = d
    for i in range(1, 20001):
        m = float(i)
        m2 = 2.0 * m
        an = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + an * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        h *= d * c
        an = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + an * d
        if abs(d) < tiny:
            d = tiny
        c = 1.0 + an / c
        if abs(c) < tiny:
            c = tiny
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-15:
            break
    v = lead * h / a
    return 1.0 - v if mirror else v


def _log_ratio(r):
    num, den = 1.0 + r, 1.0 - r
    if den == 0.0:
        return math.inf
    q = num / den
    return -math.inf if q == 0.0 else math.log(q)


def restated_cells(typ, m, k, l, d2):
    """(statistic, df, p) from the last row of the factor: l = L[y][x] and the last squared pivot"""
    ll = l * l
    q = ll + d2
    r = l / math.sqrt(q)
    omr = d2 / q
    if typ == "cor":
        df = m - float(k) - 2.0
        return r * math.sqrt(df / omr), df, restated_beta_i(0.5 * df, 0.5, omr, ll / q)
    if typ == "zf":
        df = m - float(k) - 3.0
        z = (0.5 * _log_ratio(r)) * math.sqrt(df)
        return z, df, math.erfc(abs(z) / 1.4142135623730951)
    s = -m * math.log(omr)
    return s, 1.0, math.erfc(math.sqrt(s / 2.0))


def restated_pair(mom, n, x, y, zm):
    """(k, m, l, d_y^2, r, 1 - r^2) of the header's factor of C[Z, x, y] from one set's moments, or None where a range check or
    the pivot rule refuses (the df rule is the caller's: it depends on the type)"""
    x, y, zm = int(x), int(y), int(zm)
    if not (0 <= x < n and 0 <= y < n) or x == y or zm >> n or (zm >> x) & 1 or (zm >> y) & 1:
        return None
    Z = gc.bits_of(zm)
    k = len(Z)
    if k > MAX_COND:
        return None
    m = float(mom[0])
    C = np.asarray(mom[1 + n:]).reshape(n, n)
    a = Z + [x, y]
    L = np.zeros((k + 2, k + 2))
    for i in range(k + 2):
        for j in range(i):
            s = float(C[a[i], a[j]])
            for t in range(j):
                s = s - float(L[i, t]) * float(L[j, t])
            L[i, j] = s / float(L[j, j])
        diag = float(C[a[i], a[i]])
        s = diag
        for t in range(i):
            s = s - float(L[i, t]) * float(L[i, t])
        if not (math.isfinite(s) and s > ((k + 3) * 2.0 ** -52) * diag):
            return None
        L[i, i] = math.sqrt(s)
    l, d2 = float(L[k + 1, k]), s
    q = l * l + d2
    return k, m, l, d2, l / math.sqrt(q), d2 / q


def restated_test(mom, n, x, y, zm, typ):
    """the three cells of dvs_gbn_ci_tests for one test, NaNs for a refused one"""
    f = restated_pair(mom, n, x, y, zm)
    if f is None or f[1] - f[0] - (3.0 if typ == "zf" else 2.0) < 1.0:
        return (NAN, NAN, NAN)
    return restated_cells(typ, f[1], f[0], f[2], f[3])


# ---------------------------------------------------------------------------------------------------------------------
# mpmath: the cells from (l, d_y^2) or (r, 1 - r^2), the tail grid
# ---------------------------------------------------------------------------------------------------------------------
def mp_beta_series(a, b, x, xc):
    """I_x(a, b) = x^a xc^b / (a B(a, b)) * sum_n prod_(i<n) (a + b + i) / (a + 1 + i) x^n (DLMF 8.17.8 with 2F1(a + b, 1; a + 1; x)):
    every term positive, so no cancellation at any a; the terms fall like x^n and the tail after t_n is below t_n / xc"""
    total, term, n = mp.mpf(0), mp.mpf(1), 0
    while term / xc > total * mp.mpf(10) ** -(DPS_TAIL):
        total += term
        term *= (a + b + n) / (a + 1 + n) * x
        n += 1
    return mp.exp(a * mp.log(x) + b * mp.log(xc) + mp.loggamma(a + b) - mp.loggamma(a) - mp.loggamma(b)) / a * total


def mp_beta_tail(df, x, xc):
    """I_x(df / 2, 1 / 2) with xc = 1 - x given exactly.  mpmath.betainc up to x = 1 / 2.  Above, its series fails to converge
    next to x = 1 at large df, so the reflection I_x(a, b) = 1 - I_xc(b, a) is taken; at 60 digits the subtraction keeps 40 of
    them while p > 1e-20, and a smaller p (large df, x clear of 1) is summed by mp_beta_series, which
    tests/test_gaussian_ci_ref.py holds against mpmath.betainc where both work."""
    a, b = mp.mpf(df) / 2, mp.mpf(1) / 2
    if x <= b:
        return mp.betainc(a, b, 0, x, regularized=True)
    p = 1 - mp.betainc(b, a, 0, xc, regularized=True)
    return p if p > mp.mpf("1e-20") else mp_beta_series(a, b, x, xc)


@gc.at60
def exact_p(typ, df, stat):
    """the p-value as a function of the statistic (mpmath): what the bound differentiates"""
    stat = abs(mp.mpf(stat))
    if typ == "cor":
        return mp_beta_tail(df, df / (df + stat * stat), stat * stat / (df + stat * stat))
    if typ == "zf":
        return mp.erfc(stat / mp.sqrt(2))
    return mp.erfc(mp.sqrt(stat / 2))


@gc.at60
def exact_cells(typ, m, k, r, omr):
    """(statistic, df, p) in mpmath from r and 1 - r^2"""
    if typ == "cor":
        df = m - k - 2
        return r * mp.sqrt(df / omr), df, mp_beta_tail(df, omr, r * r)
    if typ == "zf":
        df = m - k - 3
        z = mp.atanh(r) * mp.sqrt(df)
        return z, df, mp.erfc(abs(z) / mp.sqrt(2))
    s = -m * mp.log(omr)
    return s, 1, mp.erfc(mp.sqrt(s / 2))


@gc.at60
def tail_grid_error(typ, dfs=TAIL_DF, r2s=TAIL_R2):
    """The evaluation error of the restatement's tail: its p-value against mpmath *at the exact statistic*, over the grid, k = 0.
    For zf and mi-g that is the float statistic the restatement itself computed.  cor's tail is given the two floats 1 - r^2 and
    r^2, each accurate for its own quantity but not summing to 1 (at r^2 = 1e-12 the float 1 - r^2 alone knows r^2 to four
    digits), so its exact argument is d_y^2 / (l l + d_y^2) in mpmath at the floats (l, d_y^2).
    -> (largest relative p error where p >= 2^-1022, the largest absolute p error below that, points, and for information the
    largest relative error of the statistic against mpmath at the floats (l, d_y^2): what 1 - r costs zf near |r| = 1, which
    the statistic's derived bound covers through D / (1 - r^2))"""
    worst_p, worst_s, tiny, points = 0.0, 0.0, 0.0, 0
    for df in dfs:
        m = float(df + (3 if typ == "zf" else 2))
        for r2 in r2s:
            for sign in (1.0, -1.0):
                l, d2 = sign * math.sqrt(r2), 1.0 - r2
                stat, got_df, got_p = restated_cells(typ, m, 0, l, d2)
                assert got_df == (1 if typ == "mi-g" else df)
                if typ == "cor":
                    ll, q = mp.mpf(l) * mp.mpf(l), mp.mpf(l) * mp.mpf(l) + mp.mpf(d2)
                    want_p = mp_beta_tail(df, mp.mpf(d2) / q, ll / q)
                else:
                    want_p = exact_p(typ, df, stat)
                if want_p >= P_FLOOR:
                    worst_p = max(worst_p, float(abs(mp.mpf(got_p) - want_p) / want_p))
                else:
                    tiny = max(tiny, float(abs(mp.mpf(got_p) - want_p)))
                q = mp.mpf(l) * mp.mpf(l) + mp.mpf(d2)
                want_stat = exact_cells(typ, int(m), 0, mp.mpf(l) / mp.sqrt(q), mp.mpf(d2) / q)[0]
                worst_s = max(worst_s, float(abs(mp.mpf(stat) - want_stat) / abs(want_stat)))
                points += 1
    return worst_p, tiny, points, worst_s


# ---------------------------------------------------------------------------------------------------------------------
# mpmath on the exact moments: one test's r, 1 - r^2 and the ingredients of its bounds
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data_reference(n, S):
    return gc.reference_of(n, S)


class PairReference(SimpleNamespace):
    """r, omr (mpf); B, D (floats; module docstring); kappa of C[Zxy]"""


_PAIRS = {}


@gc.at60
def pair_reference(ref, key, x, y, Z):
    """the reference of the test (x, y | Z) on gaussian_corpus.Reference ``ref``, cached under (key, x, y, Z)"""
    Z = sorted(int(z) for z in Z)
    ck = (key, x, y, tuple(Z))
    if ck in _PAIRS:
        return _PAIRS[ck]
    idx = Z + [x, y]
    q = len(idx)
    P = ref.sub(idx, mp.mpf(0)) ** -1
    r = -P[q - 2, q - 1] / mp.sqrt(P[q - 2, q - 2] * P[q - 1, q - 1])
    ld = lambda s: ref.facts(s, 0.0)[0]
    omr = mp.exp(ld(idx) - ld(Z + [x]) - ld(Z + [y]) + ld(Z))
    assert abs((1 - r * r) - omr) < mp.mpf(10) ** -40, (x, y, Z)
    B = sum(ref.logdet_bound(s, 0.0) for s in (idx, Z + [x], Z + [y], Z)) + 4 * U
    F3, smin = ref.logdet_bound(idx, 0.0, solve=True)
    kappa = float(ref.facts(idx, 0.0)[1]) / smin
    eta = F3 / smin
    tau = kappa * eta / (1 - eta)
    assert tau < 1e-3, ("tau", x, y, Z, tau)
    D = 2 * tau / (1 - tau) + 4 * U * float(abs(r))
    assert D < float(omr) / 4, ("D", x, y, Z, D, float(omr))
    _PAIRS[ck] = PairReference(r=r, omr=omr, B=B, D=D, kappa=kappa)
    return _PAIRS[ck]


@gc.at60
def reference_cells(pr, typ, m, k, tail_rtol):
    """((statistic, df, p) in mpmath, the statistic's bound, the p-value's bound) of one test; None where df < 1"""
    df = m - k - (3 if typ == "zf" else 2)
    if df < 1:
        return None
    stat, df, p = exact_cells(typ, m, k, pr.r, pr.omr)
    omr, a = float(pr.omr), float(abs(stat))
    if typ == "cor":
        bound = 1.01 * (math.sqrt(df / omr) * pr.D + a * math.expm1(pr.B / 2)) + 4 * U * a
    elif typ == "zf":
        bound = math.sqrt(df) * (pr.D / (omr - 2 * pr.D) + 6 * U * (1 + float(abs(mp.atanh(pr.r)))))
    else:
        bound = m * (pr.B + 2 * U) + 4 * U * a
    lo, hi = exact_p(typ, df, max(a - bound, 0.0)), exact_p(typ, df, a + bound)
    p_bound = float(max(abs(lo - p), abs(hi - p))) + tail_rtol * float(p) + P_FLOOR
    return (stat, df, p), bound, p_bound


def assert_cells(got, want, what):
    """got: three floats; want: reference_cells' return -> (statistic error / bound, p error / bound)"""
    (stat, df, p), sb, pb = want
    assert got[1] == df, (what, "df", got[1], df)
    es, ep = float(abs(mp.mpf(float(got[0])) - stat)), float(abs(mp.mpf(float(got[2])) - p))
    assert es <= sb, (what, "statistic", float(got[0]), float(stat), es, sb)
    assert ep <= pb, (what, "p", float(got[2]), float(p), ep, pb)
    return es / sb, ep / pb


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(n):
    """the reference tests of a data set: [(x, y, Z)], k in {0, 1, 2, 10} as far as n has the variables, x above, below and
    between the members of Z, the last variable on every side; the k = 10 tests share one Z so that its factor is cached"""
    rng = np.random.default_rng(3000 + n)
    tests = []
    for k in (0, 1, 2, 10):
        if k + 2 > n:
            continue
        count = 2 if k == 10 else 6
        Z10 = sorted(int(v) for v in rng.choice(n - 1, size=k, replace=False)) if k == 10 else None
        for c in range(count):
            Z = Z10 if k == 10 else sorted(int(v) for v in rng.choice(n, size=k, replace=False))
            rest = [v for v in range(n) if v not in Z]
            x, y = (int(v) for v in rng.choice(rest, size=2, replace=False))
            if c == 0 and n - 1 in rest and y != n - 1:
                x = n - 1                                    # the last variable as x ...
            if c == 1 and n - 1 in rest and x != n - 1:
                y = n - 1                                    # ... and as y
            tests.append((x, y, tuple(Z)))
    if n == 5:
        tests += [(0, 1, (2, 3, 4)), (4, 0, (1, 2, 3))]      # k = n - 2: every variable is in the test
    return tests


def cycled(tests, T):
    return [tests[t % len(tests)] for t in range(T)]


def short_rows():
    """four distinct rows of gauss_data(5, 129): with k = 1, cor has df = 1 and zf has df = 0"""
    return np.asarray([[3, 40, 77, 120]], np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI on a back end
# ---------------------------------------------------------------------------------------------------------------------
def run_ci(be, mom, n, tests, typ, set_of=None, guard=0):
    """dvs_gbn_ci_tests over tests [(x, y, Z or mask)] -> (out [T, 3], status); ``guard`` rows of sentinels around out must survive"""
    T = len(tests)
    pairs = np.asarray([[t[0], t[1]] for t in tests], np.int32).reshape(T, 2)
    cond = np.asarray([t[2] if isinstance(t[2], (int, np.integer)) else gc.mask_of(t[2]) for t in tests], U64)
    out, status = be.put(np.full((T + 2 * guard, 3), SENTINEL)), be.put(np.zeros(1, np.int32))
    op = ctypes.c_void_p(be.ptr(out).value + guard * 24)
    gc.call(be, "dvs_gbn_ci_tests", n_tests=T, n_vars=n, moments=be.put(mom), n_sets=len(mom),
            set_of=None if set_of is None else be.put(np.asarray(set_of, np.int32)), pairs=be.put(pairs), cond=be.put(cond),
            test_type=type_id(typ), out=op, out_bytes=T * 24, status=status)
    o = np.array(be.get(out), copy=True)
    if guard:
        assert (o[:guard] == SENTINEL).all() and (o[T + guard:] == SENTINEL).all()
    return o[guard:T + guard], int(be.get(status)[0])


def run_group(be, mom, n, groups, typ, set_of=None, guard=0):
    """dvs_gbn_ci_tests_group over groups [(target, Z or mask, candidates mask)] -> (out [G, n, 3], status)"""
    G = len(groups)
    target = np.asarray([g[0] for g in groups], np.int32)
    cond = np.asarray([g[1] if isinstance(g[1], (int, np.integer)) else gc.mask_of(g[1]) for g in groups], U64)
    cand = np.asarray([g[2] for g in groups], U64)
    out, status = be.put(np.full((G + 2 * guard, n, 3), SENTINEL)), be.put(np.zeros(1, np.int32))
    op = ctypes.c_void_p(be.ptr(out).value + guard * n * 24)
    gc.call(be, "dvs_gbn_ci_tests_group", n_groups=G, n_vars=n, moments=be.put(mom), n_sets=len(mom),
            set_of=None if set_of is None else be.put(np.asarray(set_of, np.int32)), target=be.put(target), cond=be.put(cond),
            candidates=be.put(cand), test_type=type_id(typ), out=op, out_bytes=G * n * 24, status=status)
    o = np.array(be.get(out), copy=True)
    if guard:
        assert (o[:guard] == SENTINEL).all() and (o[G + guard:] == SENTINEL).all()
    return o[guard:G + guard], int(be.get(status)[0])


# ---------------------------------------------------------------------------------------------------------------------
# Checks
# ---------------------------------------------------------------------------------------------------------------------
def check_restatement(n, S):
    """the restatement on the restated moments against mpmath on the exact ones, every pool test and type, held to the
    measured tail error -> (cases, worst statistic error / bound, worst p error / bound, largest kappa)"""
    mom = gc.restated_moments(gc.gauss_data(n, S))
    ref = data_reference(n, S)
    cases, ws, wp, kappa = 0, 0.0, 0.0, 0.0
    for x, y, Z in pool(n):
        pr = pair_reference(ref, (n, S), x, y, Z)
        kappa = max(kappa, pr.kappa)
        for typ in TYPES:
            want = reference_cells(pr, typ, S, len(Z), TAIL_RTOL[typ])
            assert want is not None
            es, ep = assert_cells(restated_test(mom[0], n, x, y, gc.mask_of(Z), typ), want, (n, S, x, y, Z, typ))
            cases, ws, wp = cases + 1, max(ws, es), max(wp, ep)
    assert cases == len(pool(n)) * len(TYPES), "no case is left out for conditioning"
    return cases, ws, wp, kappa


def check_against_mpmath(be, n, S, T):
    """T tests (the pool, cycled) of every type through dvs_gbn_ci_tests: two runs of equal bytes, sentinels around the buffer,
    every cell within its bound -> (worst statistic error / bound, worst p error / bound)"""
    mom = gc.run_moments(be, gc.gauss_data(n, S))
    ref = data_reference(n, S)
    tests = cycled(pool(n), T)
    ws, wp = 0.0, 0.0
    for typ in TYPES:
        out, status = run_ci(be, mom, n, tests, typ, guard=1)
        again, _ = run_ci(be, mom, n, tests, typ)
        assert status == 0 and out.tobytes() == again.tobytes(), (n, S, T, typ)
        for t, (x, y, Z) in enumerate(tests):
            if t >= len(pool(n)):                            # a repeat of the pool: the bytes of its first occurrence
                assert out[t].tobytes() == out[t % len(pool(n))].tobytes(), (typ, t)
                continue
            want = reference_cells(pair_reference(ref, (n, S), x, y, Z), typ, S, len(Z), BUILD_FACTOR * TAIL_RTOL[typ])
            es, ep = assert_cells(out[t], want, (n, S, T, t, x, y, Z, typ))
            ws, wp = max(ws, es), max(wp, ep)
    return ws, wp


def check_short_set(be):
    """S = 4 through a row set, k = 1: cor has df = 1 (against mpmath), mi-g goes by cor's rule, zf is refused"""
    x = gc.gauss_data(5, 129)
    rows = short_rows()
    mom = gc.run_moments(be, x, rows)
    gathered = np.ascontiguousarray(x[rows[0]])
    ref = gc.Reference(gc.ExactMoments(gathered), gc.restated_moments(gathered)[0, 1:6])
    tests = [(0, 1, (2,)), (3, 4, (0,)), (2, 0, ())]
    for typ in TYPES:
        out, status = run_ci(be, mom, 5, tests, typ, guard=1)
        for t, (a, b, Z) in enumerate(tests):
            want = reference_cells(pair_reference(ref, "short", a, b, Z), typ, 4, len(Z), BUILD_FACTOR * TAIL_RTOL[typ])
            if typ == "zf" and len(Z) == 1:
                assert want is None and np.isnan(out[t]).all()
                continue
            assert_cells(out[t], want, ("short", typ, t))
            if typ == "cor" and len(Z) == 1:
                assert out[t, 1] == 1.0
        assert status == (16 if typ == "zf" else 0)
        rest = [restated_test(gc.restated_moments(gathered)[0], 5, a, b, gc.mask_of(Z), typ) for a, b, Z in tests]
        assert np.array_equal(np.isnan(np.asarray(rest)), np.isnan(out))
    # two rows fewer: m = 2 leaves cor and mi-g no degree of freedom even without conditioning
    mom2 = gc.run_moments(be, x, rows[:, :2])
    for typ in TYPES:
        out, status = run_ci(be, mom2, 5, [(0, 1, ())], typ)
        assert status == 16 and np.isnan(out).all()
    mom3 = gc.run_moments(be, x, rows[:, :3])
    for typ in TYPES:
        out, status = run_ci(be, mom3, 5, [(0, 1, ())], typ)
        assert (status == 16 and np.isnan(out).all()) if typ == "zf" else (status == 0 and not np.isnan(out).any()), typ


def refusal_cases():
    """[(name, data key, n, (x, y, Z mask), the types that refuse it)]"""
    every = TYPES
    return [
        ("x = y", "x17", 17, (3, 3, 0), every),
        ("x in Z", "x17", 17, (3, 4, gc.mask_of([3, 5])), every),
        ("y in Z", "x17", 17, (3, 4, gc.mask_of([4])), every),
        ("x = n", "x17", 17, (17, 4, 0), every),
        ("y = -1", "x17", 17, (3, -1, 0), every),
        ("x = -1", "x17", 17, (-1, 3, 0), every),
        ("cond bit n", "x17", 17, (3, 4, 1 << 17), every),
        ("cond bit 63", "x17", 17, (3, 4, 1 << 63), every),
        ("k = cap", "x17", 17, (15, 16, gc.mask_of(range(MAX_COND))), ()),
        ("k = cap + 1", "x17", 17, (15, 16, gc.mask_of(range(MAX_COND + 1))), every),
        ("bit 47", "x48", 48, (0, 46, 1 << 47), ()),
        ("x = 47", "x48", 48, (47, 0, gc.mask_of([46, 1])), ()),
        ("duplicated columns in Z", "deg", 5, (0, 2, gc.mask_of([1, 3])), every),
        ("x duplicates a member of Z", "deg", 5, (3, 0, gc.mask_of([1])), every),
        ("y duplicates x", "deg", 5, (1, 3, 0), every),
        ("y is a combination of Z and x", "deg", 5, (2, 4, gc.mask_of([0])), every),
        ("x is a combination of Z", "deg", 5, (4, 1, gc.mask_of([0, 2])), every),
        ("neither", "deg", 5, (0, 1, gc.mask_of([2])), ()),
    ]


def check_refusals(be):
    """every refusal rule alone, as the middle test of three between sentinels: NaN and bit 4 for it, the neighbours' bytes
    untouched; the restatement refuses the same tests; the grouped call refuses the same cells"""
    data = {"x17": gc.gauss_data(17, 389), "x48": gc.gauss_data(48, 389), "deg": gc.degenerate_data()}
    moms = {k: gc.run_moments(be, v) for k, v in data.items()}
    for name, key, n, (x, y, zm), refusing in refusal_cases():
        mom = moms[key]
        around = [(0, 1, 0), (2, 0, gc.mask_of([1]))]
        for typ in TYPES:
            alone, st0 = run_ci(be, mom, n, around, typ)
            assert st0 == 0 and not np.isnan(alone).any()
            out, status = run_ci(be, mom, n, [around[0], (x, y, zm), around[1]], typ, guard=1)
            refused = typ in refusing
            assert np.isnan(out[1]).all() == refused and (refused or not np.isnan(out[1]).any()), (name, typ, out[1])
            assert status == (16 if refused else 0), (name, typ, status)
            assert out[[0, 2]].tobytes() == alone.tobytes(), (name, typ)
            assert math.isnan(restated_test(mom[0], n, x, y, zm, typ)[0]) == refused, (name, typ)
            if 0 <= y < n:
                # the same test as a grouped cell, between a group that asks nothing and a sound one
                grp, gst = run_group(be, mom, n, [(0, 0, 0), (x, zm, 1 << y), (0, 0, 2)], typ, guard=1)
                assert gst == status and grp[1, y].tobytes() == out[1].tobytes(), (name, typ)
                assert np.isnan(grp[0]).all() and np.isnan(np.delete(grp[1], y, 0)).all() and not np.isnan(grp[2, 1]).any()


def group_cases(n):
    """[(target, Z, candidates mask)]: every other variable, a subset, candidates that the rules refuse (the target itself, a
    member of Z), no candidate at all, bits at or above n"""
    rng = np.random.default_rng(3100 + n)
    full = (1 << n) - 1
    groups = []
    for k in (0, 1, 2, min(MAX_COND, n - 2)):
        for _ in range(2):
            Z = sorted(int(v) for v in rng.choice(n, size=k, replace=False))
            t = int(rng.choice([v for v in range(n) if v not in Z]))
            groups.append((t, tuple(Z), full & ~gc.mask_of(Z) & ~(1 << t)))
            groups.append((t, tuple(Z), int(rng.integers(1, full + 1)) & ~gc.mask_of(Z) & ~(1 << t)))
    groups.append((n - 1, (0,), full))                       # the target and the member of Z are asked for: refused cells
    groups.append((1, (), 0))                                # asks nothing
    groups.append((0, (n - 1,), (full & ~1 & ~(1 << (n - 1))) | (1 << 50) | (1 << 63)))       # high bits name no cell
    return groups


def check_group_equal_bytes(be, n, S):
    """every grouped cell against dvs_gbn_ci_tests on the pair (target, candidate), as bytes; non-candidates NaN without a
    status bit -> cells compared"""
    mom = gc.run_moments(be, gc.gauss_data(n, S))
    groups = group_cases(n)
    cells = 0
    for typ in TYPES:
        out, status = run_group(be, mom, n, groups, typ, guard=1)
        again, _ = run_group(be, mom, n, groups, typ)
        assert out.tobytes() == again.tobytes()
        tests, where = [], []
        for g, (t, Z, cand) in enumerate(groups):
            for c in range(n):
                if (cand >> c) & 1:
                    tests.append((t, c, Z))
                    where.append((g, c))
                else:
                    assert np.isnan(out[g, c]).all(), (typ, g, c)
        per, st = run_ci(be, mom, n, tests, typ)
        got = np.stack([out[g, c] for g, c in where])
        assert got.tobytes() == per.tobytes(), (n, typ, np.argwhere(got.view(U64) != per.view(U64))[:5])
        assert status == st == 16 and int(np.isnan(per[:, 0]).sum()) == 2          # the two cells of the group that asks for them
        # without that group nothing is refused: the NaNs of the cells that were not asked for set no bit
        clean = [g for g in groups if g != (n - 1, (0,), (1 << n) - 1)]
        out2, st2 = run_group(be, mom, n, clean, typ)
        assert st2 == 0 and np.isnan(out2).any()
        cells += len(tests)
    return cells


def check_row_sets(be):
    """a row-set call (three sets through set_of, tests and groups) against the plain call on each set's gathered rows, as bytes"""
    n, S = 17, 389
    x = gc.gauss_data(n, S)
    rows = gc.row_sets(S, 150, n_sets=3)
    mom = gc.run_moments(be, x, rows)
    tests = pool(n)
    set_of = np.arange(len(tests), dtype=np.int32) % 3
    groups = group_cases(n)[:6]
    gset = (np.arange(len(groups), dtype=np.int32) + 1) % 3
    for typ in TYPES:
        out, status = run_ci(be, mom, n, tests, typ, set_of=set_of)
        grp, gst = run_group(be, mom, n, groups, typ, set_of=gset)
        assert status == 0 and gst == 0
        for r in range(3):
            one = gc.run_moments(be, np.ascontiguousarray(x[rows[r]]))
            assert one.tobytes() == mom[r:r + 1].tobytes()
            mine = [t for t, s in zip(tests, set_of) if s == r]
            assert run_ci(be, one, n, mine, typ)[0].tobytes() == out[set_of == r].tobytes(), (typ, r)
            gmine = [g for g, s in zip(groups, gset) if s == r]
            assert run_group(be, one, n, gmine, typ)[0].tobytes() == grp[gset == r].tobytes(), (typ, r)
    assert mom[0].tobytes() != mom[1].tobytes()


def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do), in the documented order"""
    def tests(**kw):
        a = dict(T=4, n=5, mom=ptr, sets=1, set_of=None, pairs=ptr, cond=ptr, typ=1, out=ptr, ob=4 * 24, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_ci_tests(a["T"], a["n"], a["mom"], a["sets"], a["set_of"], a["pairs"], a["cond"], a["typ"], a["out"], a["ob"],
                                    a["status"], None)

    def group(**kw):
        a = dict(G=4, n=5, mom=ptr, sets=1, set_of=None, target=ptr, cond=ptr, cand=ptr, typ=1, out=ptr, ob=4 * 5 * 24, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_ci_tests_group(a["G"], a["n"], a["mom"], a["sets"], a["set_of"], a["target"], a["cond"], a["cand"], a["typ"],
                                          a["out"], a["ob"], a["status"], None)
    for fn, count in ((tests, "T"), (group, "G")):
        assert fn(**{count: 0}) == 2 and fn(**{count: -1}) == 2 and fn(sets=0) == 2
        assert fn(n=0) == 3 and fn(n=49) == 3
        assert fn(typ=-1) == 12 and fn(typ=3) == 12
        assert fn(mom=None) == 10 and fn(cond=None) == 10 and fn(out=None) == 10 and fn(status=None) == 10
        # the order: counts before n_vars before the index range before the type before the pointers before the size
        assert fn(**{count: 0}, n=0) == 2 and fn(n=0, typ=9) == 3 and fn(typ=9, mom=None) == 12 and fn(mom=None, ob=0) == 10
    assert tests(pairs=None) == 10 and group(target=None) == 10 and group(cand=None) == 10
    assert tests(T=(1 << 31) // 3 + 1) == 2 and b"2^31" in lib.dvs_last_error() and tests(T=(1 << 31) // 3 + 1, typ=9) == 2
    assert group(G=(1 << 31) // (48 * 3) + 1, n=48) == 2 and b"2^31" in lib.dvs_last_error()
    assert tests(ob=95) == 14 and b"96" in lib.dvs_last_error()
    assert group(ob=479) == 14 and b"480" in lib.dvs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# PC-stable and MMPC on real data: the restatement with its guards, the raw launch sequences
# ---------------------------------------------------------------------------------------------------------------------
def guard_of(typ):
    return GUARD_FACTOR * BUILD_FACTOR * TAIL_RTOL[typ]


@functools.lru_cache(maxsize=None)
def pc_reference(n, S, typ, alpha=ALPHA):
    """pc_corpus.pc_ref over the restated tests on the restated moments, its orientation, the closest |p - alpha| / alpha and
    the tests the restatement refused"""
    mom = gc.restated_moments(gc.gauss_data(n, S))[0]
    seen = SimpleNamespace(closest=float("inf"), refused=0)

    def independent(x, y, zm):
        p = restated_test(mom, n, x, y, zm, typ)[2]
        if math.isnan(p):
            seen.refused += 1
            return False
        seen.closest = min(seen.closest, abs(p - alpha) / alpha)
        return p > alpha
    r = pc.pc_ref(n, independent)
    r.pdag, r.conflicts, r.flag = pc.orient_ref(r.adj, r.sepset)
    r.closest, r.refused = seen.closest, seen.refused
    return r


def check_pc_guard(n, S, typ):
    ref = pc_reference(n, S, typ)
    print(f"pc-stable n {n} S {S} {typ}: tests {ref.tests_per_level} = {sum(ref.tests_per_level)}, edges "
          f"{sum(bin(a).count('1') for a in ref.adj) // 2}, conflicts {ref.conflicts}, closest |p - alpha| / alpha {ref.closest:.3e} "
          f"(guard {guard_of(typ):.1e})")
    assert ref.closest > guard_of(typ) and ref.refused == 0 and len(ref.tests_per_level) >= 2, (n, S, typ, ref.closest)
    return ref


def pc_raw(be, x, typ, alpha=ALPHA, max_cond=None, chunk=65536):
    """PC-stable through the raw C ABI: the launch sequence of dags_vae_search_amd/pc.py on a Gaussian evaluator"""
    S, n = x.shape
    mom = be.put(gc.run_moments(be, x))
    adj = [((1 << n) - 1) & ~(1 << v) for v in range(n)]
    hsep = be.put(np.zeros((n, n), U64))
    status, refused = be.put(np.zeros(1, np.int32)), be.put(np.zeros(1, np.int32))
    per_level, refused_total, level = [], 0, 0
    while max_cond is None or level <= max_cond:
        pair_xy, offsets, _ = pc.ref_level(adj, level)
        T, P = offsets[-1], len(pair_xy)
        if T == 0:
            break
        ha, hn = be.put(np.array(adj, U64)), be.put(np.zeros(n, U64))
        hx, ho = be.put(np.array(pair_xy, np.int32)), be.put(np.array(offsets, np.int64))
        pairs, cond, out = be.put(np.zeros((T, 2), np.int32)), be.put(np.zeros(T, U64)), be.put(np.zeros((T, 3)))
        res = be.put(np.zeros((P, 2), np.int64))
        gc.call(be, "dvs_pc_expand", n_pairs=P, n_vars=n, level=level, adj=ha, pair_xy=hx, offsets=ho, n_tests=T, pairs=pairs,
                cond=cond, tests_bytes=T * 8)
        for t0 in range(0, T, chunk):
            m = min(chunk, T - t0)
            at = lambda h, b: ctypes.c_void_p(be.ptr(h).value + b)
            gc.call(be, "dvs_gbn_ci_tests", n_tests=m, n_vars=n, moments=mom, n_sets=1, set_of=None, pairs=at(pairs, t0 * 8),
                    cond=at(cond, t0 * 8), test_type=type_id(typ), out=at(out, t0 * 24), out_bytes=m * 24, status=status)
        gc.call(be, "dvs_pc_reduce", n_pairs=P, n_vars=n, pair_xy=hx, offsets=ho, n_tests=T, cond=cond, out=out, alpha=alpha, adj=ha,
                adj_next=hn, sepset=hsep, sepset_bytes=n * n * 8, result=res, result_bytes=P * 16, refused=refused)
        adj = [int(v) for v in be.get(hn)]
        refused_total += int(be.get(refused)[0])
        per_level.append(T)
        level += 1
    sepset = be.get(hsep).copy()
    pdag, conf, fl = pc.run_orient(be, np.array([adj], U64), sepset[None])
    return SimpleNamespace(adj=adj, sepset=sepset, tests_per_level=per_level, refused=refused_total, status=int(be.get(status)[0]),
                           pdag=[int(v) for v in pdag[0]], conflicts=int(conf[0]), flag=int(fl[0]))


def check_pc_raw(be, n, S, typ):
    ref = check_pc_guard(n, S, typ)
    got = pc_raw(be, gc.gauss_data(n, S), typ, chunk=61)
    assert got.refused == 0 and got.status == 0
    pc.assert_same_result(got, ref, (n, S, typ))
    return got


@functools.lru_cache(maxsize=None)
def mmpc_reference(n, S, typ, max_cond=3, alpha=ALPHA):
    """local_corpus.mmpc_ref over the restated tests (the pair is (target, candidate), the statistic its absolute value) with the
    guards of local_corpus.e2e_reference: the closest decision, the narrowest selection"""
    mom = gc.restated_moments(gc.gauss_data(n, S))[0]
    seen = SimpleNamespace(decision=float("inf"), gap=float("inf"), ties=0, at_flush=0)

    def watch(kind, *a):
        if kind == "decision":
            seen.decision = min(seen.decision, abs(a[0] - alpha) / alpha)
            return
        F, still = a
        mine = next(c for c in still if c[0] == F)
        seen.at_flush += sum(1 for _, pm, _ in still if lc.FLUSH / 2 <= pm <= lc.FLUSH * 2)
        for c, pm, sm in still:
            if c == F:
                continue
            if lc.flushed(pm) != lc.flushed(mine[1]):
                gap = (abs(pm - mine[1]) - 2 * P_FLOOR) / max(pm, mine[1])
            else:
                seen.ties += 1
                gap = abs(sm - mine[2]) / max(sm, mine[2]) if sm != mine[2] else 0.0
            seen.gap = min(seen.gap, gap)

    @functools.lru_cache(maxsize=None)
    def tester(c, t, zm):
        stat, _, p = restated_test(mom, n, t, c, zm, typ)
        return None if math.isnan(p) else (abs(stat), p)
    ref = lc.mmpc_ref(n, tester, alpha, max_cond, watch)
    ref.seen, ref.tests = seen, tester.cache_info().currsize
    return ref


def check_mmpc_guard(n, S, typ):
    ref = mmpc_reference(n, S, typ)
    s = ref.seen
    print(f"mmpc n {n} S {S} {typ}: groups {ref.groups_per_round} = {sum(ref.groups_per_round)}, distinct tests {ref.tests}, edges "
          f"{sum(lc.popcount(a) for a in ref.skeleton) // 2}, asymmetric {ref.asymmetric}, closest |p - alpha| / alpha {s.decision:.3e}, "
          f"narrowest selection gap {s.gap:.3e}, ties on p {s.ties} (guard {guard_of(typ):.1e})")
    assert s.decision > guard_of(typ) and s.gap > guard_of(typ) and s.at_flush == 0 and ref.refused == 0, (n, S, typ, vars(s))
    return ref


def mmpc_raw(be, x, typ, alpha=ALPHA, max_cond=3):
    """MMPC through the raw C ABI: the launch sequence of dags_vae_search_amd/local.py on a Gaussian evaluator, the statistic
    column made absolute between the grouped tests and the update"""
    S, n = x.shape
    mom = be.put(gc.run_moments(be, x))
    hstatus = be.put(np.zeros(1, np.int32))
    dev = SimpleNamespace(last=be.put(np.full(n, -1, np.int32)), pmax=be.put(np.zeros((n, n))), smin=be.put(np.full((n, n), np.inf)),
                          sepset=be.put(np.zeros((n, n), U64)), refused=be.put(np.zeros(1, np.int32)), result=be.put(np.zeros((n, 2), np.int64)))

    def round_fn(phase, groups, st):
        target, cond, candidates, offsets = groups
        G = len(target)
        ht, hz, hc = be.put(np.array(target, np.int32)), be.put(np.array(cond, U64)), be.put(np.array(candidates, U64))
        out = be.put(np.zeros((G, n, 3)))
        gc.call(be, "dvs_gbn_ci_tests_group", n_groups=G, n_vars=n, moments=mom, n_sets=1, set_of=None, target=ht, cond=hz,
                candidates=hc, test_type=type_id(typ), out=out, out_bytes=G * n * 24, status=hstatus)
        cells = np.array(be.get(out), copy=True)
        cells[:, :, 0] = np.abs(cells[:, :, 0])
        out = be.put(cells)
        cpc_next, cand_next = be.put(np.zeros(n, U64)), be.put(np.zeros(n, U64))
        gc.call(be, "dvs_mmpc_update", n_vars=n, n_groups=G, phase=phase, target=ht, cond=hz, candidates=hc,
                group_offsets=be.put(np.array(offsets, np.int64)), out=out, out_bytes=G * n * 24, alpha=alpha, cpc=be.put(np.array(st.cpc, U64)),
                cand=be.put(np.array(st.cand, U64)), cpc_next=cpc_next, cand_next=cand_next, last=dev.last, pmax=dev.pmax, smin=dev.smin,
                sepset=dev.sepset, state_bytes=n * n * 8, refused=dev.refused, result=dev.result, result_bytes=n * 16)
        new = SimpleNamespace(cpc=[int(v) for v in be.get(cpc_next)], cand=[int(v) for v in be.get(cand_next)],
                              last=[int(v) for v in be.get(dev.last)], pmax=None, smin=None, sepset=be.get(dev.sepset).copy())
        return new, int(be.get(dev.refused)[0])
    got = lc.mmpc_driver(n, max_cond, round_fn)
    got.status = int(be.get(hstatus)[0])
    return got


def check_mmpc_raw(be, n, S, typ):
    ref = check_mmpc_guard(n, S, typ)
    got = mmpc_raw(be, gc.gauss_data(n, S), typ)
    assert got.refused == 0 and got.status == 0
    lc.assert_same_mmpc(got, ref, (n, S, typ))
    return got
