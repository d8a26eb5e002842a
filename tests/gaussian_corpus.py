"""Gaussian networks (include/dvs_gaussian.h; csrc/dvs_gaussian.h): seeded linear-Gaussian data, the numpy restatement of the
header's definitions, the references, and the checks that tests/test_emu_gaussian.py and tests/test_gpu_gaussian.py run
unchanged through the C ABI on their own back end (tests/scoring_corpus.py: EmuBackend, GpuBackend).

References
  moments   exact rationals.  A float64 is a dyadic rational, so the rows become integers at one common scale 2^-K and
            C = (m sum x_i x_j - s_i s_j) / m is exact in Python integers (``exact_moments``).
  scores    mpmath at 60 digits on those exact moments (``Reference``: determinants of principal submatrices, lu_solve for the
            coefficients — no Cholesky factor), and an independent float64 route that never forms a Cholesky factor either:
            numpy.linalg.lstsq on the raw rows for RSS and the coefficients, slogdet for the determinants (``lstsq_family``).

Tolerances.  None is fitted to a kernel's output.  u = 2^-53, gamma_k = k u / (1 - k u) (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., §3.1).
  moment cell   With mu^ the computed mean and delta = mu^ - mu: sum (x_i - mu^_i)(x_j - mu^_j) = C_ij + m delta_i delta_j exactly,
            because sum (x_i - mu_i) = 0.  Every term of the computed sum carries one subtraction per factor, one product and at
            most m - 1 additions (any order): a factor (1 + e)^(m + 2) at most.  So
                |C^_ij - C_ij| <= gamma_(m+2) sum |x_i - mu^_i| |x_j - mu^_j| + m |delta_i| |delta_j| =: E_ij   (``moment_bound``),
            both terms computed in integers / Fractions.  The mean: m - 1 additions and a division, |mu^ - mu| <= gamma_m sum |x| / m.
  ln det    The factor of A = M[a][a] (order q = p + 1 or p) is computed from C^, |C^ - C| <= E, and satisfies R^T R = A^ + dA with
            |dA| <= gamma_(q+1) |R^T| |R| (Higham Thm 10.3), so ||dA||_2 <= q gamma_(q+1) / (1 - q gamma_(q+1)) ||A^||_2.  With
            F = ||E[a][a]||_F + 1.01 q gamma_(q+1) (||A||_2 + ||E[a][a]||_F) + u ||A||_2 (bge's one addition of t) and eta = F / sigma_min(A), which the derivation
            needs below ETA_CAP = 1/4 (the condition on the inputs: asserted from the mpmath reference, kappa = ||A||_2 /
            sigma_min), the product of the squared pivots is det(A + G), ||G||_2 <= F, and
                |ln det(A + G) - ln det A| = |sum ln(1 + lambda_i(A^-1 G))| <= q eta / (1 - eta).
            The sum of the logs adds rounding: each log within 2 ulp, q additions: gamma_(q+3) sum |ln d_k^2|, the reference's
            pivots standing in for the computed ones at the cost of the factor 1.01.  ``logdet_bound`` is the sum of the two.
  score     ln RSS = ln det M[fam] - ln det M[Pa].  loglik-g: (m / 2) times the bound of ln RSS, plus 8 u times the sum of the
            magnitudes of the terms.  bge: (m + g + 1) / 2 times the bound of ln det R[fam] plus (m + g) / 2 times that of
            ln det R[Pa] (ldf = ldp + log RSS adds 3 u |ldf|), plus 16 u times the sum of the magnitudes of the seven terms (lgamma
            within 4 ulp).  ``score_bound``.
  fit       beta = A^-1 b over the parents: (A + G) beta^ = b + db with ||G||_2 <= F3 (F with gamma_(3q+1): Higham Thm 10.4,
            factor and two solves) and ||db||_2 <= ||E[Pa, v]||_2, so ||beta^ - beta||_2 <= (||db|| + F3 ||beta||) / (sigma_min -
            F3) (``coef_bound``; every coefficient is held to the 2-norm bound).  sd: with b the bound of ln RSS, sd (expm1(b / 2) + 4 u).
            intercept: sum |mean_u| times the coefficient bound, plus gamma_(p+2) (|mean_v| + sum |beta_u mean_u|), plus the means' own.
The largest observed error / bound per quantity is printed by the checks and recorded in DESIGN.md §29."""
import ctypes
import functools
import itertools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

from dags_vae_search_amd import _lib as dl

DPS = 60                                   # mpmath's working precision is global state that other corpora set: every reference here runs under at60
U64 = np.uint64
U = 2.0 ** -53
CHUNK, CAP = dl.GBN_CHUNK, dl.GBN_MAX_PARENTS
N_VALUES = (1, 3, 5, 17, 48)
S_VALUES = (2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)
TYPES = ("loglik-g", "aic-g", "bic-g", "bge")
ETA_CAP = 0.25
KAPPA_CAP = 1e10
NAN = float("nan")
SENTINEL = -7.0


def at60(fn):
    """run ``fn`` at 60 digits whatever precision the process stands at"""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with mp.workdps(DPS):
            return fn(*args, **kwargs)
    return wrapped


def gamma(k):
    return k * U / (1 - k * U)


def stride(n):
    return 1 + n + n * n


def mask_of(bits):
    return sum(1 << int(b) for b in bits)


def bits_of(mask):
    return [b for b in range(64) if (int(mask) >> b) & 1]


# ---------------------------------------------------------------------------------------------------------------------
# Data
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gauss_data(n, S, seed=0):
    """float64 [S, n]: column i is a linear function of up to two earlier columns plus noise, rescaled to unit variance and
    then given one of a few scales and offsets (independent columns would let a mixed-up index pass)."""
    rng = np.random.default_rng(29000 + 97 * n + S + 7919 * seed)
    x = np.zeros((S, n))
    for i in range(n):
        pa = rng.choice(i, size=min(i, int(rng.integers(0, 3))), replace=False) if i else []
        col = rng.normal(0.0, 1.0, S)
        for j in pa:
            col = col + float(rng.uniform(0.4, 0.9)) * float(rng.choice([-1.0, 1.0])) * x[:, j]
        sd = col.std() if S > 1 and col.std() > 0 else 1.0
        x[:, i] = col / sd
    scale = np.asarray([(0.5, 1.0, 3.0)[i % 3] for i in range(n)])
    offset = np.asarray([(-2.0, 0.0, 5.0, 0.25)[i % 4] for i in range(n)])
    out = x * scale + offset
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def degenerate_data():
    """integer-valued float64 [CHUNK, 5] whose moments are exact in fp64 (a power-of-two row count, small integers): column 3
    duplicates column 1 and column 4 = column 0 + column 2, so exactly the families holding {1, 3} or {0, 2, 4} are singular"""
    rng = np.random.default_rng(2905)
    x = rng.integers(-8, 9, (CHUNK, 5)).astype(np.float64)
    x[:, 3] = x[:, 1]
    x[:, 4] = x[:, 0] + x[:, 2]
    x.setflags(write=False)
    return x


def row_sets(S, set_size, n_sets=3, seed=0):
    """int32 [n_sets, set_size] with repeated indices"""
    rng = np.random.default_rng(2950 + S + 31 * set_size + seed)
    rows = rng.integers(0, S, (n_sets, set_size)).astype(np.int32)
    if set_size > 1:
        rows[:, 1] = rows[:, 0]                              # a repeat in every set
    return rows


def random_dags(n, B, max_parents, seed):
    """uint64 [B, n] parent masks of DAGs (a random order, up to max_parents earlier variables each)"""
    rng = np.random.default_rng(2970 + n + 13 * seed)
    P = np.zeros((B, n), U64)
    for b in range(B):
        order = rng.permutation(n)
        for k in range(1, n):
            pa = rng.choice(order[:k], size=min(k, int(rng.integers(0, max_parents + 1))), replace=False)
            P[b, order[k]] = U64(mask_of(pa))
    return P


# ---------------------------------------------------------------------------------------------------------------------
# Exact moments and their bound
# ---------------------------------------------------------------------------------------------------------------------
def _scaled_ints(*arrays):
    """the float64 arrays as Python-int object arrays at one common scale: value = int * 2^-K"""
    K = 0
    for a in arrays:
        for v in np.asarray(a, np.float64).ravel():
            K = max(K, Fraction(float(v)).denominator.bit_length() - 1)
    return [np.vectorize(lambda v: int(Fraction(float(v)) * (1 << K)), otypes=[object])(np.asarray(a, np.float64)) for a in arrays], K


class ExactMoments:
    """m, the exact mean (Fractions) and C as integers: C_ij = Cnum[i][j] / (m 4^K)"""

    def __init__(self, x):
        x = np.asarray(x, np.float64)
        self.m, self.n = x.shape
        (X,), self.K = _scaled_ints(x)
        self.X = X
        self.s = X.sum(0)
        self.Cnum = self.m * (X.T.dot(X)) - np.outer(self.s, self.s)
        self.den = self.m * (1 << (2 * self.K))
        self.abs_sum = np.abs(X).sum(0)

    def mean(self, i):
        return Fraction(int(self.s[i]), self.m * (1 << self.K))

    def C(self, i, j):
        return Fraction(int(self.Cnum[i, j]), self.den)

    def C_float(self):
        return np.asarray([[float(self.C(i, j)) for j in range(self.n)] for i in range(self.n)])

    @at60
    def C_mp(self):
        return mp.matrix([[mp.mpf(int(self.Cnum[i, j])) / self.den for j in range(self.n)] for i in range(self.n)])

    def mean_bound(self, i):
        return gamma(self.m) * float(Fraction(int(self.abs_sum[i]), self.m * (1 << self.K)))

    def moment_bound(self, mean_hat):
        """E [n][n] floats (rounded up by 1 + 2^-40) for a computed mean vector"""
        m, n = self.m, self.n
        (Mh,), Kh = _scaled_ints(mean_hat)
        K = max(self.K, Kh)
        D = np.abs(self.X * (1 << (K - self.K)) - Mh * (1 << (K - Kh)))          # |x - mu^| at scale 2^-K
        A = D.T.dot(D)                                                            # sum |d_i| |d_j| at scale 4^-K
        delta = [abs(Fraction(float(mean_hat[i])) - self.mean(i)) for i in range(n)]
        g = Fraction(gamma(m + 2))
        E = np.zeros((n, n))
        for i in range(n):
            for j in range(n):
                E[i, j] = float(g * Fraction(int(A[i, j]), 1 << (2 * K)) + m * delta[i] * delta[j]) * (1 + 2.0 ** -40)
        return E


@functools.lru_cache(maxsize=None)
def exact_of(n, S, seed=0):
    return ExactMoments(gauss_data(n, S, seed))


# ---------------------------------------------------------------------------------------------------------------------
# The numpy restatement of include/dvs_gaussian.h
# ---------------------------------------------------------------------------------------------------------------------
def restated_moments(x, rows=None):
    """float64 [n_sets, stride]: the header's two passes, chunk by chunk, position by position (vectorised over the cells: every
    cell sees its own additions in the stated order)"""
    x = np.asarray(x, np.float64)
    S, n = x.shape
    sets = [x] if rows is None else [x[np.asarray(r)] for r in rows]
    out = np.zeros((len(sets), stride(n)))
    for r, g in enumerate(sets):
        m = len(g)
        total = np.zeros(n)
        for c0 in range(0, m, CHUNK):
            part = np.zeros(n)
            for row in g[c0:c0 + CHUNK]:
                part = part + row
            total = total + part
        mean = total / np.float64(m)
        C = np.zeros((n, n))
        for c0 in range(0, m, CHUNK):
            part = np.zeros((n, n))
            for row in g[c0:c0 + CHUNK]:
                d = row - mean
                part = part + np.outer(d, d)
            C = C + part
        out[r, 0] = m
        out[r, 1:1 + n] = mean
        out[r, 1 + n:] = C.ravel()
    return out


def default_args(typ, n, arg=None, arg2=None):
    """(score_arg, score_arg2) as the library resolves them on the host; bic-g's default stays NaN (taken on the device)"""
    if typ == "bge":
        return (1.0 if arg is None else float(arg)), (n + 2.0 if arg2 is None else float(arg2))
    if typ == "aic-g":
        return (1.0 if arg is None else float(arg)), NAN
    return (NAN if arg is None else float(arg)), NAN


def bge_t(n, am, aw):
    return am * (aw - n - 1.0) / (am + 1.0)


def restated_family(mom, n, v, pm, t=0.0, likelihood=True):
    """the header's factor of the family (v, pm) from one set's moments -> (p, m, ldp, rss, L, parents) or None (refused)"""
    m = float(mom[0])
    C = np.asarray(mom[1 + n:]).reshape(n, n)
    pm = int(pm) & ~(1 << v)
    pa = bits_of(pm)
    p = len(pa)
    if pm >> n or p > CAP:
        return None
    if likelihood and m - p - 1.0 < 1.0:
        return None
    a = pa + [v]
    L = np.zeros((p + 1, p + 1))
    ldp, d2 = 0.0, 0.0
    for i in range(p + 1):
        for j in range(i):
            s = float(C[a[i], a[j]])
            for k in range(j):
                s = s - float(L[i, k]) * float(L[j, k])
            L[i, j] = s / float(L[j, j])
        diag = float(C[a[i], a[i]]) + t
        s = diag
        for k in range(i):
            s = s - float(L[i, k]) * float(L[i, k])
        if not (math.isfinite(s) and s > ((p + 2) * 2.0 ** -52) * diag):
            return None
        L[i, i] = math.sqrt(s)
        d2 = s
        if i < p:
            ldp = ldp + math.log(s)
    return p, m, ldp, d2, L, pa


def restated_local(mom, n, v, pm, typ, arg=None, arg2=None):
    """the local score of include/dvs_gaussian.h in float64, operation by operation; NaN for a refused family"""
    a1, a2 = default_args(typ, n, arg, arg2)
    bge = typ == "bge"
    f = restated_family(mom, n, v, pm, bge_t(n, a1, a2) if bge else 0.0, not bge)
    if f is None:
        return NAN
    p, m, ldp, rss, _, _ = f
    if not bge:
        dof = m - p - 1.0
        ll = -(0.5 * m) * math.log(6.283185307179586 * (rss / dof)) - 0.5 * dof
        if typ == "loglik-g":
            return ll
        k = math.log(m) / 2.0 if a1 != a1 else a1
        return ll - k * (p + 2.0)
    g = a2 - float(n) + p
    ldf = ldp + math.log(rss)
    s = -(0.5 * m) * math.log(3.141592653589793)
    s = s + 0.5 * math.log(a1 / (a1 + m))
    s = s + math.lgamma(0.5 * (m + g + 1.0))
    s = s - math.lgamma(0.5 * (g + 1.0))
    s = s + (0.5 * (g + p + 1.0)) * math.log(bge_t(n, a1, a2))
    s = s - (0.5 * (m + g + 1.0)) * ldf
    s = s + (0.5 * (m + g)) * ldp
    return s


def restated_fit(mom, n, v, pm):
    """(coef [n], intercept, sd) of the header's dvs_gbn_fit for one family; NaNs for a refused one"""
    f = restated_family(mom, n, v, pm, 0.0, True)
    if f is None:
        return np.full(n, NAN), NAN, NAN
    p, m, _, rss, L, pa = f
    beta = [0.0] * p
    for i in range(p - 1, -1, -1):
        s = float(L[p, i])
        for k in range(i + 1, p):
            s = s - float(L[k, i]) * beta[k]
        beta[i] = s / float(L[i, i])
    coef = np.zeros(n)
    c0 = float(mom[1 + v])
    for i, u in enumerate(pa):
        coef[u] = beta[i]
        c0 = c0 - beta[i] * float(mom[1 + u])
    return coef, c0, math.sqrt(rss / (m - p - 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# The mpmath reference and the bounds
# ---------------------------------------------------------------------------------------------------------------------
class Reference:
    """mpmath scores and fits on the exact moments of one data set; determinants, norms and pivots are cached per (subset, t)"""

    @at60
    def __init__(self, ex, mean_hat=None):
        self.ex, self.n, self.m = ex, ex.n, ex.m
        self.C = ex.C_mp()
        self.mean = [mp.mpf(ex.mean(i).numerator) / ex.mean(i).denominator for i in range(ex.n)]
        mean_hat = [float(ex.mean(i)) for i in range(ex.n)] if mean_hat is None else mean_hat
        self.E = ex.moment_bound(mean_hat)
        self._cache = {}

    def sub(self, idx, t):
        A = mp.matrix(len(idx), len(idx))
        for r, i in enumerate(idx):
            for c, j in enumerate(idx):
                A[r, c] = self.C[i, j] + (t if i == j else 0)
        return A

    @at60
    def facts(self, idx, t):
        """(ln det, ||A||_2, sigma_min, sum |ln pivot|) of M[idx][idx] in the order given"""
        key = (tuple(idx), float(t))
        if key not in self._cache:
            if not idx:
                self._cache[key] = (mp.mpf(0), mp.mpf(0), mp.inf, mp.mpf(0))
            else:
                A = self.sub(idx, mp.mpf(t))
                ev = mp.eigsy(A, eigvals_only=True)
                ev = [ev[i] for i in range(len(idx))]
                piv, prev = mp.mpf(0), mp.mpf(1)
                for q in range(1, len(idx) + 1):
                    d = mp.det(A[:q, :q])
                    piv += abs(mp.log(d / prev))
                    prev = d
                self._cache[key] = (mp.log(prev), max(abs(e) for e in ev), min(ev), piv)
        return self._cache[key]

    @at60
    def logdet_bound(self, idx, t, solve=False):
        """the bound of the docstring on the computed ln det of M[idx][idx] (float), after asserting the input condition; with
        ``solve`` returns (F3, sigma_min) for the coefficient bound instead"""
        q = len(idx)
        if q == 0:
            return 0.0
        _, norm, smin, piv = self.facts(idx, t)
        assert smin > 0 and float(norm / smin) < KAPPA_CAP, ("kappa", idx, float(norm / smin))
        Ef = float(np.linalg.norm(self.E[np.ix_(idx, idx)]))
        gq = gamma(3 * q + 1) if solve else gamma(q + 1)
        F = Ef + 1.01 * q * gq * (float(norm) + Ef) + U * float(norm)          # the last term: bge's one addition of t on the diagonal
        eta = F / float(smin)
        assert eta < ETA_CAP, ("eta", idx, eta)
        if solve:
            return F, float(smin)
        return q * eta / (1 - eta) + 1.01 * gamma(q + 3) * float(piv)

    @at60
    def local(self, v, pa, typ, arg=None, arg2=None):
        """(score as mpf, bound as float) of the family, or (None, None) where the definition refuses it (m - p - 1 < 1)"""
        n, m, p = self.n, self.m, len(pa)
        a1, a2 = default_args(typ, n, arg, arg2)
        pa = sorted(pa)
        fam = pa + [v]
        if typ != "bge":
            dof = m - p - 1
            if dof < 1:
                return None, None
            ldp, ldf = self.facts(pa, 0.0)[0], self.facts(fam, 0.0)[0]
            rss = mp.exp(ldf - ldp)
            terms = [-(mp.mpf(m) / 2) * mp.log(2 * mp.pi * rss / dof), -mp.mpf(dof) / 2]
            if typ != "loglik-g":
                k = mp.log(m) / 2 if a1 != a1 else mp.mpf(a1)
                terms.append(-k * (p + 2))
            bound = (m / 2.0) * (self.logdet_bound(fam, 0.0) + self.logdet_bound(pa, 0.0)) + 8 * U * float(sum(abs(x) for x in terms))
            return sum(terms), bound
        tf = bge_t(n, a1, a2)                     # t is the fp64 value the library computes on the host
        t = mp.mpf(tf)
        ldp, ldf = self.facts(pa, tf)[0], self.facts(fam, tf)[0]
        g = mp.mpf(a2) - n + p
        terms = [-(mp.mpf(m) / 2) * mp.log(mp.pi), mp.log(mp.mpf(a1) / (a1 + m)) / 2, mp.loggamma((m + g + 1) / 2),
                 -mp.loggamma((g + 1) / 2), ((g + p + 1) / 2) * mp.log(t), -((m + g + 1) / 2) * ldf, ((m + g) / 2) * ldp]
        cf, cp_ = float((m + g + 1) / 2), float((m + g) / 2)
        bound = cf * (self.logdet_bound(fam, tf) + self.logdet_bound(pa, tf) + 3 * U * float(abs(ldf))) + cp_ * self.logdet_bound(pa, tf) \
            + 16 * U * float(sum(abs(x) for x in terms))
        return sum(terms), bound

    @at60
    def fit(self, v, pa):
        """((coef {u: mpf}, intercept, sd), (coefficient bound, intercept bound, sd bound)) of the family"""
        m, p = self.m, len(pa)
        pa = sorted(pa)
        fam = pa + [v]
        ldp, ldf = self.facts(pa, 0.0)[0], self.facts(fam, 0.0)[0]
        rss = mp.exp(ldf - ldp)
        sd = mp.sqrt(rss / (m - p - 1))
        sd_bound = float(sd) * (math.expm1(0.5 * (self.logdet_bound(fam, 0.0) + self.logdet_bound(pa, 0.0))) + 4 * U)
        mean_own = self.ex.mean_bound
        if p == 0:
            return ({}, self.mean[v], sd), (0.0, mean_own(v) + 2 * U * abs(float(self.mean[v])), sd_bound)
        b = mp.matrix([self.C[u, v] for u in pa])
        beta = mp.lu_solve(self.sub(pa, 0), b)
        F3, smin = self.logdet_bound(pa, 0.0, solve=True)
        nb = float(mp.norm(beta, 2))
        db = float(np.linalg.norm(self.E[pa, v]))
        cb = (db + F3 * nb) / (smin - F3) + 2 * U * nb
        icpt = self.mean[v] - sum(beta[i] * self.mean[u] for i, u in enumerate(pa))
        mags = abs(float(self.mean[v])) + sum(abs(float(beta[i] * self.mean[u])) for i, u in enumerate(pa))
        ib = cb * sum(abs(float(self.mean[u])) + mean_own(u) for u in pa) + gamma(p + 2) * mags + mean_own(v) \
            + sum((abs(float(beta[i])) + cb) * mean_own(u) for i, u in enumerate(pa))
        return ({u: beta[i] for i, u in enumerate(pa)}, icpt, sd), (cb, ib, sd_bound)


@functools.lru_cache(maxsize=None)
def reference_of(n, S, seed=0):
    ex = exact_of(n, S, seed)
    return Reference(ex, restated_moments(gauss_data(n, S, seed))[0, 1:1 + n])


def lstsq_family(x, v, pa, typ, arg=None, arg2=None):
    """the independent float64 route: lstsq on the raw rows, slogdet of the centred cross-products; no Cholesky factor"""
    x = np.asarray(x, np.float64)
    m, n = x.shape
    pa = sorted(pa)
    p = len(pa)
    a1, a2 = default_args(typ, n, arg, arg2)
    xc = x - x.mean(0)
    C = xc.T @ xc
    if typ != "bge":
        design = np.column_stack([np.ones(m)] + [x[:, u] for u in pa])
        sol = np.linalg.lstsq(design, x[:, v], rcond=None)[0]
        res = x[:, v] - design @ sol
        rss = float(res @ res)
        dof = m - p - 1.0
        ll = -(0.5 * m) * math.log(2 * math.pi * rss / dof) - 0.5 * dof
        if typ == "loglik-g":
            return ll
        k = math.log(m) / 2.0 if a1 != a1 else a1
        return ll - k * (p + 2.0)
    t = bge_t(n, a1, a2)
    R = C + t * np.eye(n)
    ldp = np.linalg.slogdet(R[np.ix_(pa, pa)])[1] if p else 0.0
    ldf = np.linalg.slogdet(R[np.ix_(pa + [v], pa + [v])])[1]
    g = a2 - n + p
    return (-(0.5 * m) * math.log(math.pi) + 0.5 * math.log(a1 / (a1 + m)) + math.lgamma(0.5 * (m + g + 1)) - math.lgamma(0.5 * (g + 1))
            + 0.5 * (g + p + 1) * math.log(t) - 0.5 * (m + g + 1) * ldf + 0.5 * (m + g) * ldp)


def lstsq_fit(x, v, pa):
    x = np.asarray(x, np.float64)
    m = len(x)
    pa = sorted(pa)
    design = np.column_stack([np.ones(m)] + [x[:, u] for u in pa])
    sol = np.linalg.lstsq(design, x[:, v], rcond=None)[0]
    res = x[:, v] - design @ sol
    return dict(zip(pa, sol[1:])), float(sol[0]), math.sqrt(float(res @ res) / (m - len(pa) - 1.0))


# the score cases: (n, S, [(v, parents)]) — every parent set at n = 5; p = CAP at n = 17; bit 47 at n = 48
def score_families(n):
    if n == 5:
        return [(v, list(c)) for v in range(5) for r in range(5) for c in itertools.combinations([u for u in range(5) if u != v], r)]
    if n == 17:
        return [(16, list(range(CAP))), (0, list(range(1, CAP + 1))), (3, [0, 16]), (8, [])]
    if n == 48:
        return [(0, [47]), (47, [0, 23, 46]), (20, [47, 1, 2, 3]), (47, [])]
    return [(v, [u for u in range(n) if u != v][:2]) for v in range(n)]


SCORE_SHAPES = ((1, CHUNK + 1), (3, CHUNK - 1), (5, CHUNK + 1), (17, 3 * CHUNK + 5), (48, 3 * CHUNK + 5))
SCORE_VARIANTS = (("loglik-g", None, None), ("aic-g", None, None), ("aic-g", 0.3, None), ("bic-g", None, None), ("bic-g", 2.5, None),
                  ("bge", None, None), ("bge", 2.0, None), ("bge", 0.5, "n+5.5"))


def variant_args(n, variant):
    typ, a, b = variant
    return typ, a, (n + 5.5 if b == "n+5.5" else b)


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI by argument name on a back end
# ---------------------------------------------------------------------------------------------------------------------
def call_rc(be, fn, **args):
    sig = dl.signature(fn)[1]
    missing, unknown = {k for k, _ in sig} - set(args) - {"stream"}, set(args) - {k for k, _ in sig}
    if missing or unknown:
        raise TypeError(f"{fn}: missing {sorted(missing)}, unknown {sorted(unknown)}")
    ptr = lambda h: h if h is None or isinstance(h, ctypes.c_void_p) else be.ptr(h)
    return getattr(be.lib, fn)(*[ptr(args.get(k, be.stream)) if ctype is ctypes.c_void_p else args[k] for k, ctype in sig])


def call(be, fn, **args):
    assert call_rc(be, fn, **args) == 0, be.lib.dvs_last_error()


def run_moments(be, x, rows=None):
    """dvs_gbn_moments -> float64 [n_sets, stride] (a host copy)"""
    x = np.ascontiguousarray(x, np.float64)
    S, n = x.shape
    n_sets, size = (1, S) if rows is None else rows.shape
    need = be.lib.dvs_gbn_moments_workspace_bytes(n, n_sets, size)
    chunks = -(-size // CHUNK)
    assert need == 8 * n_sets * chunks * (n + n * (n + 1) // 2)
    ws, mom = be.put(np.zeros(need, np.uint8)), be.put(np.full((n_sets, stride(n)), SENTINEL))
    call(be, "dvs_gbn_moments", n_vars=n, n_samples=S, data=be.put(x), rows=None if rows is None else be.put(np.ascontiguousarray(rows, np.int32)),
         n_sets=n_sets, set_size=size, workspace=ws, workspace_bytes=need, moments=mom, moments_bytes=n_sets * stride(n) * 8)
    return np.array(be.get(mom), copy=True)


def _type_args(n, typ, arg, arg2):
    return dict(score_type=dl.GSCORE_TYPES[typ], score_arg=NAN if arg is None else float(arg), score_arg2=NAN if arg2 is None else float(arg2))


def run_scores(be, mom, n, parents, typ, arg=None, arg2=None, set_of=None, guard=0):
    """dvs_gbn_scores -> (local [B, n], out [B], status); with ``guard`` rows of sentinels around local, which must survive"""
    parents = np.ascontiguousarray(parents, U64)
    B = len(parents)
    local, out, status = be.put(np.full((B + 2 * guard, n), SENTINEL)), be.put(np.full(B, SENTINEL)), be.put(np.zeros(1, np.int32))
    lp = ctypes.c_void_p(be.ptr(local).value + guard * n * 8)
    call(be, "dvs_gbn_scores", batch=B, n_vars=n, moments=be.put(mom), n_sets=len(mom), set_of=None if set_of is None else be.put(np.asarray(set_of, np.int32)),
         parents=be.put(parents), local=lp, out=out, status=status, **_type_args(n, typ, arg, arg2))
    loc = np.array(be.get(local), copy=True)
    if guard:
        assert (loc[:guard] == SENTINEL).all() and (loc[B + guard:] == SENTINEL).all()
    return loc[guard:B + guard], np.array(be.get(out), copy=True), int(be.get(status)[0])


def run_toggle(be, mom, n, parents, typ, arg=None, arg2=None, set_of=None, worklist=None, tables=None):
    parents = np.ascontiguousarray(parents, U64)
    B = len(parents)
    L0, T0 = (np.full((B, n), SENTINEL), np.full((B, n, n), SENTINEL)) if tables is None else tables
    L, T, status = be.put(L0), be.put(T0), be.put(np.zeros(1, np.int32))
    call(be, "dvs_gbn_toggle_scores", batch=B, n_vars=n, moments=be.put(mom), n_sets=len(mom),
         set_of=None if set_of is None else be.put(np.asarray(set_of, np.int32)), parents=be.put(parents),
         worklist=None if worklist is None else be.put(np.asarray(worklist, np.int32)), local=L, local_bytes=B * n * 8, toggles=T,
         toggles_bytes=B * n * n * 8, status=status, **_type_args(n, typ, arg, arg2))
    return np.array(be.get(L), copy=True), np.array(be.get(T), copy=True), int(be.get(status)[0])


def run_fit(be, mom, n, parents, set_of=None):
    parents = np.ascontiguousarray(parents, U64)
    B = len(parents)
    coef, icpt, sd, status = (be.put(np.full((B, n, n), SENTINEL)), be.put(np.full((B, n), SENTINEL)), be.put(np.full((B, n), SENTINEL)),
                              be.put(np.zeros(1, np.int32)))
    call(be, "dvs_gbn_fit", batch=B, n_vars=n, moments=be.put(mom), n_sets=len(mom), set_of=None if set_of is None else be.put(np.asarray(set_of, np.int32)),
         parents=be.put(parents), coef=coef, coef_bytes=B * n * n * 8, intercept=icpt, sd=sd, status=status)
    return np.array(be.get(coef), copy=True), np.array(be.get(icpt), copy=True), np.array(be.get(sd), copy=True), int(be.get(status)[0])


# ---------------------------------------------------------------------------------------------------------------------
# Checks
# ---------------------------------------------------------------------------------------------------------------------
def moments_against_exact(mom, ex):
    """asserts one set's moments against the exact rationals under the derived bounds -> the largest error / bound"""
    n, m = ex.n, ex.m
    assert mom[0] == m
    mean = mom[1:1 + n]
    worst = 0.0
    for i in range(n):
        err, bound = abs(Fraction(float(mean[i])) - ex.mean(i)), ex.mean_bound(i)
        assert err <= bound, ("mean", i, float(err), bound)
        worst = max(worst, float(err) / bound if bound else 0.0)
    E = ex.moment_bound(mean)
    C = mom[1 + n:].reshape(n, n)
    assert C.tobytes() == np.ascontiguousarray(C.T).tobytes()
    for i in range(n):
        for j in range(i, n):
            err = abs(Fraction(float(C[i, j])) - ex.C(i, j))
            assert err <= E[i, j], ("C", i, j, float(err), E[i, j])
            worst = max(worst, float(err) / E[i, j] if E[i, j] else 0.0)
    return worst


def check_moments(be, n, S):
    """equal bytes over two runs, the restatement's bytes, the exact rationals; then the row sets against the gathered rows"""
    x = gauss_data(n, S)
    a, b = run_moments(be, x), run_moments(be, x)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() == restated_moments(x).tobytes(), "the kernel and the numpy restatement of the header disagree"
    worst = moments_against_exact(a[0], exact_of(n, S))
    size = max(1, S // 2 + 3)
    rows = row_sets(S, size)
    assert size != S and (rows[:, 0] == rows[:, 1]).all()
    sets = run_moments(be, x, rows)
    assert sets.tobytes() == run_moments(be, x, rows).tobytes()
    for r in range(len(rows)):
        gathered = np.ascontiguousarray(x[rows[r]])
        assert sets[r].tobytes() == run_moments(be, gathered)[0].tobytes(), (n, S, r)
        worst = max(worst, moments_against_exact(sets[r], ExactMoments(gathered)))
    return worst


@at60
def check_scores(be, n, S):
    """local scores and totals of every variant against mpmath under the derived bound; -> the largest error / bound"""
    x, ref = gauss_data(n, S), reference_of(n, S)
    mom = run_moments(be, x)
    fams = score_families(n)
    worst = 0.0
    for variant in SCORE_VARIANTS:
        typ, a1, a2 = variant_args(n, variant)
        P = np.zeros((len(fams), n), U64)
        for b, (v, pa) in enumerate(fams):
            P[b, v] = U64(mask_of(pa) | (1 << v) * (b & 1))             # the self bit is ignored
        local, out, status = run_scores(be, mom, n, P, typ, a1, a2, guard=1)
        local2, _, _ = run_scores(be, mom, n, P, typ, a1, a2)
        assert local.tobytes() == local2.tobytes()
        want_status = 0
        for b, (v, pa) in enumerate(fams):
            total = 0.0
            for w in range(n):
                want, bound = ref.local(w, pa if w == v else [], typ, a1, a2)
                got = float(local[b, w])
                if want is None:
                    assert got != got
                    want_status = 16
                    total = NAN
                    continue
                err = abs(mp.mpf(got) - want)
                assert err <= bound, (typ, n, S, w, pa, got, float(want), float(err), bound)
                worst = max(worst, float(err) / bound)
                total = total + got
            assert np.float64(total).tobytes() == out[b].tobytes() or (total != total and out[b] != out[b])
        assert status == want_status
    return worst


@at60
def check_fit(be, n, S):
    x, ref = gauss_data(n, S), reference_of(n, S)
    mom = run_moments(be, x)
    fams = [f for f in score_families(n) if S - len(f[1]) - 1 >= 1]
    P = np.zeros((len(fams), n), U64)
    for b, (v, pa) in enumerate(fams):
        P[b, v] = U64(mask_of(pa))
    coef, icpt, sd, status = run_fit(be, mom, n, P)
    assert status == 0
    worst = [0.0, 0.0, 0.0]
    for b, (v, pa) in enumerate(fams):
        (beta, c0, s), (cb, ib, sb) = ref.fit(v, pa)
        for u in range(n):
            if u in beta:
                err = float(abs(mp.mpf(float(coef[b, v, u])) - beta[u]))
                assert err <= cb, ("coef", n, v, pa, u, err, cb)
                worst[0] = max(worst[0], err / cb)
            else:
                assert coef[b, v, u] == 0.0
        e1, e2 = float(abs(mp.mpf(float(icpt[b, v])) - c0)), float(abs(mp.mpf(float(sd[b, v])) - s))
        assert e1 <= ib and e2 <= sb, ("intercept / sd", n, v, pa, e1, ib, e2, sb)
        worst[1], worst[2] = max(worst[1], e1 / ib), max(worst[2], e2 / sb)
        for w in range(n):
            if w != v:                                                   # the other variables have no parents: their mean and spread
                assert coef[b, w].tobytes() == np.zeros(n).tobytes() and icpt[b, w].tobytes() == mom[0, 1 + w].tobytes()
    return worst


def refusal_cases():
    """[(name, data, rows or None, n, v, parents mask, refused by the likelihood scores, refused by bge)]"""
    x5, x17, x48, deg = gauss_data(5, CHUNK + 1), gauss_data(17, 3 * CHUNK + 5), gauss_data(48, 3 * CHUNK + 5), degenerate_data()
    distinct = lambda k: np.arange(k, dtype=np.int32)[None, :] * 7 + 1
    return [
        ("p = cap", x17, None, 17, 16, mask_of(range(CAP)), False, False),
        ("p = cap + 1", x17, None, 17, 16, mask_of(range(CAP + 1)), True, True),
        ("m = p + 1", x5, distinct(3), 5, 4, mask_of([0, 1]), True, False),
        ("m = p + 2", x5, distinct(4), 5, 4, mask_of([0, 1]), False, False),
        ("m = 1", x5, distinct(1), 5, 2, 0, True, False),
        ("duplicated column", deg, None, 5, 0, mask_of([1, 3]), True, False),
        ("duplicate as child", deg, None, 5, 3, mask_of([1]), True, False),
        ("linear combination", deg, None, 5, 4, mask_of([0, 2]), True, False),
        ("linear combination among the parents", deg, None, 5, 1, mask_of([0, 2, 4]), True, False),
        ("neither", deg, None, 5, 4, mask_of([0, 1]), False, False),
        ("bit 47", x48, None, 48, 0, 1 << 47, False, False),
        ("bit >= n", x5, None, 5, 1, (1 << 5) | 1, True, True),
        ("bit 63", x17, None, 17, 1, 1 << 63, True, True),
    ]


def degenerate_singular(v, pm):
    """whether the family is singular in exact arithmetic on degenerate_data: a Fraction elimination of the exact C[fam][fam]"""
    ex = ExactMoments(degenerate_data())
    idx = bits_of(pm & ~(1 << v)) + [v]
    A = [[ex.C(i, j) for j in idx] for i in idx]
    for k in range(len(idx)):
        piv = next((r for r in range(k, len(idx)) if A[r][k] != 0), None)
        if piv is None:
            return True
        A[k], A[piv] = A[piv], A[k]
        for r in range(k + 1, len(idx)):
            f = A[r][k] / A[k][k]
            A[r] = [a - f * b for a, b in zip(A[r], A[k])]
    return False


def check_refusals(be):
    """every refusal case as the middle structure of three, sentinels around the buffers: NaN and bit 4 for the family alone"""
    for name, x, rows, n, v, pm, by_lik, by_bge in refusal_cases():
        mom = run_moments(be, x, rows)
        P = np.zeros((3, n), U64)
        P[1, v] = U64(pm)
        if n > 2:
            P[0, 1], P[2, 2] = U64(1), U64(1)
        for typ, refused in (("loglik-g", by_lik), ("bic-g", by_lik), ("bge", by_bge)):
            local, out, status = run_scores(be, mom, n, P, typ, guard=1)
            want_nan = np.zeros((3, n), bool)
            lonely = typ != "bge" and mom[0, 0] < 2          # m = 1: no family has a residual degree of freedom
            want_nan[1, v] = refused
            if lonely:
                want_nan[:] = True
            assert np.array_equal(np.isnan(local), want_nan), (name, typ, local)
            assert status == (16 if want_nan.any() else 0), (name, typ, status)
            assert np.array_equal(np.isnan(out), want_nan.any(1))
            assert math.isnan(restated_local(mom[0], n, v, pm, typ)) == refused, (name, typ)
            L, T, st = run_toggle(be, mom, n, P, typ)
            assert L.tobytes() == local.tobytes() and (st == 16 or not want_nan.any())
        coef, icpt, sd, status = run_fit(be, mom, n, P)
        if by_lik:
            assert status == 16 and np.isnan(coef[1, v]).all() and icpt[1, v] != icpt[1, v] and sd[1, v] != sd[1, v], name
            if mom[0, 0] >= 2:
                assert not np.isnan(coef[0]).any() and not np.isnan(sd[2]).any(), name
        else:
            assert status == 0 and not np.isnan(coef).any() and not np.isnan(sd).any(), name
    # the pivot rule is exact singularity on data whose moments are exact: every family of the degenerate data set
    deg = degenerate_data()
    mom = run_moments(be, deg)
    ex = ExactMoments(deg)
    assert mom[0, 6:].tobytes() == ex.C_float().tobytes(), "the degenerate data set's moments are exact in fp64"
    fams = score_families(5)
    P = np.zeros((len(fams), 5), U64)
    for b, (v, pa) in enumerate(fams):
        P[b, v] = U64(mask_of(pa))
    local, _, status = run_scores(be, mom, 5, P, "loglik-g")
    singular = [degenerate_singular(v, mask_of(pa)) for v, pa in fams]
    assert status == 16 and 0 < sum(singular) < len(fams)
    for b, (v, pa) in enumerate(fams):
        assert (local[b, v] != local[b, v]) == singular[b], (v, pa)


def toggle_case(n):
    B = {5: 8, 17: 4, 48: 2}[n]
    return gauss_data(n, 3 * CHUNK + 5), random_dags(n, B, 3, seed=n)


def check_toggles(be, n, variants=(("bic-g", None, None), ("bge", None, None))):
    """every cell against the scorer on the flipped structure, as bytes; two sets through set_of; a worklist pass"""
    x, P = toggle_case(n)
    B = len(P)
    rows = row_sets(len(x), len(x) - 9, n_sets=2)
    mom = run_moments(be, x, rows)
    set_of = np.arange(B, dtype=np.int32) % 2
    for variant in variants:
        typ, a1, a2 = variant_args(n, variant)
        L, T, status = run_toggle(be, mom, n, P, typ, a1, a2, set_of=set_of)
        local, _, st0 = run_scores(be, mom, n, P, typ, a1, a2, set_of=set_of)
        assert L.tobytes() == local.tobytes() and st0 == 0
        flipped = np.repeat(P, n * n, 0).reshape(B, n, n, n)
        for v in range(n):
            for u in range(n):
                if u != v:
                    flipped[:, v, u, v] ^= U64(1 << u)
        fl_local, _, st1 = run_scores(be, mom, n, flipped.reshape(-1, n), typ, a1, a2, set_of=np.repeat(set_of, n * n))
        fl_local = fl_local.reshape(B, n, n, n)
        want = np.stack([fl_local[:, v, :, v] for v in range(n)], 1)        # [B, v, u]
        eye = np.eye(n, dtype=bool)
        assert np.isnan(T[:, eye]).all()
        assert T[:, ~eye].tobytes() == want[:, ~eye].tobytes(), (n, typ)
        assert status == st1
        # a worklist pass writes only its rows: slot 2b names row (b + 1) % n, slot 2b + 1 is empty or a second row
        wl = np.full(2 * B, -1, np.int32)
        for b in range(B):
            wl[2 * b] = (b + 1) % n
            if b % 2 and n > 2:
                wl[2 * b + 1] = (b + 2) % n
        L2, T2, _ = run_toggle(be, mom, n, P, typ, a1, a2, set_of=set_of, worklist=wl)
        named = np.zeros((B, n), bool)
        for s, v in enumerate(wl):
            if v >= 0:
                named[s // 2, v] = True
        assert (L2 == SENTINEL).all()
        assert (T2[~named] == SENTINEL).all()
        off = np.broadcast_to(~eye, (B, n, n)) & named[:, :, None]
        assert T2[off].tobytes() == T[off].tobytes()
        assert (T2[np.broadcast_to(eye, (B, n, n)) & named[:, :, None]] == SENTINEL).all()


def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do)"""
    nan = NAN
    mom_ws = lambda **kw: lib.dvs_gbn_moments_workspace_bytes(*[kw.get(k, d) for k, d in (("n", 5), ("sets", 2), ("size", 300))])
    assert mom_ws() == 8 * 2 * 3 * (5 + 15) and mom_ws(n=0) == 0 and mom_ws(n=49) == 0 and mom_ws(sets=0) == 0 and mom_ws(size=0) == 0
    assert mom_ws(n=48, sets=1 << 20, size=1 << 20) == 0 and b"2^31" in lib.dvs_last_error()

    def moments(**kw):
        a = dict(n=5, S=300, data=ptr, rows=ptr, sets=2, size=300, ws=ptr, wsb=1 << 20, mom=ptr, momb=2 * 31 * 8)
        a.update(kw)
        return lib.dvs_gbn_moments(a["n"], a["S"], a["data"], a["rows"], a["sets"], a["size"], a["ws"], a["wsb"], a["mom"], a["momb"], None)
    assert moments(S=0) == 2 and moments(sets=0) == 2 and moments(size=0) == 2 and moments(n=0) == 3 and moments(n=49) == 3
    assert moments(rows=None) == 13 and moments(rows=None, sets=1, size=299) == 13
    assert moments(data=None) == 10 and moments(ws=None) == 10 and moments(mom=None) == 10
    assert moments(wsb=959) == 14 and b"960" in lib.dvs_last_error()
    assert moments(momb=495) == 14 and b"496" in lib.dvs_last_error()

    def scores(**kw):
        a = dict(B=4, n=5, mom=ptr, sets=1, set_of=None, parents=ptr, typ=2, a1=nan, a2=nan, local=ptr, out=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_scores(a["B"], a["n"], a["mom"], a["sets"], a["set_of"], a["parents"], a["typ"], a["a1"], a["a2"], a["local"],
                                  a["out"], a["status"], None)

    def toggle(**kw):
        a = dict(B=4, n=5, mom=ptr, sets=1, set_of=None, parents=ptr, typ=2, a1=nan, a2=nan, wl=None, L=ptr, Lb=4 * 5 * 8, T=ptr, Tb=4 * 25 * 8,
                 status=ptr)
        a.update(kw)
        return lib.dvs_gbn_toggle_scores(a["B"], a["n"], a["mom"], a["sets"], a["set_of"], a["parents"], a["typ"], a["a1"], a["a2"], a["wl"],
                                         a["L"], a["Lb"], a["T"], a["Tb"], a["status"], None)
    for fn in (scores, toggle):
        assert fn(B=0) == 2 and fn(sets=0) == 2 and fn(n=0) == 3 and fn(n=49) == 3
        assert fn(typ=-1) == 12 and fn(typ=4) == 12
        assert fn(typ=0, a1=1.0) == 13 and fn(typ=0, a2=1.0) == 13
        for typ in (1, 2):
            assert fn(typ=typ, a1=-1.0) == 13 and fn(typ=typ, a1=float("inf")) == 13 and fn(typ=typ, a2=7.0) == 13
        assert fn(typ=3, a1=0.0) == 13 and fn(typ=3, a1=float("inf")) == 13 and fn(typ=3, a2=6.0) == 13 and fn(typ=3, a2=float("inf")) == 13
        assert fn(mom=None) == 10 and fn(parents=None) == 10 and fn(status=None) == 10
    assert scores(local=None) == 10 and scores(out=None) == 10
    assert toggle(B=1 << 20, n=48) == 2 and toggle(L=None) == 10 and toggle(T=None) == 10
    assert toggle(Lb=159) == 14 and b"160" in lib.dvs_last_error()
    assert toggle(Tb=799) == 14 and b"800" in lib.dvs_last_error()

    def fit(**kw):
        a = dict(B=4, n=5, mom=ptr, sets=1, set_of=None, parents=ptr, coef=ptr, cb=4 * 25 * 8, icpt=ptr, sd=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_fit(a["B"], a["n"], a["mom"], a["sets"], a["set_of"], a["parents"], a["coef"], a["cb"], a["icpt"], a["sd"],
                               a["status"], None)
    assert fit(B=0) == 2 and fit(sets=0) == 2 and fit(n=49) == 3 and fit(B=1 << 20, n=48) == 2
    for k in ("mom", "parents", "coef", "icpt", "sd", "status"):
        assert fit(**{k: None}) == 10
    assert fit(cb=799) == 14 and b"800" in lib.dvs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# Score equivalence of the bge restatement (mpmath): the constants of the Kuipers correction
# ---------------------------------------------------------------------------------------------------------------------
def all_dags(n):
    """every DAG on n vertices as int64 [D, n] parent masks (25 on 3, 543 on 4, 29 281 on 5): all combinations of parent sets,
    kept where peeling off the variables without a remaining parent empties the graph"""
    k = 1 << (n - 1)
    codes = np.indices((k,) * n).reshape(n, -1).T
    P = np.empty_like(codes)
    for v in range(n):
        c = codes[:, v]
        P[:, v] = (c & ((1 << v) - 1)) | ((c >> v) << (v + 1))              # a zero at the variable's own bit
    left = np.full(len(P), (1 << n) - 1)
    for _ in range(n):
        free = np.zeros(len(P), np.int64)
        for v in range(n):
            free |= (((P[:, v] & left) == 0) & (((left >> v) & 1) == 1)).astype(np.int64) << v
        left &= ~free
    return P[left == 0]


def cpdag_key(P):
    """(skeleton, v-structures) of a DAG given as parent masks: equal keys <=> Markov equivalent (Verma and Pearl)"""
    n = len(P)
    adj = {frozenset((u, v)) for v in range(n) for u in bits_of(P[v])}
    vs = {(min(a, b), v, max(a, b)) for v in range(n) for a in bits_of(P[v]) for b in bits_of(P[v]) if a < b and frozenset((a, b)) not in adj}
    return frozenset(adj), frozenset(vs)


# ---------------------------------------------------------------------------------------------------------------------
# The searches on a Gaussian evaluator (tests/test_gpu_gaussian.py): tolerances from the reference alone
# ---------------------------------------------------------------------------------------------------------------------
SEARCH_N, SEARCH_S = 6, 2000


def ordered_forbidden(n):
    """bit u of row v for every u > v: only arcs from a lower to a higher index are allowed.  Score-equivalent moves (the two
    directions of an arc between the same families, covered reversals) tie in exact arithmetic under every Gaussian score
    here, so a selection among them has no gap to its runner-up; under a fixed order no two legal moves are equivalent."""
    return np.asarray([mask_of(range(v + 1, n)) for v in range(n)], U64)


@functools.lru_cache(maxsize=None)
@at60
def family_table(n, S, typ, seed=0):
    """(scores float64 [n][2^n] of (v, parent mask without v) from mpmath, NaN where the mask holds v; the largest bound)"""
    ref = Reference(exact_of(n, S, seed), restated_moments(gauss_data(n, S, seed))[0, 1:1 + n])
    table, worst = np.full((n, 1 << n), NAN), 0.0
    for v in range(n):
        for pm in range(1 << n):
            if not (pm >> v) & 1:
                want, bound = ref.local(v, bits_of(pm), typ)
                table[v, pm], worst = float(want), max(worst, bound)
    return table, worst


def selection_gap(moves):
    """moves: [(code, delta)] without NaNs -> best delta minus the runner-up's (inf with fewer than two)"""
    d = sorted((float(x) for _, x in moves), reverse=True)
    return d[0] - d[1] if len(d) > 1 else float("inf")
