"""TEST HELPER: cases, references and the checks themselves for the exact arc posterior (csrc/dvs_posterior.h:
dvs_arc_posterior_workspace_bytes, dvs_arc_posterior; dags_vae_search_amd/posterior.py), written once and run by
tests/test_emu_posterior.py (emulator build) and tests/test_gpu_posterior.py (device).  tests/test_posterior_ref.py pins the
references themselves on the CPU.

References (mpmath, numpy and plain Python, nothing shared with the kernels)
  ref_brute  60-digit mpmath, n <= 5: every labelled DAG (tests/cpdag_corpus.all_dags through exact_corpus.dag_rows) weighted
             by its number of linear extensions times exp(sum of its cells), filtered by the cap, the blacklist and NaN.
  ref_dp     the recurrences of include/dvs.h (dvs_arc_posterior) in numpy fp64 with np.logaddexp.
  ref_mp     the same recurrences in 60-digit mpmath in the linear domain, exact products of exp(f - max_v f(v, .)).
ref_dp is pinned against ref_brute for n <= 5 and against ref_mp at n = 6 and 7 (tests/test_posterior_ref.py).

Tolerance (derived, not tuned).  The device and the emulator use different exp and log, so byte equality with numpy is not
available.  With
    M = sum_v max_P |f(v, P)| + n^2      (every log-domain value of the programme is a sum of at most one f per variable plus
                                          the log of a count of at most n! 2^(n(n-1)/2) <= e^(n^2) terms: magnitude <= M)
    D = 2 (n^2 + 3 n + 4)                (the longest chain of dependent log-adds and additions from a table cell to gamma:
                                          n folds for alpha, n levels of n + 1 operations for a chain, one addition and n folds
                                          for gamma, a handful for the ends; doubled)
the log-domain bound is
    eps = D (2^-53 M + 2^-50):
each operation rounds a value of magnitude <= M by half an ulp (first term) and each exp / log pair is allowed 8 ulp at
magnitude 1 (second term: a log-add's correction log(1 + exp(-d)) is at most ln 2, a chain cell's log(sum) at most ln n).
A log-add does not amplify the errors of its operands (the result's derivative with respect to them sums to 1), so errors
add along the chain.  log_z, log_z_back, L, Rb and gamma are within eps of the truth; prob and family = exp(f + gamma - log_z)
are within 2 eps + n 2^-52 (two log-domain errors in an exponent <= 0, then at most 2^n terms of total 1 added in a tree
and in rows: n 2^-52 covers their rounding).  Against ref_dp, which has its own rounding of the same size, eps is doubled.
alpha shares its cells with gamma and is dead once the chains are done, so it is not readable after a call: it is pinned
through L and Rb, of which every specified alpha cell is a term.

Sizes of the stage checks (STAGE_SIZES): k_post_lse takes ceil(n / 8) LDS passes, so 8 is the last size whose whole table is
one tile and 9 the first with a cross-tile pass, 17 the first with three; k_post_chain walks all levels in one workgroup up
to n = 9 and takes one launch per level from 10 on; k_post_arcs has one workgroup per table up to n = 8 and several above.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np

from tests import exact_corpus as ex
from tests.abi_cases import call, entry, run

U64 = np.uint64
INF = float("inf")
STAGE_SIZES = (6, 8, 9, 10, 12, 17)
BIG = 17                     # only the plain random table, batch 1: 2.2 M cells
KINDS = ("random", "ties", "nan", "prior")
SETTINGS = {"random": (None, False), "ties": (3, True), "nan": (None, False), "prior": (None, False)}   # (max_parents, blacklist)
MP_DIGITS = 60


# ---------------------------------------------------------------------------------------------------------------------
# Tolerance
# ---------------------------------------------------------------------------------------------------------------------
def f_cells(table, max_parents=None, forbidden=None, size_prior=None):
    """f(v, P) of include/dvs.h: f64 [2^n, n], -inf where P is not admissible for v"""
    rows, n = table.shape
    ok = ex.admissible(n, max_parents, forbidden, table)
    f = np.where(ok, np.nan_to_num(table, nan=0.0), -INF)
    if size_prior is not None:
        f = np.where(ok, f + np.asarray(size_prior, np.float64)[np.minimum(ex.popcounts(n), n - 1)][:, None], -INF)
    return f


def eps_of(f):
    """the log-domain bound of the module docstring for the cells f [2^n, n]"""
    n = f.shape[1]
    M = n * n + sum(float(np.abs(col[np.isfinite(col)]).max()) if np.isfinite(col).any() else 0.0 for col in f.T)
    return 2 * (n * n + 3 * n + 4) * (2.0 ** -53 * M + 2.0 ** -50)


def prob_tol(eps, n):
    return 2 * eps + n * 2.0 ** -52


def assert_close(got, want, tol, what):
    """no NaN, -inf exactly where the reference has it, everything else within tol"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any() and not np.isnan(want).any(), (what, "NaN")
    low = want == -INF
    assert ((got == -INF) == low).all(), (what, "-inf cells differ")
    assert np.isfinite(got[~low]).all(), (what, "+inf")
    err = float(np.abs(got[~low] - want[~low]).max()) if (~low).any() else 0.0
    assert err <= tol, (what, err, tol)
    return err


# ---------------------------------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_extensions(n):
    """int64 [DAGs]: the number of variable orders each DAG of exact_corpus.dag_rows(n) is consistent with"""
    D = ex.dag_rows(n)
    ext = np.zeros((len(D), 1 << n), np.int64)
    ext[:, 0] = 1
    for W in range(1, 1 << n):
        for v in range(n):
            if (W >> v) & 1:
                prev = W ^ (1 << v)
                ext[:, W] += np.where((D[:, v] & ~prev) == 0, ext[:, prev], 0)
    return ext[:, -1]


def ref_brute(table, max_parents=None, forbidden=None, size_prior=None):
    """-> namespace(prob [n, n], log_z, family [2^n, n], flag) by enumeration in mpmath; n <= 5"""
    import mpmath as mpm
    rows, n = table.shape
    assert rows == 1 << n and n <= 5
    f = f_cells(table, max_parents, forbidden, size_prior)
    D, ext = ex.dag_rows(n), linear_extensions(n)
    fine = np.ones(len(D), bool)
    for v in range(n):
        fine &= f[D[:, v], v] > -INF
    prob, family = np.zeros((n, n)), np.zeros((rows, n))
    if not fine.any():
        return SimpleNamespace(prob=prob, log_z=-INF, family=family, flag=1)
    with mpm.workdps(MP_DIGITS):
        fm = {(P, v): mpm.mpf(float(f[P, v])) for P in range(rows) for v in range(n) if f[P, v] > -INF}
        Z = mpm.mpf(0)
        fam = {}
        for d in np.nonzero(fine)[0]:
            P = [int(p) for p in D[d]]
            w = int(ext[d]) * mpm.exp(mpm.fsum(fm[(P[v], v)] for v in range(n)))
            Z += w
            for v in range(n):
                fam[(P[v], v)] = fam.get((P[v], v), 0) + w
        for (P, v), w in fam.items():
            family[P, v] = float(w / Z)
        for u in range(n):
            for v in range(n):
                prob[u, v] = float(mpm.fsum(w for (P, vv), w in fam.items() if vv == v and (P >> u) & 1) / Z)
        log_z = float(mpm.log(Z))
    return SimpleNamespace(prob=prob, log_z=log_z, family=family, flag=0)


def ref_dp(table, max_parents=None, forbidden=None, size_prior=None):
    """the recurrences of include/dvs.h in numpy -> namespace(f, alpha, L, Rb, gamma, family, prob, log_z, log_z_back, flag)"""
    rows, n = table.shape
    assert rows == 1 << n
    full = rows - 1
    f = f_cells(table, max_parents, forbidden, size_prior)
    S = np.arange(rows, dtype=np.int64)
    pop = ex.popcounts(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = f.copy()
        for i in range(n):
            into = S[(S >> i) & 1 == 1]
            alpha[into] = np.logaddexp(alpha[into], alpha[into ^ (1 << i)])
        L, Rb = np.zeros(rows), np.zeros(rows)
        for k in range(1, n + 1):
            W = S[pop == k]
            tl, tr = np.full((len(W), n), -INF), np.full((len(W), n), -INF)
            for s in range(n):
                has = (W >> s) & 1 == 1
                prev = W[has] ^ (1 << s)
                tl[has, s] = alpha[prev, s] + L[prev]
                tr[has, s] = alpha[full ^ W[has], s] + Rb[prev]
            L[W], Rb[W] = np.logaddexp.reduce(tl, axis=1), np.logaddexp.reduce(tr, axis=1)
        gamma = np.full((rows, n), -INF)
        for v in range(n):
            out = S[(S >> v) & 1 == 0]
            gamma[out, v] = L[out] + Rb[full ^ out ^ (1 << v)]
        for i in range(n):
            into = S[(S >> i) & 1 == 0]
            gamma[into] = np.logaddexp(gamma[into], gamma[into | (1 << i)])
        log_z, log_z_back = float(L[full]), float(Rb[full])
        flag = int(log_z == -INF)
        family = np.zeros((rows, n))
        if not flag:
            e = f + gamma - log_z
            family = np.where(f > -INF, np.exp(np.where(f > -INF, e, 0.0)), 0.0)
    prob = np.stack([family[(S >> u) & 1 == 1].sum(0) for u in range(n)])
    return SimpleNamespace(f=f, alpha=alpha, L=L, Rb=Rb, gamma=gamma, family=family, prob=prob, log_z=log_z,
                           log_z_back=log_z_back, flag=flag)


def ref_mp(table, max_parents=None, forbidden=None, size_prior=None):
    """the same recurrences in mpmath, linear domain with the per-column shifts m_v = max_P f(v, P): exact products, sums at 60
    digits; returned as correctly rounded fp64 logs -> namespace(L, Rb, gamma, family, prob, log_z, log_z_back, flag)"""
    import mpmath as mpm
    rows, n = table.shape
    full = rows - 1
    f = f_cells(table, max_parents, forbidden, size_prior)
    with mpm.workdps(MP_DIGITS):
        zero, one = mpm.mpf(0), mpm.mpf(1)
        m = [float(f[:, v].max()) if (f[:, v] > -INF).any() else 0.0 for v in range(n)]
        shift = [mpm.fsum(mpm.mpf(m[v]) for v in range(n) if (W >> v) & 1) for W in range(rows)]
        a = [[mpm.exp(mpm.mpf(float(f[P, v])) - mpm.mpf(m[v])) if f[P, v] > -INF else zero for v in range(n)] for P in range(rows)]
        al = [row[:] for row in a]
        for i in range(n):
            for W in range(rows):
                if (W >> i) & 1:
                    src = al[W ^ (1 << i)]
                    al[W] = [x + y for x, y in zip(al[W], src)]
        Ll, Rl = [zero] * rows, [zero] * rows
        Ll[0] = Rl[0] = one
        for W in sorted(range(1, rows), key=lambda w: bin(w).count("1")):
            bits = [v for v in range(n) if (W >> v) & 1]
            Ll[W] = mpm.fsum(al[W ^ (1 << v)][v] * Ll[W ^ (1 << v)] for v in bits)
            Rl[W] = mpm.fsum(al[full ^ W][v] * Rl[W ^ (1 << v)] for v in bits)
        g = [[Ll[P] * Rl[full ^ P ^ (1 << v)] if not (P >> v) & 1 else zero for v in range(n)] for P in range(rows)]
        for i in range(n):
            for P in range(rows):
                if not (P >> i) & 1:
                    src = g[P | (1 << i)]
                    g[P] = [x + y for x, y in zip(g[P], src)]

        def lg(x, s):
            return float(mpm.log(x) + s) if x > 0 else -INF
        L = np.array([lg(Ll[W], shift[W]) for W in range(rows)])
        Rb = np.array([lg(Rl[W], shift[W]) for W in range(rows)])
        gamma = np.array([[lg(g[P][v], shift[full ^ (1 << v)]) for v in range(n)] for P in range(rows)])
        Z = Ll[full]
        flag = int(not Z > 0)
        family, prob = np.zeros((rows, n)), np.zeros((n, n))
        if not flag:
            fam = [[a[P][v] * g[P][v] / Z for v in range(n)] for P in range(rows)]          # the shifts cancel: sum_w m_w each
            family = np.array([[float(x) for x in row] for row in fam])
            prob = np.array([[float(mpm.fsum(fam[P][v] for P in range(rows) if (P >> u) & 1)) for v in range(n)] for u in range(n)])
    return SimpleNamespace(f=f, L=L, Rb=Rb, gamma=gamma, family=family, prob=prob, log_z=float(L[full]),
                           log_z_back=float(Rb[full]), flag=flag)


# ---------------------------------------------------------------------------------------------------------------------
# Driver: dvs_arc_posterior through the raw C ABI on a back end of scoring_corpus
# ---------------------------------------------------------------------------------------------------------------------
def split(n):
    """(rows, sweeps, groups) of include/dvs.h: how the arc kernel divides the parent sets of a table"""
    rows = 256 // n
    sweeps = max(8, -(-(1 << n) // (rows * 2048)))
    return rows, sweeps, -(-(1 << n) // (rows * sweeps))


def layout(batch, n):
    """byte offsets of gamma, L, Rb, the partial sums and the total, as include/dvs.h documents them"""
    up = lambda x: (x + 255) & ~255
    subsets = batch << n
    L = up(subsets * n * 8)
    Rb = L + up(subsets * 8)
    partial = Rb + up(subsets * 8)
    return 0, L, Rb, partial, partial + up(batch * split(n)[2] * n * n * 8)


class Driver:
    def __init__(self, be):
        self.be, self.lib = be, be.lib

    def posterior(self, tables, max_parents=None, forbidden=None, size_prior=None, family=True):
        """one dvs_arc_posterior on f64 [B, 2^n, n] -> every output and every stage of the workspace; the workspace starts as
        all-ones bytes (NaN as f64: a cell read before it is written poisons the result), the outputs as -7"""
        be, lib = self.be, self.lib
        tables = np.ascontiguousarray(tables, np.float64)
        B, rows, n = tables.shape
        assert rows == 1 << n
        o_g, o_L, o_R, o_p, total = layout(B, n)
        assert lib.dvs_arc_posterior_workspace_bytes(B, n) == total
        hT, ws = be.put(tables), be.put(np.full(total, 0xFF, np.uint8))
        hp, hz = be.put(np.full((B, n, n), -7.0)), be.put(np.full((B, 2), -7.0))
        hf = be.put(np.full(B, -7, np.int32))
        hfam = be.put(np.full((B, rows, n), -7.0)) if family else None
        forb = None if forbidden is None else be.put(np.ascontiguousarray(forbidden, U64))
        prior = None if size_prior is None else be.put(np.ascontiguousarray(size_prior, np.float64))
        call(be, "dvs_arc_posterior", batch=B, n_vars=n, table=hT, table_bytes=tables.nbytes, max_parents=max_parents or 0,
             forbidden=forb, size_prior=prior, workspace=ws, workspace_bytes=total, prob=hp, log_z=hz, family=hfam,
             family_bytes=tables.nbytes if family else 0, flags=hf)
        w = be.get(ws).copy()
        assert be.get(hT).tobytes() == tables.tobytes()                    # the input is not written
        cells, G = B * rows * n, split(n)[2]
        z = be.get(hz).copy()
        return SimpleNamespace(
            ws=w, gamma=w[o_g:o_g + cells * 8].view(np.float64).reshape(B, rows, n),
            L=w[o_L:o_L + B * rows * 8].view(np.float64).reshape(B, rows),
            Rb=w[o_R:o_R + B * rows * 8].view(np.float64).reshape(B, rows),
            partial=w[o_p:o_p + B * G * n * n * 8].view(np.float64).reshape(B, G, n, n),
            prob=be.get(hp).copy(), log_z=z[:, 0].copy(), log_z_back=z[:, 1].copy(), both=z,
            family=be.get(hfam).copy() if family else np.zeros((B, 0, n)), flags=be.get(hf).copy())


OUTPUTS = ("ws", "prob", "both", "family", "flags")
STAGES = ("gamma", "L", "Rb", "partial", "prob", "both", "family", "flags")


def same_bytes(a, b, fields=OUTPUTS):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in fields)


def row_of(r, t):
    return SimpleNamespace(**{f: getattr(r, f)[t:t + 1] for f in STAGES})


def assert_matches(got, t, ref, eps, what, stages=True):
    """table t of a result against a reference, log-domain tolerance eps; -> the largest errors (log domain, linear domain)"""
    n = got.prob.shape[-1]
    assert int(got.flags[t]) == ref.flag, (what, "flag")
    e_log = max(assert_close(got.log_z[t], ref.log_z, eps, (what, "log_z")),
                assert_close(got.log_z_back[t], ref.log_z_back if hasattr(ref, "log_z_back") else ref.log_z, eps, (what, "log_z_back")))
    if stages:
        e_log = max(e_log, assert_close(got.L[t], ref.L, eps, (what, "L")), assert_close(got.Rb[t], ref.Rb, eps, (what, "Rb")),
                    assert_close(got.gamma[t], ref.gamma, eps, (what, "gamma")))
    tol = prob_tol(eps, n)
    e_lin = max(assert_close(got.prob[t], ref.prob, tol, (what, "prob")), assert_close(got.family[t], ref.family, tol, (what, "family")))
    assert (np.diagonal(got.prob[t]) == 0.0).all(), (what, "diagonal")
    return e_log, e_lin


# ---------------------------------------------------------------------------------------------------------------------
# Tables
# ---------------------------------------------------------------------------------------------------------------------
def make_tables(kind, batch, n, seed, scale=3.0):
    rng = np.random.default_rng(seed)
    shape = (batch, 1 << n, n)
    if kind == "ties":
        return rng.choice(np.array([-1.5, 0.25, 2.0]), shape)
    t = rng.standard_normal(shape) * scale
    if kind == "nan":
        t[rng.random(shape) < 0.15] = np.nan
        t[:, 0, :] = rng.standard_normal((batch, n))      # the empty parent set stays available: no flag here
    return t


def settings(kind, n, seed):
    """-> (max_parents, forbidden, size_prior) of a kind"""
    cap, with_forb = SETTINGS[kind]
    forb = ex.random_forbidden(np.random.default_rng(seed), n, 0.15) if with_forb else None
    prior = np.random.default_rng(seed + 1).standard_normal(n) * 2.0 if kind == "prior" else None
    return cap, forb, prior


# ---------------------------------------------------------------------------------------------------------------------
# 1. Brute force, n <= 5
# ---------------------------------------------------------------------------------------------------------------------
BRUTE_BATCH = 2


@functools.lru_cache(maxsize=None)
def brute_case(n, kind):
    tables = make_tables(kind, BRUTE_BATCH, n, seed=100 * n + KINDS.index(kind))
    cap, forb, prior = settings(kind, n, n)
    if kind == "ties" and n >= 3:
        forb[1] |= U64(1)                                  # at least one forbidden arc: 0 -> 1
    return tables, cap, forb, prior, [ref_brute(tables[t], cap, forb, prior) for t in range(BRUTE_BATCH)]


def check_brute(drv, n, kind):
    tables, cap, forb, prior, refs = brute_case(n, kind)
    got = drv.posterior(tables, cap, forb, prior)
    assert not got.flags.any()
    worst = (0.0, 0.0)
    for t in range(BRUTE_BATCH):
        eps = eps_of(f_cells(tables[t], cap, forb, prior))
        worst = max(worst, assert_matches(got, t, refs[t], eps, (n, kind, t), stages=False))
        assert abs(got.log_z[t] - got.log_z_back[t]) <= 2 * eps
        if forb is not None:
            for v in range(n):
                for u in range(n):
                    if (int(forb[v]) >> u) & 1:
                        assert got.prob[t, u, v].tobytes() == np.float64(0.0).tobytes(), (n, kind, u, v)
        if n == 1:
            f0 = tables[t, 0, 0] + (0.0 if prior is None else prior[0])
            assert got.prob[t].tolist() == [[0.0]] and got.log_z[t] == f0 == got.log_z_back[t] and got.family[t].tolist() == [[1.0], [0.0]]
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 2. Every stage against ref_dp; a batch is its rows
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stage_case(n, kind):
    batch = 3 if n <= 10 else 1
    tables = make_tables(kind, batch, n, seed=1000 * n + KINDS.index(kind))
    cap, forb, prior = settings(kind, n, n)
    return tables, cap, forb, prior, [ref_dp(tables[t], cap, forb, prior) for t in range(batch)]


def check_stages(drv, n, kind):
    """every workspace stage and every output against ref_dp (twice the bound: ref_dp rounds too); at batch 3 a table's
    results are, byte for byte, those of the table run alone"""
    tables, cap, forb, prior, refs = stage_case(n, kind)
    got = drv.posterior(tables, cap, forb, prior)
    assert not got.flags.any()
    worst = (0.0, 0.0)
    for t in range(len(tables)):
        eps = eps_of(refs[t].f)
        worst = max(worst, assert_matches(got, t, refs[t], 2 * eps, (n, kind, t)))
        assert abs(got.log_z[t] - got.log_z_back[t]) <= 2 * eps
        # the partial sums of the workspace add up to prob in k_post_finish's order: lane i takes i, i + 256, ..., then a tree
        red = np.zeros((256, n, n))
        for g in range(got.partial.shape[1]):
            red[g % 256] += got.partial[t, g]
        for s in (128, 64, 32, 16, 8, 4, 2, 1):
            red[:s] += red[s:2 * s]
        assert red[0].tobytes() == got.prob[t].tobytes()
    if len(tables) > 1:
        alone = drv.posterior(tables[1:2], cap, forb, prior)
        assert same_bytes(row_of(got, 1), alone, STAGES), (n, kind)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 3. Closed form on the all-zero table
# ---------------------------------------------------------------------------------------------------------------------
def closed_form(n, cap):
    """(log_z, the off-diagonal prob) of the all-zero table: every order weighs prod_i sum_{j <= cap} C(i, j), i the number
    of predecessors, so the orders are equally likely; v has i predecessors with probability 1 / n, u is one of them with
    probability i / (n - 1) and then in the parent set with probability sum_{1 <= j <= cap} C(i - 1, j - 1) / sum_{j <= cap} C(i, j)"""
    k = n if cap is None else cap
    sets = [sum(math.comb(i, j) for j in range(min(i, k) + 1)) for i in range(n)]
    log_z = math.lgamma(n + 1) + sum(math.log(s) for s in sets)
    if n == 1:
        return log_z, 0.0
    p = sum(i / (n - 1) * sum(math.comb(i - 1, j - 1) for j in range(1, min(i, k) + 1)) / sets[i] for i in range(n)) / n
    return log_z, p


def check_closed_form(drv, n, cap):
    got = drv.posterior(np.zeros((1, 1 << n, n)), cap, family=n < BIG)
    log_z, p = closed_form(n, cap)
    if cap is None:
        assert abs(log_z - (math.lgamma(n + 1) + n * (n - 1) / 2 * math.log(2.0))) <= 1e-12 * max(1.0, log_z) and (n == 1 or p == 0.25)
    eps = 2 * (n * n + 3 * n + 4) * (2.0 ** -53 * n * n + 2.0 ** -50)
    assert got.flags.tolist() == [0]
    assert abs(got.log_z[0] - log_z) <= eps and abs(got.log_z_back[0] - log_z) <= eps, (n, cap, got.both, log_z, eps)
    want = np.full((n, n), p)
    np.fill_diagonal(want, 0.0)
    err = assert_close(got.prob[0], want, prob_tol(eps, n), (n, cap, "prob"))
    return abs(got.log_z[0] - log_z), err


# ---------------------------------------------------------------------------------------------------------------------
# 4. Range: tables whose exp underflows in fp64
# ---------------------------------------------------------------------------------------------------------------------
def range_tables(which, n):
    rng = np.random.default_rng(40 + n)
    shape = (1, 1 << n, n)
    if which == "offsets":                                 # non-trivial probabilities, exp(f) = 0
        return -10000.0 * (np.arange(n) + 1.0)[None, None, :] + 3.0 * rng.standard_normal(shape)
    return 3000.0 * rng.standard_normal(shape) - 9000.0    # "dominated": one DAG carries all the mass


@functools.lru_cache(maxsize=None)
def range_case(which, n):
    tables = range_tables(which, n)
    return tables, ref_dp(tables[0])


def check_range(drv, which, n):
    tables, ref = range_case(which, n)
    assert which != "offsets" or (np.exp(tables) == 0.0).all()
    got = drv.posterior(tables)
    eps = eps_of(ref.f)
    tol = prob_tol(eps, n)
    for f in ("gamma", "L", "Rb", "prob", "both", "family"):
        assert not np.isnan(getattr(got, f)).any(), f
    worst = assert_matches(got, 0, ref, 2 * eps, (which, n))
    assert abs(got.log_z[0] - got.log_z_back[0]) <= 2 * eps
    assert np.abs(got.family[0].sum(0) - 1.0).max() <= tol, (which, n, got.family[0].sum(0))
    assert (got.prob[0] + got.prob[0].T <= 1.0 + tol).all() and (got.prob[0] >= 0.0).all()
    if which == "offsets":
        assert ((got.prob[0] > 0.01) & (got.prob[0] < 0.99)).sum() >= n        # the probabilities are not trivial
    else:
        best = ex.ref_dp(tables[0]).parents
        want = np.array([[float((int(best[v]) >> u) & 1) for v in range(n)] for u in range(n)])
        assert_close(got.prob[0], want, tol, (which, n, "one DAG"))
    return worst


def dominated(n):
    """(tables [1, 2^n, n], the parent masks of the DAG that carries the mass)"""
    tables = range_tables("dominated", n)
    return tables, ex.ref_dp(tables[0]).parents


# ---------------------------------------------------------------------------------------------------------------------
# 5. Flags
# ---------------------------------------------------------------------------------------------------------------------
def check_flags(drv, n):
    """Batch 2, table 1 is the bad one.  With only table[0][v] NaN, variable v cannot stand without parents: at n = 1 that is
    the whole column and no DAG is admissible; at n > 1 the definitions of include/dvs.h leave v its non-empty parent sets, so
    DAGs exist (v is never first in an order), no flag is set and the result is ref_dp's with family[0][v] exactly 0.  With
    the whole column of v NaN no DAG is admissible at any n: flag 1, prob and family all zero, log_z -inf, no NaN anywhere, for
    that table alone."""
    v = n // 2
    tables = make_tables("random", 2, n, seed=7 + n)
    clean = drv.posterior(tables)
    assert clean.flags.tolist() == [0, 0]
    tables[1, 0, v] = np.nan
    got = drv.posterior(tables)
    if n > 1:
        ref = ref_dp(tables[1])
        assert got.flags.tolist() == [0, 0]
        assert_matches(got, 1, ref, 2 * eps_of(ref.f), ("empty set only", n))
        assert got.family[1, 0, v] == 0.0 and got.L[1, 1 << v] == -INF
    tables[1, :, v] = np.nan
    got = drv.posterior(tables)
    assert got.flags.tolist() == [0, 1]
    assert got.log_z[1] == -INF and got.log_z_back[1] == -INF
    assert not got.prob[1].any() and not got.family[1].any()
    for f in ("gamma", "L", "Rb", "partial", "prob", "both", "family"):
        assert not np.isnan(getattr(got, f)).any(), f
    assert same_bytes(row_of(got, 0), row_of(clean, 0), STAGES)
    ref = ref_dp(tables[1])
    assert ref.flag == 1
    assert_matches(got, 1, ref, 2 * eps_of(ref.f), ("flags", n))


# ---------------------------------------------------------------------------------------------------------------------
# 6. Determinism
# ---------------------------------------------------------------------------------------------------------------------
def check_determinism(drv, n=10, batch=2):
    tables = make_tables("nan", batch, n, seed=5)
    cap, forb, prior = 4, ex.random_forbidden(np.random.default_rng(5), n, 0.1), np.linspace(0.0, -2.0, n)
    a = drv.posterior(tables, cap, forb, prior)
    b = drv.posterior(tables, cap, forb, prior)
    assert not a.flags.any() and same_bytes(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 7. Real data: `real` is an exact_corpus.EmuReal or a test_gpu_exact.GpuReal (table, search)
# ---------------------------------------------------------------------------------------------------------------------
def check_real_asia(real, drv):
    """asia, uncapped: against the mpmath programme within eps, the two summation orders within eps of each other, and every
    arc of exact search's optimum with positive strength"""
    n = real.n
    table = real.table(None)
    ref = ref_mp(table)
    eps = eps_of(ref.f)
    got = drv.posterior(table[None])
    e_log, e_lin = assert_matches(got, 0, ref, eps, ("asia", real.typ))
    assert abs(got.log_z[0] - got.log_z_back[0]) <= eps, (got.both, eps)
    parents = real.search(table, None, None)[0]
    strength = got.prob[0] + got.prob[0].T
    arcs = [(u, v) for v in range(n) for u in range(n) if (int(parents[v]) >> u) & 1]
    assert arcs and all(strength[u, v] > 0.0 for u, v in arcs)
    print(f"\nasia {real.typ}: log_z {got.log_z[0]!r} back {got.log_z_back[0]!r} eps {eps:.3e} worst log error {e_log:.3e} "
          f"worst prob error {e_lin:.3e}; weakest optimal arc {min(strength[u, v] for u, v in arcs):.6f}")
    return e_log, e_lin


def check_real_capped(real, drv, cap):
    """a capped table (sachs at 3 parents) against ref_dp"""
    table = real.table(cap)
    ref = ref_dp(table, cap)
    eps = eps_of(ref.f)
    got = drv.posterior(table[None], cap)
    worst = assert_matches(got, 0, ref, 2 * eps, ("capped", real.typ))
    assert abs(got.log_z[0] - got.log_z_back[0]) <= 2 * eps
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 8. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    """(entry point, arguments, return code, text dvs_last_error must contain) of dvs_arc_posterior: every check, and the pairs
    where two checks fail and the earlier one decides.  D: a dummy non-null pointer, never dereferenced."""
    tb, wb = 3 * 256 * 8 * 8, layout(3, 8)[4]
    cases = []
    c = entry("dvs_arc_posterior", cases, batch=3, n_vars=8, table=D, table_bytes=tb, max_parents=0, forbidden=None,
              size_prior=None, workspace=D, workspace_bytes=wb, prob=D, log_z=D, family=None, family_bytes=0, flags=D, stream=None)
    big = dict(table_bytes=1 << 40, workspace_bytes=1 << 40)
    c(2, "batch must be > 0", batch=0)
    c(2, "batch must be > 0", batch=-2)
    c(3, "n_vars must be in [1, 20]", n_vars=0)
    c(3, "n_vars must be in [1, 20]", n_vars=21)
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=128, n_vars=20, **big)      # 2^27 * 20 > 2^31
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=1 << 30, n_vars=1, **big)   # 2^31 exactly
    for name in ("table", "workspace", "prob", "log_z", "flags"):
        c(10, "null pointer", **{name: None})
    c(14, f"table_bytes < batch * 2^n_vars * n_vars * 8 = {tb}", table_bytes=tb - 1)
    c(14, f"workspace_bytes < dvs_arc_posterior_workspace_bytes = {wb}", workspace_bytes=wb - 1)
    c(14, f"workspace_bytes < dvs_arc_posterior_workspace_bytes = {layout(5, 20)[4]}", batch=5, n_vars=20, table_bytes=1 << 40,
      workspace_bytes=0)
    c(14, f"family_bytes < batch * 2^n_vars * n_vars * 8 = {tb}", family=D, family_bytes=tb - 1)
    c(2, "batch must be > 0", batch=0, n_vars=21)                                      # batch before n_vars
    c(3, "n_vars must be in [1, 20]", batch=1 << 30, n_vars=21)                        # n_vars before the product
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=128, n_vars=20, table=None)   # the product before null
    c(10, "null pointer", flags=None, table_bytes=0, workspace_bytes=0)                # null before the sizes
    c(14, f"table_bytes < batch * 2^n_vars * n_vars * 8 = {tb}", table_bytes=0, workspace_bytes=0)   # table_bytes before workspace_bytes
    c(14, f"workspace_bytes < dvs_arc_posterior_workspace_bytes = {wb}", workspace_bytes=0, family=D,
      family_bytes=0)                                                                  # workspace before family
    return cases


def check_argument_refusals(lib, D):
    run(lib, validation_cases(D))
    assert [split(n) for n in (1, 8, 10, 17, 20)] == [(256, 8, 1), (32, 8, 1), (25, 8, 6), (15, 8, 1093), (12, 43, 2033)]
    for batch, n in ((1, 1), (3, 8), (5, 20), (1, 14), (2, 10)):
        assert lib.dvs_arc_posterior_workspace_bytes(batch, n) == layout(batch, n)[4]
    for (batch, n), text in (((0, 8), "batch must be > 0"), ((1, 0), "n_vars must be in [1, 20]"), ((1, 21), "n_vars must be in [1, 20]"),
                             ((128, 20), "must be < 2^31")):
        assert lib.dvs_arc_posterior_workspace_bytes(batch, n) == 0
        msg = lib.dvs_last_error().decode()
        assert msg.startswith("dvs_arc_posterior_workspace_bytes: ") and text in msg
