"""A multivariate normal conditioned on every row's observed part (include/dvs_gaussian_incomplete.h;
csrc/dvs_gaussian_incomplete.h): the cases, the restatement of the header in Python floats, the exact reference and the checks that
tests/test_emu_gaussian_incomplete.py and tests/test_gpu_gaussian_incomplete.py run unchanged through the C ABI on their own back
end (tests/scoring_corpus.py: EmuBackend, GpuBackend); tests/test_gaussian_incomplete_ref.py holds the restatement itself against
the reference on the CPU.

The joint that is conditioned is the restated one of a seeded network of tests/gaussian_params_corpus.py (restated_joint): its
doubles are the inputs, so the reference takes them as exact.

Reference.  mpmath at 60 digits, sharing no formula with the header: with O the observed and M the missing variables,
  w = S_OO^-1 (x_O - m_O) by an LU solve;  mean_M = m_M + S_MO w;  cov_M = S_MM - S_MO S_OO^-1 S_OM;
  logp = -(k ln(2 pi) + ln det S_OO + (x_O - m_O)^T w) / 2.

Bounds.  None is fitted to a kernel's output.  u = 2^-53, gamma_k = k u / (1 - k u).  The header's loop is k stages of the
outer-product Cholesky factorisation of the matrix with O ordered first.  Higham (Accuracy and Stability, 2nd ed., Theorem 10.3 and
the k-stage form in the proof of Theorem 10.14): the computed R = [R11 R12] and trailing block T satisfy
  S + E = R^T R + [0 0; 0 T],  |E| <= gamma_(k+1) (|R^T| |R| + [0 0; 0 |T|]),
so ||E||_F <= gamma_(k+1) (trace S + ||S_MM||_F) to first order (||R||_F^2 = trace R^T R; T is the Schur complement, below S_MM in
the Loewner order).  The substitution is a forward solve with R11^T (Theorem 8.5): (R11^T + dT) y = d, |dT| <= gamma_k |R11^T|, so y is
the exact solve of S_OO perturbed by E' with ||E'||_F <= ||E||_F + 2 gamma_k trace S_OO =: e1.  d = x_O - m_O is one rounding per
component.  With W = S_OO^-1 S_OM and w as above, both from the reference (this is where kappa(S_OO) enters: ||w||, ||W|| and
||S_OO^-1|| carry it), to first order
  T (cvar, ccov)   |dT_ih| <= ||E||_F (1 + ||W||_F)^2                                   (Higham, Lemma 10.10)
  mean_M           ||d mean||_2 <= (||E||_F + e1 ||W||_F) ||w||_2 + u ||W||_F ||d||_2 + gamma_(k+1) sqrt(trace S_MM q), then one
                   subtraction: u |mean_i|
  q                |dq| <= e1 ||w||_2^2 + 2 u |w|^T |d| + gamma_(k+1) q
  ld               |d ld| <= ||S_OO^-1||_F ||E||_F + LOG_ULPS 2 u sum |ln pivot_j| + gamma_k sum |ln pivot_j|
  logp             (d ld + dq) / 2 + 3 u (|k c| + |ld| / 2 + q / 2) + u k c (the constant's own rounding)
Every first-order bound is doubled for the terms the analysis drops, which is sound while k gamma_(3k) kappa_F < 0.01,
kappa_F = ||S_OO||_F ||S_OO^-1||_F >= kappa_2; pattern_reference asserts that.  ccov adds the product by len and the summation
(gamma_(runs + 16 + ceil(chunks / 256)) on the sum of the magnitudes); loglik adds the summation terms of
gaussian_params_corpus.out_bound.
Between two builds (the emulator or the device against the restatement) only log may differ: completed, cvar, quad and ccov are
compared as bytes; logp is allowed 2 LOG_ULPS ulp on every pivot's log, and the additions behind it round on either side
(build_bound); loglik follows out_bound_between_builds."""
import ctypes
import functools
import math
from types import SimpleNamespace

import mpmath as mp
import numpy as np

from tests import gaussian_corpus as gc
from tests import gaussian_params_corpus as gp

U64 = np.uint64
U = gc.U
NAN = gc.NAN
SENTINEL = gc.SENTINEL
LOG_ULPS = gp.LOG_ULPS
HALF_LOG_2PI = gp.HALF_LOG_2PI
EPS = 2.0 ** -52
N_VALUES = (1, 5, 17, 48)
S_VALUES = (1, 256, 257, 700)
NET_KEYS = {1: ("one", 1), 5: ("dag", 5), 17: ("dag", 17), 48: ("full", 48)}
gamma = gp.gamma


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def joint_of(n):
    """(mean [n], cov [n, n]) float64: the restated joint of the corpus network of n variables"""
    mean, cov = gp.restated_joint(gp.NETS[NET_KEYS[n]])
    assert np.isfinite(cov).all()
    for a in (mean, cov):
        a.setflags(write=False)
    return mean, cov


def masks_for(n, S, kind, seed=0):
    """uint64 [S] masks.  "one": a single seeded pattern; "few": three seeded patterns (with all-observed among them); "unique":
    seeded masks, every row its own where 2^n allows; "mixed": all observed, none observed, one observed, one missing, then seeded"""
    rng = np.random.default_rng(34000 + 131 * n + S + 7 * seed)
    low = (1 << n) - 1
    draw = lambda: int(rng.integers(0, 1 << min(n, 62))) & low if n > 1 else int(rng.integers(0, 2))
    if kind == "one":
        m = draw() | 1
        return np.full(S, m, U64)
    if kind == "few":
        pats = [low, draw(), draw() | (1 << (n - 1))]
        return np.asarray([pats[i] for i in rng.integers(0, 3, S)], U64)
    if kind == "unique":
        seen, out = set(), []
        while len(out) < S:
            m = draw()
            if m not in seen or len(seen) >= (1 << n):
                seen.add(m)
                out.append(m)
        return np.asarray(out, U64)
    if kind == "mixed":
        head = [low, 0, 1 << (n // 2), low & ~(1 << (n // 3))]
        return np.asarray((head + [draw() for _ in range(S)])[:S], U64)
    raise KeyError(kind)


def sorted_order(masks):
    """what torch.sort(observed, stable=True) gives: the stable ascending order of the masks as int32"""
    return np.argsort(np.asarray(masks, U64), kind="stable").astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# The restatement of include/dvs_gaussian_incomplete.h
# ---------------------------------------------------------------------------------------------------------------------
def restated_row(mean, cov, x, mask):
    """one row in Python floats, operation by operation -> (completed [n], cvar [n], q, logp, T [n][n] or None) ; None: refused"""
    n = len(mean)
    mask = int(mask)
    if mask >> n:
        return None
    O = [v for v in range(n) if (mask >> v) & 1]
    k = len(O)
    if any(not math.isfinite(float(x[v])) for v in O):
        return None
    A = [[float(cov[max(i, j)][min(i, j)]) for j in range(n)] for i in range(n)]         # the lower triangle, mirrored
    t = [float(x[v]) - float(mean[v]) if (mask >> v) & 1 else 0.0 for v in range(n)]
    ld, q = 0.0, 0.0
    rem = list(range(n))
    for j in O:
        ajj = A[j][j]
        if not math.isfinite(ajj) or ajj <= ((k + 1) * EPS) * float(cov[j][j]):
            return None
        d = math.sqrt(ajj)
        ld = ld + math.log(ajj)
        y = t[j] / d
        q = q + y * y
        rem.remove(j)
        l = {}
        for i in rem:
            l[i] = A[i][j] / d
            t[i] = t[i] - l[i] * y
        for i in rem:
            for h in rem:
                if h <= i:
                    A[i][h] = A[i][h] - l[i] * l[h]
                    A[h][i] = A[i][h]
    completed = [float(x[v]) if (mask >> v) & 1 else float(mean[v]) - t[v] for v in range(n)]
    cvar = [0.0 if (mask >> v) & 1 else A[v][v] for v in range(n)]
    logp = -((k * HALF_LOG_2PI + 0.5 * ld) + 0.5 * q)
    T = [[A[i][h] if not (mask >> i) & 1 and not (mask >> h) & 1 else 0.0 for h in range(n)] for i in range(n)]
    return completed, cvar, q, logp, T


def restated_factor(cov, mask):
    """the factor of one pattern, vectorised over the cells (numpy's elementwise float64 operations round as Python's do, one at
    a time) -> None (refused) or (O, k, ld, logs, d {j: d_j}, l {j: l [n]}, A final [n, n] symmetric)"""
    n = len(cov)
    mask = int(mask)
    if mask >> n:
        return None
    O = [v for v in range(n) if (mask >> v) & 1]
    k = len(O)
    A = np.tril(cov) + np.tril(cov, -1).T
    ld, logs, ds, ls = 0.0, [], {}, {}
    rem = np.ones(n, bool)
    for j in O:
        ajj = float(A[j, j])
        if not math.isfinite(ajj) or ajj <= ((k + 1) * EPS) * float(cov[j, j]):
            return None
        d = math.sqrt(ajj)
        lg = math.log(ajj)
        ld = ld + lg
        logs.append(lg)
        rem[j] = False
        l = np.where(rem, A[:, j] / d, 0.0)
        idx = np.flatnonzero(rem)
        A[np.ix_(idx, idx)] = A[np.ix_(idx, idx)] - np.outer(l[idx], l[idx])
        ds[j], ls[j] = d, l
    return O, k, ld, logs, ds, ls, A


def two_level(parts):
    """the chunk values [chunks, ...] added as dvs_bn_loglik adds chunk sums: slot t of 256 adds the chunks t, t + 256, ... in
    ascending order, then the tree (for s = 128 .. 1: slot t < s adds slot t + s)"""
    parts = np.asarray(parts, np.float64)
    second = np.zeros((256,) + parts.shape[1:])
    for c in range(len(parts)):
        second[c % 256] = second[c % 256] + parts[c]
    s = 128
    while s:
        second[:s] = second[:s] + second[s:2 * s]
        s >>= 1
    return second[0]


def restated_condition(mean, cov, x, masks, order=None):
    """every output of dvs_gbn_condition -> SimpleNamespace(completed, cvar, quad, logp [S...], loglik, ccov [n, n], counts,
    status, logs: {row: the pivots' logs}, refused [S] bool)"""
    mean, cov, x = np.asarray(mean, np.float64), np.asarray(cov, np.float64), np.asarray(x, np.float64)
    masks = [int(m) for m in np.asarray(masks, U64)]
    S, n = x.shape
    order = np.arange(S) if order is None else np.asarray(order)
    completed, cvar, quad, logp = np.full((S, n), NAN), np.full((S, n), NAN), np.full(S, NAN), np.full(S, NAN)
    refused = np.ones(S, bool)
    factors, ks, lds = {}, np.zeros(S, int), np.zeros(S)
    by_mask = {}
    for r, m in enumerate(masks):
        by_mask.setdefault(m, []).append(r)
    for m, rows in by_mask.items():
        f = factors[m] = restated_factor(cov, m)
        if f is None:
            continue
        O, k, ld, logs, ds, ls, A = f
        rows = np.asarray(rows)
        obs = np.asarray([(m >> v) & 1 for v in range(n)], bool)
        good = np.isfinite(x[np.ix_(rows, np.flatnonzero(obs))]).all(axis=1) if k else np.ones(len(rows), bool)
        rows = rows[good]
        if not len(rows):
            continue
        t = np.where(obs, np.where(obs, x[rows], 0.0) - mean, 0.0)
        q = np.zeros(len(rows))
        for j in O:
            y = t[:, j] / ds[j]
            q = q + y * y
            t = t - np.where(_rem_after(O, j, n), ls[j] * y[:, None], 0.0)
        completed[rows] = np.where(obs, x[rows], mean - t)
        cvar[rows] = np.where(obs, 0.0, np.diag(A))
        quad[rows] = q
        logp[rows] = -((k * HALF_LOG_2PI + 0.5 * ld) + 0.5 * q)
        refused[rows] = False
        ks[rows], lds[rows] = k, ld
    terms = np.where(refused, 0.0, logp)[order]
    loglik = gp.stated_sum(terms)
    chunks = -(-S // 256)
    parts = np.zeros((chunks, n, n))
    for c in range(chunks):
        pos = order[c * 256:(c + 1) * 256]
        a = 0
        while a < len(pos):
            b = a + 1
            while b < len(pos) and masks[pos[b]] == masks[pos[a]]:
                b += 1
            cnt = int((~refused[pos[a:b]]).sum())
            if cnt:
                m = masks[pos[a]]
                mis = np.asarray([not (m >> v) & 1 for v in range(n)], bool)
                T = np.where(np.outer(mis, mis), factors[m][6], 0.0)
                parts[c] = parts[c] + np.where(np.outer(mis, mis), float(cnt) * T, 0.0)
            a = b
    return SimpleNamespace(completed=completed, cvar=cvar, quad=quad, logp=logp, loglik=float(loglik), ccov=two_level(parts),
                           counts=int(refused.sum()), status=16 if refused.any() else 0, refused=refused, factors=factors, k=ks, ld=lds)


def _rem_after(O, j, n):
    """bool [n]: the variables not yet pivoted once j is (the later members of O and all of M)"""
    done = set(O[:O.index(j) + 1])
    return np.asarray([v not in done for v in range(n)], bool)


def build_bound(res):
    """[S]: what another build's logp may differ by from the restated one: 2 LOG_ULPS ulp on each pivot's log and one rounding
    of each addition behind it on either side (the k additions of ld, the two of logp)"""
    out = np.zeros(len(res.logp))
    for r in range(len(out)):
        if res.refused[r]:
            continue
        f = res.factors[_mask_of_row(res, r)]
        logs = f[3]
        dld, run = 0.0, 0.0
        for lg in logs:
            dld += 2 * LOG_ULPS * 2 * U * abs(lg)
            run += abs(lg) + dld
            dld += 2 * U * run
        k = f[1]
        norm = abs(k * HALF_LOG_2PI) + 0.5 * abs(f[2])
        out[r] = (0.5 * dld + 2 * U * (norm + 0.5 * dld) + 2 * U * (abs(float(res.logp[r])) + dld)) * (1 + 1e-9)
    return out


def _mask_of_row(res, r):
    return res.row_masks[r]


# ---------------------------------------------------------------------------------------------------------------------
# The reference and its bounds
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
@gc.at60
def pattern_reference(n, mask):
    """what a pattern fixes, in mpmath from the restated joint's doubles: SimpleNamespace(O, M, Sinv (S_OO^-1), W (S_OO^-1 S_OM),
    T (the conditional covariance), logdet, sum of |ln pivot|, and the norms the bounds take)"""
    mean, cov = joint_of(n)
    O = [v for v in range(n) if (mask >> v) & 1]
    M = [v for v in range(n) if not (mask >> v) & 1]
    k = len(O)
    S = lambda a, b: mp.matrix([[mp.mpf(float(cov[max(i, j), min(i, j)])) for j in b] for i in a]) if a and b else mp.matrix(len(a), len(b))
    ref = SimpleNamespace(O=O, M=M, k=k)
    Soo, Som, Smm = S(O, O), S(O, M), S(M, M)
    if k:
        ref.Sinv = Soo ** -1
        L = mp.cholesky(Soo)
        piv = [L[i, i] ** 2 for i in range(k)]
        ref.logdet = mp.fsum(mp.log(p) for p in piv)
        ref.logs = float(mp.fsum(abs(mp.log(p)) for p in piv))
        ref.W = ref.Sinv * Som if M else mp.matrix(k, 0)
        ref.T = Smm - Som.T * ref.W if M else mp.matrix(0, 0)
        fro = lambda A: float(mp.sqrt(mp.fsum(A[i, j] ** 2 for i in range(A.rows) for j in range(A.cols)))) if A.rows and A.cols else 0.0
        ref.Sinv_F, ref.W_F, ref.Soo_F = fro(ref.Sinv), fro(ref.W), fro(Soo)
    else:
        ref.Sinv, ref.logdet, ref.logs, ref.W, ref.T = None, mp.mpf(0), 0.0, None, Smm
        ref.Sinv_F = ref.W_F = ref.Soo_F = 0.0
    tr = float(mp.fsum(mp.mpf(float(cov[v, v])) for v in range(n)))
    ref.tr_O = float(mp.fsum(mp.mpf(float(cov[v, v])) for v in O)) if O else 0.0
    ref.tr_M = tr - ref.tr_O
    Smm_F = float(mp.sqrt(mp.fsum(Smm[i, j] ** 2 for i in range(len(M)) for j in range(len(M))))) if M else 0.0
    ref.E_F = gamma(k + 1) * (tr + Smm_F)
    ref.e1 = ref.E_F + 2 * gamma(max(k, 1)) * ref.tr_O
    ref.kappa_F = ref.Soo_F * ref.Sinv_F
    assert k * gamma(3 * max(k, 1)) * ref.kappa_F < 0.01, ("the first-order analysis needs a milder pattern", n, mask, ref.kappa_F)
    ref.T_bound = 2 * ref.E_F * (1 + ref.W_F) ** 2 * (1 + 1e-9) if k else 0.0
    return ref


@gc.at60
def row_reference(n, mask, x):
    """(mean of every missing variable {v: mpf}, logp mpf, q mpf, bounds SimpleNamespace(mean, q, logp)) of one row"""
    mean, cov = joint_of(n)
    ref = pattern_reference(n, int(mask))
    O, M, k = ref.O, ref.M, ref.k
    if not k:
        return {v: mp.mpf(float(mean[v])) for v in M}, mp.mpf(0), mp.mpf(0), SimpleNamespace(mean=0.0, q=0.0, logp=0.0)
    d = mp.matrix([mp.mpf(float(x[v])) - mp.mpf(float(mean[v])) for v in O])
    w = ref.Sinv * d
    q = (d.T * w)[0]
    cm = {}
    for a, v in enumerate(M):
        cm[v] = mp.mpf(float(mean[v])) + mp.fsum(mp.mpf(float(cov[max(v, o), min(v, o)])) * w[i] for i, o in enumerate(O))
    logp = -(k * mp.log(2 * mp.pi) + ref.logdet + q) / 2
    w2, d2 = float(mp.norm(w, 2)), float(mp.norm(d, 2))
    wd = float(mp.fsum(abs(w[i]) * abs(d[i]) for i in range(k)))
    qf = float(q)
    bq = 2 * (ref.e1 * w2 * w2 + 2 * U * wd + gamma(k + 1) * qf)
    bm = 2 * ((ref.E_F + ref.e1 * ref.W_F) * w2 + U * ref.W_F * d2 + gamma(k + 1) * math.sqrt(max(ref.tr_M, 0.0) * qf))
    bld = 2 * ref.Sinv_F * ref.E_F + (LOG_ULPS * 2 * U + gamma(k)) * ref.logs
    kc = k * HALF_LOG_2PI
    bl = 0.5 * (bld + bq) + 3 * U * (kc + 0.5 * float(abs(ref.logdet)) + 0.5 * qf) + U * kc
    s = 1 + 1e-9
    return cm, logp, q, SimpleNamespace(mean=bm * s, q=bq * s, logp=bl * s)


def assert_rows_against_reference(n, x, masks, res, rows):
    """the restated (or a build's) per-row outputs against mpmath under the derived bounds on ``rows`` -> worst error / bound"""
    mean, _ = joint_of(n)
    worst = 0.0
    for r in rows:
        m = int(masks[r])
        assert not res.refused[r], (n, r, m)
        ref = pattern_reference(n, m)
        cm, logp, q, b = row_reference(n, m, x[r])
        for v in ref.O:
            assert np.float64(res.completed[r, v]).tobytes() == np.float64(x[r, v]).tobytes() and res.cvar[r, v] == 0.0
        for a, v in enumerate(ref.M):
            err = float(abs(mp.mpf(float(res.completed[r, v])) - cm[v]))
            bound = b.mean + U * float(abs(cm[v]))
            assert err <= bound, (n, r, m, v, "mean", err, bound)
            verr = float(abs(mp.mpf(float(res.cvar[r, v])) - ref.T[a, a]))
            assert verr <= ref.T_bound, (n, r, m, v, "var", verr, ref.T_bound)
            worst = max(worst, err / bound if bound else 0.0, verr / ref.T_bound if ref.T_bound else 0.0)
        for name, have, want, bound in (("q", res.quad[r], q, b.q), ("logp", res.logp[r], logp, b.logp)):
            err = float(abs(mp.mpf(float(have)) - want))
            assert err <= bound, (n, r, m, name, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
    return worst


@gc.at60
def assert_sums_against_reference(n, x, masks, res, order=None):
    """loglik and ccov against the reference's sums under the rows' bounds plus the summation's"""
    S = len(x)
    order = np.arange(S) if order is None else order
    chunks = -(-S // 256)
    terms, bounds = [], []
    acc = [[mp.mpf(0)] * n for _ in range(n)]
    mag, tb = np.zeros((n, n)), np.zeros((n, n))
    runs = 0
    prev = None
    for p, r in enumerate(order):
        m = int(masks[r])
        runs += 1 if (m != prev or p % 256 == 0) else 0
        prev = m
        ref = pattern_reference(n, m)
        _, logp, _, b = row_reference(n, m, x[r])
        terms.append(logp)
        bounds.append(b.logp)
        for a, v in enumerate(ref.M):
            for c, u in enumerate(ref.M):
                acc[v][u] += ref.T[a, c]
                mag[v, u] += float(abs(ref.T[a, c]))
                tb[v, u] += ref.T_bound
    ob = gp.out_bound([float(abs(t)) for t in terms], bounds, S)
    err = float(abs(mp.mpf(res.loglik) - mp.fsum(terms)))
    assert err <= ob, ("loglik", err, ob)
    g = gamma(runs + 17 + -(-chunks // 256))
    for v in range(n):
        for u in range(n):
            err = float(abs(mp.mpf(float(res.ccov[v, u])) - acc[v][u]))
            bound = (tb[v, u] + g * (mag[v, u] + tb[v, u])) * (1 + 1e-9)
            assert err <= bound, ("ccov", v, u, err, bound)


def blanket_mask(net, t):
    """the Markov blanket of t (parents, children, the children's other parents) as a mask"""
    n = net.n
    kids = [c for c in range(n) if c != t and t in net.pa(c)]
    members = set(net.pa(t)) | set(kids) | {u for c in kids for u in net.pa(c)}
    members.discard(t)
    return gc.mask_of(sorted(members))


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI on a back end
# ---------------------------------------------------------------------------------------------------------------------
def workspace_bytes(n, S):
    up = lambda v: (v + 255) & ~255
    chunks = -(-S // 256)
    return up(chunks * 8) + up(chunks * 4) + n * (n + 1) // 2 * chunks * 8


ALL_OUTPUTS = ("completed", "cvar", "quad", "ccov", "counts")


def run_condition(be, mean, cov, x, masks, order=None, outputs=ALL_OUTPUTS):
    """dvs_gbn_condition -> SimpleNamespace of host copies (an output left out of ``outputs`` is passed null and is None here);
    a row of sentinels before and after every per-row output must survive"""
    x = np.ascontiguousarray(x, np.float64)
    S, n = x.shape
    need = int(be.lib.dvs_gbn_condition_workspace_bytes(n, S))
    assert need == workspace_bytes(n, S), (need, workspace_bytes(n, S))
    at = lambda h, b: ctypes.c_void_p(be.ptr(h).value + b)
    rows2 = lambda: be.put(np.full((S + 2, n), SENTINEL))
    rows1 = lambda: be.put(np.full(S + 2, SENTINEL))
    hc = rows2() if "completed" in outputs else None
    hv = rows2() if "cvar" in outputs else None
    hq = rows1() if "quad" in outputs else None
    hl, hs = rows1(), be.put(np.full(3, SENTINEL))
    hcc = be.put(np.full((n + 2, n), SENTINEL)) if "ccov" in outputs else None
    hcnt = be.put(np.full(3, -7, np.int64)) if "counts" in outputs else None
    status = be.put(np.zeros(1, np.int32))
    ws = be.put(np.zeros(need, np.uint8))
    gc.call(be, "dvs_gbn_condition", n_vars=n, n_rows=S, mean=be.put(np.ascontiguousarray(mean, np.float64)),
            cov=be.put(np.ascontiguousarray(cov, np.float64)), x=be.put(x), observed=be.put(np.ascontiguousarray(masks, U64)),
            order=None if order is None else be.put(np.ascontiguousarray(order, np.int32)),
            completed=None if hc is None else at(hc, n * 8), cvar=None if hv is None else at(hv, n * 8),
            quad=None if hq is None else at(hq, 8), logp=at(hl, 8), loglik=at(hs, 8), ccov=None if hcc is None else at(hcc, n * 8),
            counts=None if hcnt is None else at(hcnt, 8), workspace=ws, workspace_bytes=need, status=status)

    def guarded(h, sentinel=SENTINEL):
        if h is None:
            return None
        a = np.array(be.get(h), copy=True)
        assert (a[0] == sentinel).all() and (a[-1] == sentinel).all()
        return a[1:-1]
    cnt = guarded(hcnt, -7)
    return SimpleNamespace(completed=guarded(hc), cvar=guarded(hv), quad=guarded(hq), logp=guarded(hl), loglik=float(guarded(hs)[0]),
                           ccov=guarded(hcc), counts=None if cnt is None else int(cnt[0]), status=int(be.get(status)[0]))


def restated(n, x, masks, order=None, cov=None):
    mean, joint_cov = joint_of(n)
    res = restated_condition(mean, joint_cov if cov is None else cov, x, masks, order)
    res.row_masks = [int(m) for m in np.asarray(masks, U64)]
    return res


def same(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def assert_equals_restatement(got, res, order, what, outputs=ALL_OUTPUTS):
    """a build against the restatement: completed, cvar, quad, ccov and counts as bytes, logp and loglik under build_bound"""
    for name in ("completed", "cvar", "quad", "ccov"):
        if name in outputs:
            have, want = getattr(got, name), getattr(res, name)
            assert same(have, want), (what, name, np.argwhere(~((have == want) | (np.isnan(have) & np.isnan(want))))[:4])
    if "counts" in outputs:
        assert got.counts == res.counts, (what, got.counts, res.counts)
    assert got.status == res.status, (what, got.status, res.status)
    assert (np.isnan(got.logp) == res.refused).all(), what
    bounds = build_bound(res)
    err = np.where(res.refused, 0.0, np.abs(got.logp - res.logp))
    assert (err <= bounds).all(), (what, "logp", int(np.argmax(err - bounds)), float(err.max()))
    S = len(res.logp)
    order = np.arange(S) if order is None else order
    terms = np.where(res.refused, 0.0, res.logp)[order]
    ob = gp.out_bound_between_builds(terms, bounds)
    assert abs(got.loglik - res.loglik) <= ob, (what, "loglik", got.loglik, res.loglik, ob)
    # the build's own loglik is the stated tree over its own logp, as bytes
    own = gp.stated_sum(np.where(np.isnan(got.logp), 0.0, got.logp)[order])
    assert np.float64(own).tobytes() == np.float64(got.loglik).tobytes(), (what, own, got.loglik)
    nz = bounds[~res.refused & (bounds > 0)]
    return float(np.max(err[~res.refused & (bounds > 0)] / nz)) if len(nz) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# Checks on a back end
# ---------------------------------------------------------------------------------------------------------------------
def shape_cases():
    """(n, S, kind): every n at every S with one pattern and with a few; the mixed head once per n"""
    cases = [(n, S, kind) for n in N_VALUES for S in S_VALUES for kind in ("one", "few")]
    return cases + [(n, 257, "mixed") for n in N_VALUES]


def check_condition(be, n, S, kind):
    """sorted order, every output: the build equals the restatement; two calls give equal bytes -> worst logp error / bound"""
    mean, cov = joint_of(n)
    x, masks = gp.rows_for(n, S), masks_for(n, S, kind)
    order = sorted_order(masks)
    res = restated(n, x, masks, order)
    got = run_condition(be, mean, cov, x, masks, order)
    again = run_condition(be, mean, cov, x, masks, order)
    for name in ("completed", "cvar", "quad", "logp", "ccov"):
        assert same(getattr(got, name), getattr(again, name)), name
    assert got.loglik == again.loglik and got.counts == again.counts == 0
    return assert_equals_restatement(got, res, order, (n, S, kind))


def check_unique_patterns(be, n=17, S=300):
    """every row its own pattern: 256 factorisations in the first chunk"""
    masks = masks_for(n, S, "unique")
    assert len(set(int(m) for m in masks)) == S
    mean, cov = joint_of(n)
    x, order = gp.rows_for(n, S), sorted_order(masks)
    return assert_equals_restatement(run_condition(be, mean, cov, x, masks, order), restated(n, x, masks, order), order, "unique")


def straddle_masks(n=5, S=300):
    """already sorted: one mask at positions 250 .. 262, across the chunk boundary at 256"""
    masks = np.zeros(S, U64)
    masks[:250], masks[250:263], masks[263:] = 0b00101, 0b01001, 0b11010
    return masks


def check_straddle(be):
    """a run across a chunk boundary is two runs in ccov, as the header says: the restatement does that and the build equals it"""
    n, S = 5, 300
    masks = straddle_masks(n, S)
    assert (np.diff(masks.astype(np.int64)) >= 0).all()
    mean, cov = joint_of(n)
    x = gp.rows_for(n, S)
    res = restated(n, x, masks)
    got = run_condition(be, mean, cov, x, masks)
    assert_equals_restatement(got, res, None, "straddle")
    T = res.factors[0b01001][6]
    assert res.ccov[1, 1] != 0.0 and T[1, 1] > 0.0


def check_second_level(be):
    """S = 65 537 at n = 5 with three patterns: 257 chunks, so slot 0 of the second array adds chunks 0 and 256"""
    n, S = 5, 65537
    masks = masks_for(n, S, "few")
    assert len(set(int(m) for m in masks)) == 3
    mean, cov = joint_of(n)
    x, order = gp.rows_for(n, S), sorted_order(masks)
    return assert_equals_restatement(run_condition(be, mean, cov, x, masks, order), restated(n, x, masks, order), order, "second level")


def check_orders(be, n=17, S=700):
    """per-row outputs are equal as bytes under order = null, sorted and a seeded permutation; ccov and loglik equal the
    restatement run with that same order"""
    masks = masks_for(n, S, "few")
    mean, cov = joint_of(n)
    x = gp.rows_for(n, S)
    orders = (None, sorted_order(masks), np.random.default_rng(3407).permutation(S).astype(np.int32))
    runs = [run_condition(be, mean, cov, x, masks, o) for o in orders]
    for got, o in zip(runs, orders):
        assert_equals_restatement(got, restated(n, x, masks, o), o, ("order", None if o is None else int(o[0])))
        for name in ("completed", "cvar", "quad", "logp"):
            assert same(getattr(got, name), getattr(runs[0], name)), name


def check_null_outputs(be, n=17, S=300):
    """cvar and ccov null (the M x M updates may be skipped), then every nullable output null: the rest keeps its bytes"""
    masks = masks_for(n, S, "few")
    mean, cov = joint_of(n)
    x, order = gp.rows_for(n, S), sorted_order(masks)
    full = run_condition(be, mean, cov, x, masks, order)
    part = run_condition(be, mean, cov, x, masks, order, outputs=("completed", "quad", "counts"))
    bare = run_condition(be, mean, cov, x, masks, order, outputs=())
    assert part.cvar is None and part.ccov is None and bare.completed is None
    assert same(part.completed, full.completed) and same(part.quad, full.quad) and part.counts == full.counts
    for got in (part, bare):
        assert same(got.logp, full.logp) and got.loglik == full.loglik and got.status == full.status


def duplicated_cov(n, i, j):
    """the joint's covariance with variable j made a copy of variable i: every observed set holding both is singular"""
    cov = np.array(joint_of(n)[1], copy=True)
    cov[j, :], cov[:, j] = cov[i, :], cov[:, i]
    cov[j, j] = cov[i, i]
    return cov


def check_refusals(be, n=5, S=300):
    """each refusal rule alone on three rows between rows that keep their bytes; counts and bit 4"""
    mean, cov = joint_of(n)
    x0 = np.array(gp.rows_for(n, S), copy=True)
    masks0 = masks_for(n, S, "few")
    low = (1 << n) - 1
    hit = (7, 130, 299)
    base = run_condition(be, mean, cov, x0, masks0, sorted_order(masks0))
    assert base.status == 0 and base.counts == 0
    keep = np.ones(S, bool)
    keep[list(hit)] = False

    def one(x, masks, cov_=cov, refuse=True):
        order = sorted_order(masks)
        res = restated(n, x, masks, order, cov=cov_)
        assert list(np.flatnonzero(res.refused)) == (list(hit) if refuse else []), np.flatnonzero(res.refused)
        got = run_condition(be, mean, cov_, x, masks, order)
        assert_equals_restatement(got, res, order, "refusal")
        if refuse:
            assert got.status == 16 and got.counts == 3
            for name in ("completed", "cvar"):
                assert np.isnan(getattr(got, name)[list(hit)]).all() and not np.isnan(getattr(got, name)[keep]).any()
            assert np.isnan(got.quad[list(hit)]).all() and np.isnan(got.logp[list(hit)]).all()
        return got

    # a mask bit at n
    masks = masks0.copy()
    masks[list(hit)] |= U64(1 << n)
    got = one(x0, masks)
    for name in ("completed", "cvar", "quad", "logp"):
        assert same(getattr(got, name)[keep], getattr(base, name)[keep]), name
    # an observed NaN, an observed infinity
    for bad in (NAN, math.inf):
        x = x0.copy()
        masks = masks0.copy()
        for r in hit:
            masks[r] = low
            x[r, r % n] = bad
        got = one(x, masks)
        for name in ("completed", "cvar", "quad", "logp"):
            assert same(getattr(got, name)[keep], getattr(base, name)[keep]), name
    # an unobserved NaN is harmless: the bytes of the run without it
    x, masks = x0.copy(), masks0.copy()
    for r in hit:
        masks[r] = low & ~(1 << (r % n))
        x[r, r % n] = NAN
    clean = x.copy()
    clean[np.isnan(clean)] = 0.25
    got, ref = one(x, masks, refuse=False), run_condition(be, mean, cov, clean, masks, sorted_order(masks))
    for name in ("cvar", "quad", "logp", "ccov"):
        assert same(getattr(got, name), getattr(ref, name)), name
    assert same(got.completed, ref.completed) and got.loglik == ref.loglik and got.counts == 0 and got.status == 0
    # a duplicated column: the rows that observe both copies are refused, the rows that observe one are not
    dup = duplicated_cov(n, 1, 3)
    masks = np.where((masks0 & U64(0b01010)) == U64(0b01010), masks0 & ~U64(0b01000), masks0)
    masks[list(hit)] = low
    got = one(x0, masks, cov_=dup)
    assert not np.isnan(got.logp[keep]).any()


def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do), in the documented order"""
    need = workspace_bytes(5, 300)

    def cond(**kw):
        a = dict(n=5, rows=300, mean=ptr, cov=ptr, x=ptr, obs=ptr, order=ptr, completed=ptr, cvar=ptr, quad=ptr, logp=ptr, loglik=ptr,
                 ccov=ptr, counts=ptr, ws=ptr, wb=need, status=ptr)
        a.update(kw)
        return lib.dvs_gbn_condition(a["n"], a["rows"], a["mean"], a["cov"], a["x"], a["obs"], a["order"], a["completed"], a["cvar"],
                                     a["quad"], a["logp"], a["loglik"], a["ccov"], a["counts"], a["ws"], a["wb"], a["status"], None)
    assert cond(rows=0) == 2 and cond(rows=1 << 31) == 2 and cond(n=0) == 3 and cond(n=49) == 3 and cond(rows=0, n=0) == 2
    assert all(cond(**{k: None}) == 10 for k in ("mean", "cov", "x", "obs", "logp", "loglik", "ws", "status"))
    assert cond(n=0, mean=None) == 3 and cond(mean=None, wb=0) == 10
    assert cond(wb=need - 1) == 14 and str(need).encode() in lib.dvs_last_error()
    # the nullable arguments: a null one passes the checks (the size check behind them is reached)
    assert cond(order=None, completed=None, cvar=None, quad=None, ccov=None, counts=None, wb=need - 1) == 14
    assert lib.dvs_gbn_condition_workspace_bytes(0, 10) == 0 and lib.dvs_gbn_condition_workspace_bytes(49, 10) == 0
    assert lib.dvs_gbn_condition_workspace_bytes(5, 0) == 0 and lib.dvs_gbn_condition_workspace_bytes(5, 1 << 31) == 0
    assert lib.dvs_gbn_condition_workspace_bytes(5, 300) == need and lib.dvs_gbn_condition_workspace_bytes(48, 1) == 256 + 256 + 1176 * 8


# ---------------------------------------------------------------------------------------------------------------------
# EM on the restatement: one step, the closed form, the settings the GPU tests use (chosen here, on the CPU)
# ---------------------------------------------------------------------------------------------------------------------
EM_ROWS, EM_SEED, EM_MASK_SEED, EM_STEPS = 2048, 512, 3412, 4
# x0 -> x1 with x1 missing in a seeded third of the rows.  The pattern is monotone, so EM's linear rate on the regression of x1
# is the missing fraction, 1/3: CLOSED_ITERATIONS = 40 steps leave (1/3)^40 < 1e-19 of the start's error, and what remains is
# rounding: the moments of 2048 rows carry gamma_2050 = 2.3e-13 relative to sum |d_i d_j|, which the fit amplifies by the
# condition of the two-variable cross-products (below 20 here, asserted on the CPU), so CLOSED_RTOL = 1e-10 leaves a factor of
# about 40.  tests/test_gaussian_incomplete_ref.py runs the restatement to these settings and holds it inside the tolerance.
CLOSED_ITERATIONS, CLOSED_RTOL, CLOSED_ROWS, CLOSED_SEED = 40, 1e-10, 2048, 3434
CLOSED_NET = gp.NETS[("pair", 2)]


def em_masks(S, n, fraction, seed):
    """uint64 [S]: every cell missing with probability ``fraction``, seeded"""
    rng = np.random.default_rng(seed)
    seen = rng.random((S, n)) >= fraction
    return (seen.astype(U64) << np.arange(n, dtype=U64)).sum(1, dtype=U64)


def net_copy(net, coef, intercept, sd):
    return gp.Net(n=net.n, parents=list(net.parents), coef=np.array(coef, np.float64), intercept=np.array(intercept, np.float64),
                  sd=np.array(sd, np.float64))


def start_net(parents, x, masks):
    """gaussian_em_fit's default start, in numpy: not compared as bytes (torch's reductions have their own order)"""
    n = len(parents)
    seen = ((np.asarray(masks, U64)[:, None] >> np.arange(n, dtype=U64)) & U64(1)).astype(bool)
    cnt = np.maximum(seen.sum(0), 1)
    mean = np.where(seen, x, 0.0).sum(0) / cnt
    sd = np.sqrt(np.where(seen, (x - mean) ** 2, 0.0).sum(0) / cnt)
    return gp.Net(n=n, parents=list(parents), coef=np.zeros((n, n)), intercept=mean, sd=sd)


def restated_em_step(net, x, masks, variance="mle"):
    """one iteration as gaussian_em_fit composes it: the restated joint, the restated conditioning in sorted order, the restated
    moments of the completed rows plus the summed conditional covariance (one elementwise add), the restated fit, the M-step's
    rescaling -> (the next network, the log-likelihood under ``net``, the conditioning's result)"""
    n, m = net.n, float(len(x))
    mean, cov = gp.restated_joint(net)
    res = restated_condition(mean, cov, x, masks, sorted_order(masks))
    res.row_masks = [int(v) for v in np.asarray(masks, U64)]
    assert not res.refused.any()
    mom = gc.restated_moments(np.ascontiguousarray(res.completed))[0]
    mom[1 + n:] = mom[1 + n:] + res.ccov.ravel()
    coef, icpt, sd = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    for v in range(n):
        coef[v], icpt[v], sd[v] = gc.restated_fit(mom, n, v, net.parents[v])
        if variance == "mle":
            sd[v] = sd[v] * math.sqrt(max(m - len(net.pa(v)) - 1.0, 0.0) / m)
    return net_copy(net, coef, icpt, sd), res.loglik, res


def closed_form_case():
    """(x [S, 2], masks [S]) of the two-variable case: rows drawn from CLOSED_NET by numpy, x1 missing in a seeded third"""
    rng = np.random.default_rng(CLOSED_SEED)
    x0 = CLOSED_NET.intercept[0] + CLOSED_NET.sd[0] * rng.normal(size=CLOSED_ROWS)
    x1 = CLOSED_NET.intercept[1] + CLOSED_NET.coef[1, 0] * x0 + CLOSED_NET.sd[1] * rng.normal(size=CLOSED_ROWS)
    masks = np.where(rng.random(CLOSED_ROWS) < 1.0 / 3.0, U64(1), U64(3)).astype(U64)
    return np.ascontiguousarray(np.stack([x0, x1], axis=1)), masks


def closed_form(x, masks):
    """the ML estimate under x0 -> x1 with x1 missing at random given x0: the mean and variance (/ m) of x0 from all rows, the
    regression of x1 on x0 from the complete rows with RSS / m_c -> (intercept [2], slope, sd [2]); plain numpy: the reference of
    a tolerance far above its own rounding"""
    full = np.asarray(masks, U64) == U64(3)
    a = x[:, 0]
    mu0, sd0 = a.mean(), math.sqrt(((a - a.mean()) ** 2).mean())
    xc = x[full]
    ac, bc = xc[:, 0] - xc[:, 0].mean(), xc[:, 1] - xc[:, 1].mean()
    slope = float(ac @ bc) / float(ac @ ac)
    icpt = xc[:, 1].mean() - slope * xc[:, 0].mean()
    res = xc[:, 1] - icpt - slope * xc[:, 0]
    return np.asarray([mu0, icpt]), slope, np.asarray([sd0, math.sqrt(float(res @ res) / len(xc))])


def assert_meets_closed_form(coef, intercept, sd, x, masks, what):
    icpt, slope, sds = closed_form(x, masks)
    scale = max(abs(icpt).max(), abs(slope), sds.max())
    err = max(abs(np.asarray(intercept) - icpt).max(), abs(float(coef[1][0]) - slope), abs(np.asarray(sd) - sds).max())
    assert err <= CLOSED_RTOL * scale, (what, err, CLOSED_RTOL * scale)
    return err / (CLOSED_RTOL * scale)


# ---------------------------------------------------------------------------------------------------------------------
# Closing the loop with missing cells, on the CPU first: the setting below is the one at which the restatement alone recovers
# the generator's equivalence class (tests/test_gaussian_incomplete_ref.py holds that, with its gap)
# ---------------------------------------------------------------------------------------------------------------------
MISSING_LOOP_MASK_SEED, MISSING_LOOP_STEPS = 3410, 12
MISSING_LOOP_DAG = [0, 1, 3, 7, 15]          # the complete DAG in index order: EM under it estimates an unrestricted covariance


def missing_loop_case():
    """(x [2000, 5], masks): the restated rows of gaussian_params_corpus.LOOP_NET with a seeded 10 % of the cells missing"""
    x = gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[0]
    return x, em_masks(gp.LOOP_ROWS, 5, 0.1, MISSING_LOOP_MASK_SEED)


@functools.lru_cache(maxsize=None)
def missing_loop_reference():
    """MISSING_LOOP_STEPS restated EM steps under the complete DAG, the restated expected moments under the result, the restated
    bge scores of all 80 families on them, the best equivalence class over all 29 281 DAGs and its gap to the best other class"""
    n = 5
    x, masks = missing_loop_case()
    net = start_net(MISSING_LOOP_DAG, x, masks)
    for _ in range(MISSING_LOOP_STEPS):
        net, _, _ = restated_em_step(net, x, masks, "mle")
    mean, cov = gp.restated_joint(net)
    res = restated_condition(mean, cov, x, masks, sorted_order(masks))
    mom = gc.restated_moments(np.ascontiguousarray(res.completed))[0]
    mom[1 + n:] = mom[1 + n:] + res.ccov.ravel()
    table = np.full((n, 1 << n), NAN)
    for v in range(n):
        for pm in range(1 << n):
            if not (pm >> v) & 1:
                table[v, pm] = gc.restated_local(mom, n, v, pm, "bge")
    dags = gc.all_dags(n)
    scores = sum(table[v, dags[:, v]] for v in range(n))
    best = int(np.argmax(scores))
    best_key = gc.cpdag_key([int(m) for m in dags[best]])
    others = [float(s) for d, s in zip(dags, scores) if s > scores[best] - 50.0 and gc.cpdag_key([int(m) for m in d]) != best_key]
    return SimpleNamespace(best_key=best_key, truth=gc.cpdag_key(gp.LOOP_NET.parents), gap=float(scores[best]) - max(others),
                           missing=1 - float(np.mean([bin(int(m)).count("1") for m in masks])) / n)
