"""A fitted conditional Gaussian network (include/dvs_mixed_params.h; csrc/dvs_mixed_params.h): the cases, the restatement of the
header's definitions in numpy float64 (every elementwise operation one rounding, in the header's order), the exact references
and the checks that tests/test_emu_mixed_params.py and tests/test_gpu_mixed_params.py run unchanged through the C ABI on their
own back end (tests/scoring_corpus.py: EmuBackend, GpuBackend); tests/test_mixed_params_ref.py holds the restatement itself
against the references on the CPU.

A row of a CG network with its levels fixed is a row of a Gaussian network over the real columns alone (row_net): the parameters
of every continuous variable are those of its cell.  The references and bounds of tests/gaussian_params_corpus.py apply to that
network unchanged, so they are taken from there, not restated: exact_loglik_row (mpmath at 60 digits and its bound),
predict_bound, the quantile's restatement and QUANTILE_RTOL.

References
  loglik       gaussian_params_corpus.exact_loglik_row on row_net: mpmath on the header's formula.
  mode 1       the exact Gaussian joint of the real columns given the row's levels in mpmath (A = (I - B)^-1 by forward
               substitution, mean = A c, cov = A diag(sd^2) A^T), conditioned on all other real columns with an mpmath LU solve.
               It shares no formula with the kernel's closed form over the Markov blanket.
  mode 2       brute force: prior_k times the full density of ALL real columns at level k of the target (not the children
               alone), in mpmath, normalised.
  sampler      per configuration the sample mean of the residual x_v - mu and its variance against 0 and sd^2 within 5 standard
               errors (sd / sqrt(m) and sd^2 sqrt(2 / m)).

Tolerances.  None is fitted to a kernel's output; u = 2^-53, gamma_k = k u / (1 - k u).
  loglik       against mpmath: exact_loglik_row's bound.  Between two builds (the restatement here, a kernel there): only c =
               log(sd) + const can differ, gaussian_params_corpus.restated_loglik_rows_fast's argument per cell (between_builds).
  modes 0, 1   no library call: a build equals the restatement as bytes.
  mode 2       a_k is a sum like the row term: its bound D_k against the truth is exact_loglik_row's over the children plus the
               log of the prior (LOG_ULPS ulp and nothing else: it is the first term).  w_k = exp(a_k - M): the argument carries
               D_k + D_M + u |a_k - M|, exp adds EXP_ULPS ulp; W adds gamma_r; the division one rounding.  With E = max_k (D_k +
               D_M + u |a_k - M|): |dp_k| <= p_k (expm1(2 E) + (2 EXP_ULPS + r + 3) u) (posterior_bound; expm1(2 E) covers w_k
               and W each moving by a factor within exp(+-E)).  pred is compared on the rows whose two largest a_k differ by more
               than the sum of their two bounds; the corpus asserts that those are at least three quarters of the rows.
               Between two builds the same formula with the between-builds D_k.
  sampler      a row whose draws all take the central branch equals the restatement as bytes.  Elsewhere
               |dx_v| <= sum |b_vk| |dx_k| + sd_v |dz_v| + 2 gamma_(p+2) (|c_v| + sum |b_vk x_k| + sd_v |z_v|), dz_v = BUILD_FACTOR *
               QUANTILE_RTOL[branch] |z_v| on a tail draw and 0 on a central one: the §31 bound through the row's equations."""
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
MAXQ = 4096
LOG_ULPS = gp.LOG_ULPS
EXP_ULPS = 2
HALF_LOG_2PI = gp.HALF_LOG_2PI
S_VALUES = (1, 256, 257, 700)
BIG_S = 65537
gamma = gp.gamma


# ---------------------------------------------------------------------------------------------------------------------
# A network and its rows
# ---------------------------------------------------------------------------------------------------------------------
class CgNet(SimpleNamespace):
    """n, card [n] (0: continuous), parents (Python ints [n]), offset int64 [n + 1], coef float64 [cells, n], intercept, sd
    float64 [cells]"""

    @property
    def cvars(self):
        return [v for v in range(self.n) if self.card[v] == 0]

    @property
    def nc(self):
        return len(self.cvars)

    @property
    def cells(self):
        return len(self.sd)

    def col(self, v):
        return self.cvars.index(v)

    def pa(self, v):
        return [u for u in gc.bits_of(self.parents[v] & ~(1 << v)) if u < self.n]

    def dpa(self, v):
        return [u for u in self.pa(v) if self.card[u]]

    def cpa(self, v):
        return [u for u in self.pa(v) if not self.card[u]]

    def q(self, v):
        return int(np.prod([self.card[u] for u in self.dpa(v)], dtype=np.int64)) if self.card[v] == 0 else 0

    def copy(self):
        return CgNet(n=self.n, card=list(self.card), parents=list(self.parents), offset=self.offset.copy(), coef=self.coef.copy(),
                     intercept=self.intercept.copy(), sd=self.sd.copy())


def make_net(card, parents, seed, sd_range=(0.5, 2.0), strength=(0.3, 0.9), shift=2.0):
    """random parameters for every cell of the structure; cells lie in ascending variable order, as dvs_cg_fit writes them"""
    n = len(card)
    net = CgNet(n=n, card=list(card), parents=list(parents), offset=None, coef=None, intercept=None, sd=None)
    qs = [net.q(v) for v in range(n)]
    assert all(q <= MAXQ for q in qs)
    net.offset = np.concatenate([[0], np.cumsum(qs)]).astype(np.int64)
    cells = int(net.offset[-1])
    rng = np.random.default_rng(33000 + 131 * n + seed)
    net.coef = np.zeros((cells, n))
    for v in net.cvars:
        lo, hi = int(net.offset[v]), int(net.offset[v + 1])
        for u in net.cpa(v):
            scale = 1.0 if len(net.cpa(v)) <= 4 else 0.15    # many parents: small coefficients keep the values in range
            net.coef[lo:hi, u] = rng.choice([-1.0, 1.0], hi - lo) * rng.uniform(*strength, hi - lo) * scale
    net.intercept = rng.uniform(-shift, shift, cells)
    net.sd = rng.uniform(*sd_range, cells)
    return net


def pack(levels, n):
    """int levels [S, n] -> u64 [S, ceil(n / 16)]"""
    out = np.zeros((len(levels), (n + 15) // 16), U64)
    for v in range(n):
        out[:, v // 16] |= levels[:, v].astype(U64) << U64(4 * (v % 16))
    return out


def unpack(packed, n):
    return np.stack([((packed[:, v // 16] >> U64(4 * (v % 16))) & U64(15)).astype(np.int64) for v in range(n)], axis=1)


def net_status(net, target=-1, mode=0):
    """(status bits, topological order) by the header's rules: the structural ones, then (only when they pass) bit 6 over the cells"""
    n, bits = net.n, 0
    for v in range(n):
        pm = net.parents[v] & ~(1 << v)
        if pm >> n or net.card[v] > 16:
            bits |= 16
        q = 0 if net.card[v] else 1
        for u in net.pa(v):
            if net.card[v] and not net.card[u]:
                bits |= 16
            if not net.card[v] and net.card[u] and q <= MAXQ:
                q *= net.card[u]
        if q > MAXQ or int(net.offset[v + 1]) - int(net.offset[v]) != q:
            bits |= 16
    if int(net.offset[0]) != 0 or int(net.offset[n]) != net.cells or getattr(net, "n_cont", net.nc) != net.nc:
        bits |= 16
    if target >= 0 and (net.card[target] > 0) != (mode == 2):
        bits |= 16
    placed, order = 0, []
    low = (1 << n) - 1
    for _ in range(n):
        pick = next((v for v in range(n) if not (placed >> v) & 1 and not (net.parents[v] & low & ~(1 << v) & ~placed)), None)
        if pick is None:
            return bits | 1, order
        order.append(pick)
        placed |= 1 << pick
    if bits:
        return bits, order
    for v in net.cvars:
        for cell in range(int(net.offset[v]), int(net.offset[v + 1])):
            sd = float(net.sd[cell])
            if sd != sd:
                continue
            if not (math.isfinite(net.intercept[cell]) and math.isfinite(sd) and sd > 0.0) or any(not math.isfinite(net.coef[cell, u]) for u in net.cpa(v)):
                bits |= 64
    return bits, order


def cells_of(net, v, lev, set_var=-1, set_level=0):
    """(cell [S], bad [S]) of the continuous v in rows with the levels lev [S, n]; the level of ``set_var`` is ``set_level``"""
    z, mul, bad = np.zeros(len(lev), np.int64), 1, np.zeros(len(lev), bool)
    for u in net.dpa(v):
        l = np.full(len(lev), set_level, np.int64) if u == set_var else lev[:, u]
        bad |= l >= net.card[u]
        z += l * mul
        mul *= net.card[u]
    return np.where(bad, int(net.offset[v]), int(net.offset[v]) + z), bad


def full(net, x):
    """x [S, nc] -> [S, n] with the real columns at their variables (the others are never read)"""
    out = np.full((len(x), net.n), NAN)
    out[:, net.cvars] = x
    return out


def mu_rows(net, v, cell, xf, skip=-1):
    mu = net.intercept[cell].copy()
    for u in net.cpa(v):
        if u != skip:
            mu = mu + net.coef[cell, u] * xf[:, u]
    return mu


def _visit(net, v, lev, set_var=-1, set_level=0):
    """(cell, dead [S], flags) of v: dead rows met a level out of range (bit 4) or an empty configuration (bit 7)"""
    cell, bad = cells_of(net, v, lev, set_var, set_level)
    empty = ~bad & np.isnan(net.sd[cell])
    return cell, bad | empty, (16 if bad.any() else 0) | (128 if empty.any() else 0)


def restated_sample(net, lev, seed, row_offset=0):
    """(x [S, nc], z [S, n], branch [S, n], status) of a sound network"""
    bits, order = net_status(net)
    assert not bits
    S = len(lev)
    xf, z, branch, flags = np.full((S, net.n), NAN), np.zeros((S, net.n)), np.zeros((S, net.n), np.int8), 0
    for v in order:
        if net.card[v]:
            continue
        cell, dead, f = _visit(net, v, lev)
        flags |= f
        qz = [gp.restated_quantile(gp.draw_k(seed, (row_offset + i) & gp.M32, v)) for i in range(S)]
        z[:, v], branch[:, v] = [a for a, _ in qz], [b for _, b in qz]
        val = mu_rows(net, v, cell, xf) + net.sd[cell] * z[:, v]
        xf[:, v] = np.where(dead, NAN, val)
    return np.ascontiguousarray(xf[:, net.cvars]), z, branch, flags


def cell_constants(net, log=math.log):
    return np.asarray([log(float(s)) + HALF_LOG_2PI if s == s and s > 0 else NAN for s in net.sd])


def restated_loglik_rows(net, lev, x):
    """(terms [S], status)"""
    if net_status(net)[0]:
        return np.full(len(x), NAN), net_status(net)[0]
    xf, c = full(net, x), cell_constants(net)
    term, gone, flags = np.zeros(len(x)), np.zeros(len(x), bool), 0
    with np.errstate(all="ignore"):
        for v in net.cvars:
            cell, dead, f = _visit(net, v, lev)
            flags |= f
            gone |= dead
            e = (xf[:, v] - mu_rows(net, v, cell, xf)) / net.sd[cell]
            term = term - (c[cell] + 0.5 * (e * e))
    return np.where(gone, NAN, term), flags


def between_builds(net, lev, x, children_of=None, set_level=0):
    """[S]: what two builds' row terms (or a_k over the continuous children of ``children_of`` at ``set_level``) may differ by:
    dc = 2 LOG_ULPS 2 u |ln sd| + 2 u |c| per cell, then two roundings a side on the piece and on the running magnitude"""
    xf, c = full(net, x), cell_constants(net)
    running, bound = np.zeros(len(x)), np.zeros(len(x))
    vs = net.cvars if children_of is None else [v for v in net.cvars if children_of in net.pa(v)]
    with np.errstate(all="ignore"):
        for v in vs:
            cell, _ = cells_of(net, v, lev, -1 if children_of is None else children_of, set_level)
            sd = net.sd[cell]
            e = (xf[:, v] - mu_rows(net, v, cell, xf)) / sd
            piece = np.abs(c[cell] + 0.5 * (e * e))
            dc = 2 * LOG_ULPS * 2 * U * np.abs(np.log(sd)) + 2 * U * np.abs(c[cell])
            running = running + piece + dc
            bound = bound + dc + 2 * U * (piece + dc) + 2 * U * running
    return np.nan_to_num(bound * (1 + 1e-9))


def restated_predict(net, t, mode, lev, x, prior=None):
    """modes 0, 1: (pred [S], var [S], status); mode 2: (pred u8 [S], posterior [S, r], a [S, r], status)"""
    S, r = len(x), net.card[t] if 0 <= t < net.n else 0
    bits = net_status(net, t, mode)[0]
    if bits:
        return (np.full(S, NAN), np.full(S, NAN), bits) if mode != 2 else (np.full(S, 255, np.uint8), np.full((S, min(r, 16)), NAN), None, bits)
    xf, flags = full(net, x), 0
    with np.errstate(all="ignore"):
        if mode != 2:
            cell, gone, flags = _visit(net, t, lev)
            sd = net.sd[cell]
            s = sd * sd
            pred, var = mu_rows(net, t, cell, xf), s
            if mode == 1:
                prec = 1.0 / s
                num = pred * prec
                for c in net.cvars:
                    if c == t or t not in net.pa(c):
                        continue
                    cc, dead, f = _visit(net, c, lev)
                    flags |= f
                    gone = gone | dead
                    beta = net.coef[cc, t]
                    w = beta / (net.sd[cc] * net.sd[cc])
                    res = xf[:, c] - mu_rows(net, c, cc, xf, skip=t)
                    num = num + w * res
                    prec = prec + beta * w
                pred, var = num / prec, 1.0 / prec
            return np.where(gone, NAN, pred), np.where(gone, NAN, var), flags
        c0 = cell_constants(net)
        a = np.zeros((S, r)) if prior is None else np.log(prior)
        for c in net.cvars:
            if t not in net.pa(c):
                continue
            for k in range(r):
                cc, dead, f = _visit(net, c, lev, t, k)
                flags |= f
                e = (xf[:, c] - mu_rows(net, c, cc, xf)) / net.sd[cc]
                a[:, k] = np.where(dead, NAN, a[:, k] - (c0[cc] + 0.5 * (e * e)))
        any_nan = np.isnan(a).any(axis=1)
        M = np.max(np.where(np.isnan(a), -np.inf, a), axis=1)
        label = np.argmax(np.where(np.isnan(a), -np.inf, a) == M[:, None], axis=1)
        w = np.exp(a - M[:, None])
        W = np.zeros(S)
        for k in range(r):
            W = W + w[:, k]
        post = np.where(any_nan[:, None], NAN, w / W[:, None])
        return np.where(any_nan, 255, label).astype(np.uint8), post, a, flags


# ---------------------------------------------------------------------------------------------------------------------
# The row's Gaussian network, the exact references, the bounds
# ---------------------------------------------------------------------------------------------------------------------
def row_net(net, lev_row):
    """the Gaussian network (gaussian_params_corpus.Net) over the real columns alone that the CG network is at these levels"""
    cv = net.cvars
    rank = {v: j for j, v in enumerate(cv)}
    m = len(cv)
    parents, coef, icpt, sd = [0] * m, np.zeros((m, m)), np.zeros(m), np.zeros(m)
    for v in cv:
        cell, bad = cells_of(net, v, np.asarray([lev_row]))
        assert not bad[0]
        j = rank[v]
        icpt[j], sd[j] = net.intercept[cell[0]], net.sd[cell[0]]
        for u in net.cpa(v):
            parents[j] |= 1 << rank[u]
            coef[j, rank[u]] = net.coef[cell[0], u]
    return gp.Net(n=m, parents=parents, coef=coef, intercept=icpt, sd=sd)


@gc.at60
def exact_conditional(g, t, row):
    """(mean, variance) of column t of the Gaussian network g given all its other columns at ``row``, through the joint"""
    n = g.n
    _, order = gp.net_status(g)
    A = mp.zeros(n, n)
    for v in order:
        A[v, v] = mp.mpf(1)
        for k in g.pa(v):
            b = mp.mpf(float(g.coef[v, k]))
            for j in range(n):
                A[v, j] += b * A[k, j]
    c = mp.matrix([mp.mpf(float(v)) for v in g.intercept])
    d = [mp.mpf(float(s)) ** 2 for s in g.sd]
    mean = A * c
    cov = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            cov[i, j] = mp.fsum(A[i, k] * d[k] * A[j, k] for k in range(n))
    others = [v for v in range(n) if v != t]
    if not others:
        return mean[t], cov[t, t]
    Soo = mp.matrix([[cov[i, j] for j in others] for i in others])
    Sot = mp.matrix([cov[i, t] for i in others])
    w = mp.lu_solve(Soo, Sot)
    m = mean[t] + mp.fsum(w[i] * (mp.mpf(float(row[o])) - mean[o]) for i, o in enumerate(others))
    return m, cov[t, t] - mp.fsum(w[i] * Sot[i] for i in range(len(others)))


@gc.at60
def exact_class_row(net, t, lev_row, x_row, prior_row):
    """(posterior [r] as mpf, log-weights [r] as mpf, bounds D [r] of a restated a_k) by brute force over the target's levels"""
    r = net.card[t]
    logw, D = [], []
    kids = [v for v in net.cvars if t in net.pa(v)]
    for k in range(r):
        lv = np.array(lev_row, copy=True)
        lv[t] = k
        g = row_net(net, lv)
        ll, _ = gp.exact_loglik_row(g, x_row)                # every real column, not the children alone
        p = 1.0 if prior_row is None else float(prior_row[k])
        logw.append(ll + mp.log(mp.mpf(p)))
        # the bound of a_k: the children's pieces alone are summed, in the same order, after the prior's log
        bound, running = LOG_ULPS * 2 * U * abs(math.log(p)), abs(math.log(p))
        for v in kids:
            err, mag = _piece_bound(g, net.col(v), x_row)
            running += mag
            bound += err + U * running
        D.append(bound * (1 + 1e-9))
    top = max(logw)
    w = [mp.exp(l - top) for l in logw]
    W = mp.fsum(w)
    return [v / W for v in w], logw, D


def _piece_bound(g, j, row):
    """(the error bound of the piece of column j of g at row, its magnitude): exact_loglik_row's terms for one variable"""
    sd = float(g.sd[j])
    mu = gp.restated_mu(g, j, row)
    d = float(row[j]) - mu
    e = abs(d / sd)
    dmu = gp.mu_bound(g, j, row)
    de = ((dmu + U * (abs(d) + dmu)) / sd + U * (e + 1e-300)) * (1 + 4 * U)
    dq = 0.5 * (de * (2 * e + de) + U * (e + de) ** 2)
    c = math.log(sd) + HALF_LOG_2PI
    dc = LOG_ULPS * 2 * U * abs(math.log(sd)) + U * abs(c) * (1 + 8 * U) + U * HALF_LOG_2PI
    piece = abs(c + 0.5 * e * e)
    return dq + dc + U * (piece + dq + dc), piece + dq + dc


def posterior_bound(post, a, D):
    """[r]: the module docstring's bound of a restated (or a build's) posterior row from the log-weights a and their bounds D"""
    r = len(a)
    M = max(a)
    k_top = int(np.argmax(a))
    E = max(D[k] + D[k_top] + U * abs(a[k] - M) for k in range(r))
    rel = math.expm1(2 * E) + (2 * EXP_ULPS + r + 3) * U
    return [float(p) * rel * (1 + 1e-9) + 1e-320 for p in post]


def decided(a, D):
    """the two largest a_k differ by more than the sum of their bounds"""
    order = np.argsort(a)
    return len(a) == 1 or a[order[-1]] - a[order[-2]] > D[order[-1]] + D[order[-2]]


def sample_bounds(net, lev, x, z, branch):
    """[S, n]: the bound of every real cell of a build's sample against the restated one (0 where the row is all central)"""
    _, order = net_status(net)
    xf, out = full(net, x), np.zeros((len(x), net.n))
    rtol = np.asarray([0.0] + [gp.BUILD_FACTOR * gp.QUANTILE_RTOL[b] for b in gp.BRANCHES[1:]])
    for v in order:
        if net.card[v]:
            continue
        cell, _ = cells_of(net, v, lev)
        pa = net.cpa(v)
        sd = net.sd[cell]
        dz = rtol[branch[:, v]] * np.abs(z[:, v])
        mag = np.abs(net.intercept[cell]) + sum(np.abs(net.coef[cell, u] * xf[:, u]) for u in pa) + sd * np.abs(z[:, v])
        out[:, v] = (sum(np.abs(net.coef[cell, u]) * out[:, u] for u in pa) + sd * dz + 2 * gamma(len(pa) + 2) * mag) * (1 + 1e-9)
    out[~branch.any(axis=1)] = 0.0
    return out[:, net.cvars]


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
def _mask(*vs):
    return sum(1 << v for v in vs)


def small_net():
    """n = 5: the factors 0 (3 levels) and 2 (2 levels), the reals 1, 3, 4; 3 is a root and comes before 1 in the order, 4 has
    both factors (q = 6) and both other reals as parents"""
    return make_net([3, 0, 2, 0, 0], [0, _mask(0, 3), _mask(0), 0, _mask(0, 2, 1, 3)], 1)


def random_structure(n, cards, seed, max_d=2, max_c=3):
    """a DAG in a random order: a factor takes up to max_d factors, a real up to max_d factors and max_c reals"""
    rng = np.random.default_rng(33500 + 17 * n + seed)
    order = [int(v) for v in rng.permutation(n)]
    parents = [0] * n
    for k, v in enumerate(order):
        before = order[:k]
        ds, cs = [u for u in before if cards[u]], [u for u in before if not cards[u]]
        for u in rng.choice(ds, size=min(len(ds), int(rng.integers(0, max_d + 1))), replace=False) if ds else []:
            parents[v] |= 1 << int(u)
        if not cards[v]:
            for u in rng.choice(cs, size=min(len(cs), int(rng.integers(0, max_c + 1))), replace=False) if cs else []:
                parents[v] |= 1 << int(u)
    return parents


def mid_net():
    """n = 17: seven factors (a 1-level and a 16-level one among them) between ten reals"""
    cards = [0, 3, 0, 0, 16, 0, 2, 0, 1, 0, 0, 4, 0, 5, 0, 2, 0]
    return make_net(cards, random_structure(17, cards, 2), 2)


def wide_net():
    """n = 48: eight factors, forty reals; real 20 has the three 16-level factors as parents (q = 4096), real 47 has 20 real
    parents, real 3 is a parent of many"""
    cards = [16, 0, 0, 0, 16, 0, 3, 0, 0, 2, 0, 0, 16, 0, 0, 4, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert len(cards) == 48 and cards.count(0) == 40
    parents = random_structure(48, cards, 3)
    reals = [v for v in range(48) if not cards[v]]
    parents[20] = _mask(0, 4, 12)
    for v in reals:                                          # keep the graph acyclic: 20 and 47 are rewired below
        parents[v] &= ~(1 << 47)
    parents[47] = _mask(6, *[v for v in reals if v not in (47,)][:20])
    net = make_net(cards, parents, 3)
    assert not net_status(net)[0] and net.q(20) == 4096 and len(net.cpa(47)) == 20
    return net


def kids_net():
    """n = 42: the class 0 (3 levels) and a second factor 1 (2 levels) drive 40 real children with standard deviations of 1e7
    .. 1e9, so each density is below 1e-8 and the product of 40 underflows to 0 in fp64 at every level"""
    n = 42
    cards = [3, 2] + [0] * 40
    parents = [0, 0] + [_mask(0) | (_mask(1) if v % 3 == 0 else 0) | (_mask(v - 1) if v % 4 == 1 and v > 2 else 0) for v in range(2, n)]
    net = make_net(cards, parents, 4, sd_range=(1e7, 1e9), shift=2e9)
    return net


@functools.lru_cache(maxsize=None)
def net_of(key):
    return {"small": small_net, "mid": mid_net, "wide": wide_net, "kids": kids_net}[key]()


@functools.lru_cache(maxsize=None)
def rows_of(key, S, seed=0):
    """(levels int [S, n], packed u64, x [S, nc]): uniform levels, the real columns by a forward pass with numpy's normals"""
    net = net_of(key)
    rng = np.random.default_rng(34000 + S + 7919 * seed + len(key))
    lev = np.stack([rng.integers(0, c, S) if c else rng.integers(0, 16, S) for c in net.card], axis=1).astype(np.int64)
    _, order = net_status(net)
    xf = np.full((S, net.n), NAN)
    for v in order:
        if not net.card[v]:
            cell, _ = cells_of(net, v, lev)
            xf[:, v] = mu_rows(net, v, cell, xf) + net.sd[cell] * rng.normal(0.0, 1.0, S)
    out = (lev, pack(lev, net.n), np.ascontiguousarray(xf[:, net.cvars]))
    for a in out:
        a.setflags(write=False)
    return out


def prior_of(key, t, S):
    rng = np.random.default_rng(34500 + S + t)
    p = rng.uniform(0.05, 1.0, (S, net_of(key).card[t]))
    return p / p.sum(axis=1, keepdims=True)


def class_targets(key):
    """the discrete targets of mode 2: the one with the most real children, and one with none (when there is one)"""
    net = net_of(key)
    kids = {t: sum(1 for c in net.cvars if t in net.pa(c)) for t in range(net.n) if net.card[t]}
    best = max(kids, key=kids.get)
    none = [t for t, k in kids.items() if k == 0]
    return [best] + none[:1]


def real_targets(key):
    """continuous targets: one with no real children, one with the most, one with factors among its parents"""
    net = net_of(key)
    kids = {t: sum(1 for c in net.cvars if t in net.pa(c)) for t in net.cvars}
    out = [min(kids, key=kids.get), max(kids, key=kids.get)] + [t for t in net.cvars if net.dpa(t)][:1]
    return sorted(set(out))


RULES = {"cycle": 1, "bit": 16, "illegal-arc": 16, "card17": 16, "q": 16, "offset": 16, "cells": 16, "n-cont": 16,
         "nan-coef": 64, "inf-intercept": 64, "sd0": 64, "inf-sd": 64}


def malformed(net, rule):
    """a copy of the sound small or mid network that breaks one rule alone"""
    m = net.copy()
    n = m.n
    order = net_status(net)[1]
    if rule == "cycle":
        first, last = [v for v in order if not m.card[v]][0], [v for v in order if not m.card[v]][-1]
        m.parents[first] |= 1 << last                        # real -> real against the order: the offsets stay right
    elif rule == "bit":
        m.parents[m.cvars[0]] |= 1 << n
    elif rule == "illegal-arc":
        m.parents[next(v for v in order if m.card[v])] |= 1 << next(v for v in m.cvars if not m.pa(v))     # a root real into a factor
    elif rule == "card17":
        m.card[max(v for v in range(n) if m.card[v])] = 17
    elif rule == "q":
        raise KeyError("built by too_many_configurations()")
    elif rule == "offset":
        v = m.cvars[1]
        m.offset[v + 1:] += 1
        m.coef, m.intercept, m.sd = np.vstack([m.coef, m.coef[:1]]), np.append(m.intercept, 0.0), np.append(m.sd, 1.0)
    elif rule == "cells":
        m.coef, m.intercept, m.sd = np.vstack([m.coef, m.coef[:1]]), np.append(m.intercept, 0.0), np.append(m.sd, 1.0)
    elif rule == "n-cont":
        m.n_cont = m.nc - 1
    elif rule == "nan-coef":
        v = next(v for v in m.cvars if m.cpa(v))
        m.coef[int(m.offset[v + 1]) - 1, m.cpa(v)[0]] = NAN
    elif rule == "inf-intercept":
        m.intercept[-1] = math.inf
    elif rule == "sd0":
        m.sd[0] = 0.0
    elif rule == "inf-sd":
        m.sd[-1] = math.inf
    else:
        raise KeyError(rule)
    return m


def too_many_configurations():
    """a real with four 16-level parents: q = 65 536; its offset slot says 4096, which no slot can make right"""
    cards = [16, 16, 16, 16, 0, 0]
    net = CgNet(n=6, card=cards, parents=[0, 0, 0, 0, _mask(0, 1, 2, 3), _mask(4)], offset=np.asarray([0, 0, 0, 0, 0, 4096, 4097], np.int64),
                coef=np.zeros((4097, 6)), intercept=np.zeros(4097), sd=np.ones(4097))
    return net


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI on a back end
# ---------------------------------------------------------------------------------------------------------------------
def _net_args(be, net):
    return dict(n_vars=net.n, n_cont=getattr(net, "n_cont", net.nc), n_cells=net.cells, card=be.put(np.asarray(net.card, np.uint8)),
                parents=be.put(np.asarray([p & ((1 << 64) - 1) for p in net.parents], U64)), offset=be.put(np.asarray(net.offset, np.int64)),
                coef=be.put(np.ascontiguousarray(net.coef, np.float64)), intercept=be.put(np.asarray(net.intercept, np.float64)),
                sd=be.put(np.asarray(net.sd, np.float64)))


def _at(be, h, nbytes):
    return ctypes.c_void_p(be.ptr(h).value + nbytes)


def run_sample(be, net, packed, seed, row_offset=0):
    """dvs_cgbn_sample -> (x [S, nc], status); a row of sentinels either side of x_out must survive"""
    S, nc = len(packed), net.nc
    need = be.lib.dvs_cgbn_sample_workspace_bytes(net.n)
    assert need == 256
    ws, out, status = be.put(np.zeros(need, np.uint8)), be.put(np.full((S + 2, nc), SENTINEL)), be.put(np.zeros(1, np.int32))
    gc.call(be, "dvs_cgbn_sample", **_net_args(be, net), n_rows=S, packed=be.put(np.ascontiguousarray(packed)), seed=seed, row_offset=row_offset,
            workspace=ws, workspace_bytes=need, x_out=_at(be, out, nc * 8), status=status)
    o = np.array(be.get(out), copy=True)
    assert (o[0] == SENTINEL).all() and (o[-1] == SENTINEL).all()
    return o[1:-1], int(be.get(status)[0])


def loglik_workspace(S, cells):
    return 256 + ((-(-S // 256) * 8 + 255) & ~255) + cells * 8


def run_loglik(be, net, packed, x, per_row=True):
    """dvs_cgbn_loglik -> (out, per_row [S] or None, status)"""
    S = len(packed)
    need = be.lib.dvs_cgbn_loglik_workspace_bytes(net.n, S, net.cells)
    assert need == loglik_workspace(S, net.cells)
    ws, out, status = be.put(np.zeros(need, np.uint8)), be.put(np.full(3, SENTINEL)), be.put(np.zeros(1, np.int32))
    rows = be.put(np.full(S + 2, SENTINEL)) if per_row else None
    gc.call(be, "dvs_cgbn_loglik", **_net_args(be, net), n_rows=S, packed=be.put(np.ascontiguousarray(packed)),
            x=be.put(np.ascontiguousarray(x, np.float64)), per_row=None if rows is None else _at(be, rows, 8), out=_at(be, out, 8),
            workspace=ws, workspace_bytes=need, status=status)
    o = np.array(be.get(out), copy=True)
    assert o[0] == SENTINEL and o[2] == SENTINEL
    r = None
    if per_row:
        r = np.array(be.get(rows), copy=True)
        assert r[0] == SENTINEL and r[-1] == SENTINEL
        r = r[1:-1]
    return o[1], r, int(be.get(status)[0])


def run_predict(be, net, packed, x, target, mode, prior=None, posterior=True):
    """dvs_cgbn_predict -> modes 0, 1: (pred [S], var [S], status); mode 2: (pred u8 [S], posterior [S, r] or None, status)"""
    S = len(packed)
    need = be.lib.dvs_cgbn_predict_workspace_bytes(net.n, net.cells)
    assert need == 256 + net.cells * 8
    ws, status = be.put(np.zeros(need, np.uint8)), be.put(np.zeros(1, np.int32))
    common = dict(**_net_args(be, net), n_rows=S, packed=be.put(np.ascontiguousarray(packed)), x=be.put(np.ascontiguousarray(x, np.float64)),
                  target=target, mode=mode, workspace=ws, workspace_bytes=need, status=status)
    if mode != 2:
        pred, var = be.put(np.full(S + 2, SENTINEL)), be.put(np.full(S + 2, SENTINEL))
        gc.call(be, "dvs_cgbn_predict", **common, prior=None, pred=_at(be, pred, 8), var=_at(be, var, 8), posterior=None)
        p, v = np.array(be.get(pred), copy=True), np.array(be.get(var), copy=True)
        assert p[0] == SENTINEL and p[-1] == SENTINEL and v[0] == SENTINEL and v[-1] == SENTINEL
        return p[1:-1], v[1:-1], int(be.get(status)[0])
    r = min(net.card[target], 16)
    pred = be.put(np.full(S + 32, 77, np.uint8))
    post = be.put(np.full((S + 2, r), SENTINEL)) if posterior else None
    gc.call(be, "dvs_cgbn_predict", **common, prior=None if prior is None else be.put(np.ascontiguousarray(prior, np.float64)),
            pred=_at(be, pred, 16), var=None, posterior=None if post is None else _at(be, post, r * 8))
    p = np.array(be.get(pred), copy=True)
    assert (p[:16] == 77).all() and (p[S + 16:] == 77).all()
    o = None
    if posterior:
        o = np.array(be.get(post), copy=True)
        assert (o[0] == SENTINEL).all() and (o[-1] == SENTINEL).all()
        o = o[1:-1]
    return p[16:S + 16], o, int(be.get(status)[0])


# ---------------------------------------------------------------------------------------------------------------------
# Checks on a back end
# ---------------------------------------------------------------------------------------------------------------------
def check_sample(be, key, S, seed=91):
    """rows whose draws are all central equal the restatement as bytes, every other cell lies within sample_bounds; two calls
    give equal bytes -> (central rows, the largest error / bound elsewhere)"""
    net = net_of(key)
    lev, packed, _ = rows_of(key, S)
    x, z, branch, flags = restated_sample(net, lev, seed)
    got, st = run_sample(be, net, packed, seed)
    again, _ = run_sample(be, net, packed, seed)
    assert st == 0 and flags == 0 and got.tobytes() == again.tobytes()
    central = ~branch.any(axis=1)
    if key == "small" and S > 1:                             # on the restatement first: 0.85^3 = 0.61 of the rows are expected
        assert int(central.sum()) >= S // 4, (S, int(central.sum()))
    assert got[central].tobytes() == x[central].tobytes(), (key, S, np.argwhere(got[central] != x[central])[:4])
    bounds = sample_bounds(net, lev, x, z, branch)
    err = np.abs(got - x)
    assert (err <= bounds).all(), (key, S, np.argwhere(err > bounds)[:4])
    live = bounds > 0
    return int(central.sum()), float(np.max(err[live] / bounds[live])) if live.any() else 0.0


def check_sample_cut(be, key="mid", seed=92):
    """a request cut into three calls with consecutive row_offset gives the bytes of the uncut one; another seed does not; an
    offset that wraps 2^32"""
    net = net_of(key)
    _, packed, _ = rows_of(key, 700)
    whole, _ = run_sample(be, net, packed[:600], seed, row_offset=40)
    parts = [run_sample(be, net, packed[at:at + m], seed, row_offset=40 + at)[0] for at, m in ((0, 255), (255, 88), (343, 257))]
    assert np.concatenate(parts).tobytes() == whole.tobytes()
    assert run_sample(be, net, packed[:600], seed + 1, row_offset=40)[0].tobytes() != whole.tobytes()
    same = np.repeat(packed[:1], 4, axis=0)
    wrap, _ = run_sample(be, net, same, seed, row_offset=(1 << 32) - 2)
    assert wrap[2:].tobytes() == run_sample(be, net, same[:2], seed, row_offset=0)[0].tobytes()


def check_loglik(be, key, S, exact_rows=6):
    """per_row null and given give equal out bytes; out is the stated tree over per_row as bytes; every row lies within the
    between-builds bound of the restatement and the first rows (and the last) within exact_loglik_row's of mpmath -> worst
    error / bound of the mpmath comparison"""
    net = net_of(key)
    lev, packed, x = rows_of(key, S)
    out, rows, st = run_loglik(be, net, packed, x)
    out2, _, st2 = run_loglik(be, net, packed, x, per_row=False)
    assert st == 0 and st2 == 0 and np.float64(out).tobytes() == np.float64(out2).tobytes()
    assert np.float64(gp.stated_sum(rows)).tobytes() == np.float64(out).tobytes(), (key, S)
    rest, flags = restated_loglik_rows(net, lev, x)
    bounds = between_builds(net, lev, x)
    err = np.abs(rows - rest)
    assert flags == 0 and (err <= bounds).all(), (key, S, int(np.argmax(err - bounds)), float(err.max()))
    assert abs(float(out) - gp.stated_sum(rest)) <= gp.out_bound_between_builds(rest, bounds)
    worst = 0.0
    for i in sorted(set(list(range(min(S, exact_rows))) + [S - 1])):
        term, bound = gp.exact_loglik_row(row_net(net, lev[i]), x[i])
        for have in (rows[i], rest[i]):
            e = float(abs(mp.mpf(float(have)) - term))
            assert e <= bound, (key, S, i, float(have), float(term), e, bound)
        worst = max(worst, float(abs(mp.mpf(float(rows[i])) - term)) / bound)
    return worst


def check_predict_real(be, key, S, exact_rows=3):
    """modes 0 and 1 equal the restatement as bytes (no library call); the target's own column filled with NaN changes nothing;
    mode 1 lies within predict_bound of the mpmath conditional on the first rows -> worst mode 1 error / bound"""
    net = net_of(key)
    lev, packed, x = rows_of(key, S)
    worst = 0.0
    for t in real_targets(key):
        blind = np.array(x, copy=True)
        blind[:, net.col(t)] = NAN
        for mode in (0, 1):
            pred, var, st = run_predict(be, net, packed, x, t, mode)
            pred2, var2, _ = run_predict(be, net, packed, blind, t, mode)
            rp, rv, flags = restated_predict(net, t, mode, lev, x)
            assert st == 0 and flags == 0
            assert pred.tobytes() == pred2.tobytes() == rp.tobytes() and var.tobytes() == var2.tobytes() == rv.tobytes(), (key, S, t, mode)
        for i in range(min(S, exact_rows if net.nc <= 12 else 1)):
            g = row_net(net, lev[i])
            want, wvar = exact_conditional(g, net.col(t), x[i])
            bound, rel = gp.predict_bound(g, net.col(t), x[i])
            e = float(abs(mp.mpf(float(pred[i])) - want))
            assert e <= bound, (key, t, i, float(pred[i]), float(want), e, bound)
            assert float(abs(mp.mpf(float(var[i])) - wvar) / wvar) <= rel, (key, t, i, "var")
            worst = max(worst, e / bound)
    return worst


def check_predict_class(be, key, S):
    """mode 2 with a prior and without: the posterior within posterior_bound (between builds) of the restatement, pred equal to
    it on the rows whose two largest a_k are apart by more than their bounds (at least three quarters, asserted on the
    restatement first); scrambling the target's own nibble changes nothing; posterior null gives the same pred"""
    net = net_of(key)
    lev, packed, x = rows_of(key, S)
    worst = 0.0
    for t in class_targets(key):
        r = net.card[t]
        scrambled = np.array(lev, copy=True)
        scrambled[:, t] = 15 - scrambled[:, t]
        has_kids = any(t in net.pa(c) for c in net.cvars)   # without children a null prior ties every level: the prior alone then
        for prior in ((None,) if has_kids else ()) + (prior_of(key, t, S),):
            pred, post, st = run_predict(be, net, packed, x, t, 2, prior)
            pred2, post2, _ = run_predict(be, net, pack(scrambled, net.n), x, t, 2, prior)
            pred3, _, _ = run_predict(be, net, packed, x, t, 2, prior, posterior=False)
            rp, rpost, a, flags = restated_predict(net, t, 2, lev, x, prior)
            assert st == 0 and flags == 0 and pred.tobytes() == pred2.tobytes() == pred3.tobytes() and post.tobytes() == post2.tobytes()
            D = np.stack([between_builds(net, lev, x, t, k) for k in range(r)], axis=1)
            if prior is not None:
                D = D + 2 * LOG_ULPS * 2 * U * np.abs(np.log(prior))
            keep = np.asarray([decided(a[i], D[i]) for i in range(S)])
            assert keep.sum() * 4 >= 3 * S, (key, t, int(keep.sum()), S)
            assert (pred[keep] == rp[keep]).all(), (key, t, np.argwhere(pred[keep] != rp[keep])[:4])
            for i in range(S):
                bound = posterior_bound(rpost[i], a[i], D[i])
                e = np.abs(post[i] - rpost[i])
                assert (e <= bound).all(), (key, t, i, post[i], rpost[i], bound)
                worst = max(worst, float(np.max(e / np.asarray(bound))))
            assert np.allclose(post.sum(axis=1), 1.0, rtol=0, atol=(r + 4) * 4 * U)
    return worst


def check_all_continuous_identities(be, n=17, S=300):
    """with every variable continuous the bytes are dvs_gbn_sample's, dvs_gbn_loglik's at batch 1 and dvs_gbn_predict's pred"""
    g = gp.NETS[("hub", n)]
    net = CgNet(n=n, card=[0] * n, parents=list(g.parents), offset=np.arange(n + 1, dtype=np.int64), coef=g.coef.copy(),
                intercept=g.intercept.copy(), sd=g.sd.copy())
    packed = np.zeros((S, (n + 15) // 16), U64)
    assert not net_status(net)[0]
    want, st0 = gp.run_sample(be, g, S, 93, row_offset=7)
    got, st = run_sample(be, net, packed, 93, row_offset=7)
    assert st0 == 0 and st == 0 and got.tobytes() == want.tobytes()
    x = gp.rows_for(n, S)
    wo, wr, _ = gp.run_loglik(be, [g], x)
    out, rows, st = run_loglik(be, net, packed, x)
    assert st == 0 and rows.tobytes() == wr[0].tobytes() and np.float64(out).tobytes() == wo[0].tobytes()
    for t in gp.sinks_and_sources(g):
        for mode in (0, 1):
            wp, wv, _ = gp.run_predict(be, [g], x, t, mode)
            pred, var, st = run_predict(be, net, packed, x, t, mode)
            assert st == 0 and pred.tobytes() == wp[0].tobytes() and (var == wv[0]).all(), (t, mode)


def check_malformed(be, S=300):
    """every rule, one at a time: the sampler's output stays untouched between its sentinels, the two row entry points give NaN
    (255) everywhere, the status is the rule's bit alone; the sound network next to them is evaluated as usual"""
    key = "small"
    net = net_of(key)
    lev, packed, x = rows_of(key, S)
    t_real, t_class = net.cvars[-1], 0
    base = run_loglik(be, net, packed, x)
    for rule, bit in RULES.items():
        if rule == "q":
            bad = too_many_configurations()
            bl, bp, bx = np.zeros((S, 6), np.int64), np.zeros((S, 1), U64), np.zeros((S, 2))
            tr, tc = 5, 0
        else:
            bad, (bl, bp, bx), tr, tc = malformed(net, rule), (lev, packed, x), t_real, t_class
        assert net_status(bad)[0] == bit, (rule, net_status(bad)[0])
        got, st = run_sample(be, bad, bp, 5)
        assert st == bit and (got == SENTINEL).all(), (rule, st)
        out, rows, st = run_loglik(be, bad, bp, bx)
        assert st == bit and np.isnan(out) and np.isnan(rows).all() and np.isnan(restated_loglik_rows(bad, bl, bx)[0]).all(), (rule, st)
        for mode in (0, 1):
            pred, var, st = run_predict(be, bad, bp, bx, tr, mode)
            assert st == bit and np.isnan(pred).all() and np.isnan(var).all(), (rule, mode, st)
        if rule != "card17" or bad.card[tc] <= 16:
            pred, post, st = run_predict(be, bad, bp, bx, tc, 2)
            assert st == bit and (pred == 255).all() and np.isnan(post).all(), (rule, st)
        again = run_loglik(be, net, packed, x)
        assert np.float64(again[0]).tobytes() == np.float64(base[0]).tobytes() and again[1].tobytes() == base[1].tobytes() and again[2] == 0
    # a target of the wrong kind is a refusal on the device (bit 4), not a wrong answer
    for t, mode in ((t_class, 0), (t_class, 1), (t_real, 2)):
        assert net_status(net, t, mode)[0] == 16
        if mode != 2:
            pred, var, st = run_predict(be, net, packed, x, t, mode)
            assert st == 16 and np.isnan(pred).all() and np.isnan(var).all()
        else:
            pred, _, st = run_predict(be, net, packed, x, t, mode, posterior=False)
            assert st == 16 and (pred == 255).all()


def check_row_trouble(be, S=300):
    """a level at or above its card: NaN in that row, bit 4; an empty configuration met by exactly one row: NaN in that row only,
    bit 7, every other row unchanged as bytes; a NaN data cell propagates; the sampler alike"""
    key = "small"
    net = net_of(key).copy()
    lev, packed, x = (np.array(a, copy=True) for a in rows_of(key, S))
    t = 0
    clean = dict(ll=run_loglik(be, net, packed, x), m0=run_predict(be, net, packed, x, 4, 0), m1=run_predict(be, net, packed, x, 1, 1),
                 m2=run_predict(be, net, packed, x, t, 2), sm=run_sample(be, net, packed, 5))

    def compare(net2, lev2, x2, rows_hit, bit, class_hit=None):
        p2 = pack(lev2, net.n)
        class_hit = rows_hit if class_hit is None else class_hit
        out, rows, st = run_loglik(be, net2, p2, x2)
        assert st == bit and np.isnan(out) and np.isnan(rows[rows_hit]).all()
        keep = np.setdiff1d(np.arange(S), rows_hit)
        assert rows[keep].tobytes() == clean["ll"][1][keep].tobytes()
        rest, flags = restated_loglik_rows(net2, lev2, x2)
        assert flags == bit and np.isnan(rest[rows_hit]).all() and not np.isnan(rest[keep]).any()
        got, st = run_sample(be, net2, p2, 5)
        assert st == bit and np.isnan(got[rows_hit]).any(axis=1).all() and got[keep].tobytes() == clean["sm"][0][keep].tobytes()
        pred, post, st = run_predict(be, net2, p2, x2, t, 2)
        ckeep = np.setdiff1d(np.arange(S), class_hit)
        assert st == bit and (pred[class_hit] == 255).all() and np.isnan(post[class_hit]).all()
        assert pred[ckeep].tobytes() == clean["m2"][0][ckeep].tobytes() and post[ckeep].tobytes() == clean["m2"][1][ckeep].tobytes()
        rp, rpost, _, flags = restated_predict(net2, t, 2, lev2, x2)
        assert flags == bit and (rp[class_hit] == 255).all() and (rp[ckeep] != 255).all()
        return p2

    # factor 2 (2 levels) is a parent of the real 4: level 5 in row 11
    lev2 = np.array(lev, copy=True)
    lev2[11, 2] = 5
    p2 = compare(net, lev2, x, np.asarray([11]), 16)
    pred, var, st = run_predict(be, net, p2, x, 4, 0)
    assert st == 16 and np.isnan(pred[11]) and np.isnan(var[11]) and np.delete(pred, 11).tobytes() == np.delete(clean["m0"][0], 11).tobytes()
    pred, var, st = run_predict(be, net, p2, x, 1, 1)        # 1's child 4 has the factor 2 as a parent
    assert st == 16 and np.isnan(pred[11]) and np.isnan(var[11]) and np.delete(pred, 11).tobytes() == np.delete(clean["m1"][0], 11).tobytes()
    # the configuration (0 = 2, 2 = 1) of the real 4 is empty and exactly row 17 is in it; in mode 2 every row with 2 = 1 looks
    # at it (the target 0 takes every level), so those rows are 255
    lev3 = np.array(lev, copy=True)
    lev3[(lev3[:, 0] == 2) & (lev3[:, 2] == 1), 0] = 1
    lev3[17, 0], lev3[17, 2] = 2, 1
    base = dict(ll=run_loglik(be, net, pack(lev3, net.n), x), sm=run_sample(be, net, pack(lev3, net.n), 5), m2=run_predict(be, net, pack(lev3, net.n), x, t, 2))
    clean.update(base)
    empty = net.copy()
    cell = int(net.offset[4]) + 2 + 3 * 1
    empty.sd[cell] = empty.intercept[cell] = NAN
    empty.coef[cell, :] = NAN
    assert net_status(empty)[0] == 0
    compare(empty, lev3, x, np.asarray([17]), 128, class_hit=np.nonzero(lev3[:, 2] == 1)[0])
    pred, var, st = run_predict(be, empty, pack(lev3, net.n), x, 4, 0)
    assert st == 128 and np.isnan(pred[17]) and np.isnan(var[17]) and not np.isnan(np.delete(pred, 17)).any()
    # a NaN and an infinite data cell propagate by IEEE arithmetic: no status bit
    poisoned = np.array(x, copy=True)
    poisoned[7, 1], poisoned[9, 0] = NAN, math.inf
    out, rows, st = run_loglik(be, net, packed, poisoned)
    assert st == 0 and np.isnan(rows[7]) and not np.isfinite(rows[9]) and np.isfinite(np.delete(rows, [7, 9])).all()


def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do), in the documented order"""
    assert lib.dvs_cgbn_sample_workspace_bytes(0) == 0 and lib.dvs_cgbn_sample_workspace_bytes(49) == 0
    assert lib.dvs_cgbn_sample_workspace_bytes(1) == 256 and lib.dvs_cgbn_sample_workspace_bytes(48) == 256
    assert lib.dvs_cgbn_loglik_workspace_bytes(5, 0, 10) == 0 and lib.dvs_cgbn_loglik_workspace_bytes(49, 10, 10) == 0
    assert lib.dvs_cgbn_loglik_workspace_bytes(5, 300, 11) == loglik_workspace(300, 11)
    assert lib.dvs_cgbn_predict_workspace_bytes(5, 0) == 0 and lib.dvs_cgbn_predict_workspace_bytes(5, 11) == 256 + 88

    def sample(**kw):
        a = dict(n=5, nc=3, rows=10, cells=11, card=ptr, par=ptr, off=ptr, coef=ptr, icpt=ptr, sd=ptr, packed=ptr, seed=1, ro=0, ws=ptr, wb=256,
                 out=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_cgbn_sample(a["n"], a["nc"], a["rows"], a["cells"], a["card"], a["par"], a["off"], a["coef"], a["icpt"], a["sd"], a["packed"],
                                   a["seed"], a["ro"], a["ws"], a["wb"], a["out"], a["status"], None)
    assert sample(rows=0) == 2 and sample(rows=1 << 31) == 2 and sample(cells=0) == 2 and sample(cells=(1 << 31) // 5 + 1) == 2
    assert sample(n=0) == 3 and sample(n=49) == 3 and sample(nc=0) == 3 and sample(nc=6) == 3 and sample(ro=-1) == 12
    assert all(sample(**{k: None}) == 10 for k in ("card", "par", "off", "coef", "icpt", "sd", "packed", "ws", "out", "status"))
    assert sample(wb=255) == 14 and b"256" in lib.dvs_last_error()
    assert sample(rows=0, n=0) == 2 and sample(n=0, ro=-1) == 3 and sample(ro=-1, card=None) == 12 and sample(card=None, wb=0) == 10

    def loglik(**kw):
        a = dict(n=5, nc=3, rows=300, cells=11, card=ptr, par=ptr, off=ptr, coef=ptr, icpt=ptr, sd=ptr, packed=ptr, x=ptr, per=ptr, out=ptr,
                 ws=ptr, wb=loglik_workspace(300, 11), status=ptr)
        a.update(kw)
        return lib.dvs_cgbn_loglik(a["n"], a["nc"], a["rows"], a["cells"], a["card"], a["par"], a["off"], a["coef"], a["icpt"], a["sd"], a["packed"],
                                   a["x"], a["per"], a["out"], a["ws"], a["wb"], a["status"], None)

    def predict(**kw):
        a = dict(n=5, nc=3, rows=300, cells=11, card=ptr, par=ptr, off=ptr, coef=ptr, icpt=ptr, sd=ptr, packed=ptr, x=ptr, t=1, mode=1, prior=ptr,
                 pred=ptr, var=ptr, post=ptr, ws=ptr, wb=256 + 88, status=ptr)
        a.update(kw)
        return lib.dvs_cgbn_predict(a["n"], a["nc"], a["rows"], a["cells"], a["card"], a["par"], a["off"], a["coef"], a["icpt"], a["sd"], a["packed"],
                                    a["x"], a["t"], a["mode"], a["prior"], a["pred"], a["var"], a["post"], a["ws"], a["wb"], a["status"], None)
    for fn in (loglik, predict):
        assert fn(rows=0) == 2 and fn(rows=1 << 31) == 2 and fn(cells=0) == 2 and fn(n=0) == 3 and fn(n=49) == 3 and fn(nc=0) == 3
        assert all(fn(**{k: None}) == 10 for k in ("card", "par", "off", "coef", "icpt", "sd", "packed", "x", "ws", "status"))
        assert fn(rows=0, n=0) == 2 and fn(n=0, card=None) == 3 and fn(card=None, wb=0) == 10
    assert loglik(per=None, out=None) == 10 and loglik(out=None) == 10
    assert loglik(wb=loglik_workspace(300, 11) - 1) == 14 and str(loglik_workspace(300, 11)).encode() in lib.dvs_last_error()
    assert predict(mode=3) == 12 and predict(mode=-1) == 12 and predict(t=-1) == 13 and predict(t=5) == 13
    assert predict(n=0, mode=3) == 3 and predict(mode=3, t=-1) == 12 and predict(t=-1, card=None) == 13
    assert predict(pred=None) == 10 and predict(var=None) == 10 and predict(mode=2, var=None, pred=None) == 10
    assert predict(wb=256 + 87) == 14 and str(256 + 88).encode() in lib.dvs_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# The restatement against the exact references, on the CPU (tests/test_mixed_params_ref.py)
# ---------------------------------------------------------------------------------------------------------------------
def ref_loglik(key, S=64, rows=16):
    """the restated row terms within exact_loglik_row's bound of mpmath -> worst error / bound"""
    net = net_of(key)
    lev, _, x = rows_of(key, S)
    rest, flags = restated_loglik_rows(net, lev, x)
    assert flags == 0
    worst = 0.0
    for i in range(min(S, rows)):
        term, bound = gp.exact_loglik_row(row_net(net, lev[i]), x[i])
        e = float(abs(mp.mpf(float(rest[i])) - term))
        assert e <= bound, (key, i, float(rest[i]), float(term), e, bound)
        worst = max(worst, e / bound)
    return worst


def ref_predict_real(key, S=64, rows=4):
    """restated mode 1 within predict_bound of the mpmath conditional of the row's Gaussian joint; mode 0's var is sd^2"""
    net = net_of(key)
    lev, _, x = rows_of(key, S)
    worst = 0.0
    for t in real_targets(key):
        pred, var, flags = restated_predict(net, t, 1, lev, x)
        assert flags == 0
        for i in range(min(S, rows if net.nc <= 12 else 1)):
            g = row_net(net, lev[i])
            want, wvar = exact_conditional(g, net.col(t), x[i])
            bound, rel = gp.predict_bound(g, net.col(t), x[i])
            e = float(abs(mp.mpf(float(pred[i])) - want))
            assert e <= bound, (key, t, i, float(pred[i]), float(want), e, bound)
            assert float(abs(mp.mpf(float(var[i])) - wvar) / wvar) <= rel, (key, t, i)
            worst = max(worst, e / bound)
    return worst


def ref_predict_class(key, S=48, underflow=False):
    """restated mode 2 against the brute-force posterior in mpmath: the guard first (at least three quarters of the rows have
    their two largest log-weights apart by more than the derived bounds, on the reference alone), pred on those rows, the
    posterior under posterior_bound on every row -> (rows kept, worst error / bound)"""
    net = net_of(key)
    lev, _, x = rows_of(key, S)
    t = class_targets(key)[0]
    r = net.card[t]
    kept_all, worst = S, 0.0
    for prior in (None, prior_of(key, t, S)):
        rp, rpost, a, flags = restated_predict(net, t, 2, lev, x, prior)
        assert flags == 0
        exact = [exact_class_row(net, t, lev[i], x[i], None if prior is None else prior[i]) for i in range(S)]
        keep = [decided([float(l) for l in logw], D) for _, logw, D in exact]
        assert sum(keep) * 4 >= 3 * S, (key, sum(keep), S)
        kept_all = min(kept_all, sum(keep))
        for i, (post, logw, D) in enumerate(exact):
            if keep[i]:
                assert int(rp[i]) == int(np.argmax([float(l) for l in logw])), (key, i, rp[i])
            bound = posterior_bound([float(p) for p in post], [float(l) for l in logw], D)
            for k in range(r):
                e = float(abs(mp.mpf(float(rpost[i, k])) - post[k]))
                assert e <= bound[k], (key, i, k, float(rpost[i, k]), float(post[k]), e, bound[k])
                worst = max(worst, e / bound[k])
            if underflow:                                    # the linear-domain product of the children's densities is 0 in fp64
                xf = full(net, x[i:i + 1])
                for k in range(r):
                    dens = 1.0
                    for c in net.cvars:
                        if t in net.pa(c):
                            cell, _ = cells_of(net, c, lev[i:i + 1], t, k)
                            sd = float(net.sd[cell[0]])
                            e = (float(xf[0, c]) - float(mu_rows(net, c, cell, xf)[0])) / sd
                            dens *= math.exp(-0.5 * e * e) / (sd * math.sqrt(2 * math.pi))
                    assert dens == 0.0, (key, i, k, dens)
                assert abs(float(rpost[i].sum()) - 1.0) < 1e-12
    return kept_all, worst


SAMPLING_ROWS, SAMPLING_SEED = 16384, 510


def ref_sampling_statistics():
    """16 384 restated rows of the small network on uniform levels: every configuration of every real variable has at least 1000
    expected rows; per configuration the mean of the residual x_v - mu_{v,z}(x) lies within 5 sd / sqrt(m) of 0 and its mean
    square within 5 sd^2 sqrt(2 / m) of sd^2 -> the configurations checked"""
    net = net_of("small")
    lev, _, _ = rows_of("small", SAMPLING_ROWS)
    x, _, _, flags = restated_sample(net, lev, SAMPLING_SEED)
    assert flags == 0 and not np.isnan(x).any()
    xf, checked = full(net, x), 0
    for v in net.cvars:
        assert SAMPLING_ROWS / net.q(v) >= 1000
        cell, _ = cells_of(net, v, lev)
        res = xf[:, v] - mu_rows(net, v, cell, xf)
        for c in range(int(net.offset[v]), int(net.offset[v + 1])):
            mine = res[cell == c]
            m, sd = len(mine), float(net.sd[c])
            assert m >= 800, (v, c, m)
            assert abs(mine.mean()) <= 5 * sd / math.sqrt(m), (v, c, mine.mean(), sd, m)
            assert abs((mine * mine).mean() - sd * sd) <= 5 * sd * sd * math.sqrt(2.0 / m), (v, c, (mine * mine).mean(), sd * sd, m)
            checked += 1
    return checked
