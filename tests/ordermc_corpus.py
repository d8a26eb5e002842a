"""TEST HELPER: cases, references and the checks themselves for order MCMC over family lists (csrc/dvs_ordermc.h:
dvs_order_mcmc, dvs_order_mcmc_finish; dags_vae_search_amd/ordermc.py), written once and run by tests/test_emu_ordermc.py
(emulator build) and tests/test_gpu_ordermc.py (device).  tests/test_ordermc_ref.py pins the reference itself on the CPU: that
the sampler it restates has the order-modular posterior of tests/posterior_corpus.py as its stationary distribution, and that
every seeded case below meets the bracket condition.  The device then only has to equal the reference.

Reference (ref_run): the definitions of include/dvs.h (dvs_order_mcmc) in numpy and plain Python, fp64, with the draws of
oracle/rng.py (site_key, draw) and every term's sum taken by math.fsum, so a term carries one rounding of its sum, not a chain
of them.  Nothing is shared with the kernels.

Tolerances (derived, not tuned).  M = max |score| of the list, Fmax = the largest number of families of one variable.
  A term is bestf + log(sum_j exp(score_j - bestf)).  bestf is exact.  score_j - bestf rounds by 2^-53 * 2 M, so exp carries
  that as a relative error plus a few ulp of its own (allowed: 2^-51).  The sum has positive summands in [0, 1] and at least
  one equal to 1; lane i adds ceil(Fmax / 256) of them in sequence, a wave's butterfly adds 6 levels and the waves 3 more: a
  relative error of (ceil(Fmax / 256) + 9) 2^-53.  A relative error of the sum is an absolute error of its log; the log's own
  few ulp act on a value <= log Fmax < 22, and the final addition rounds a value <= M + 22.  The reference's fsum-grade term
  has the roundings of the subtraction, exp, log and the addition as well.  With
      D = ceil(Fmax / 256) + 14
  all of it is below
      eps_term = D (2^-53 M + 2^-52),
  the form (depth + c) (2^-53 max|score| + 2^-52) with the depth of the kernel's own sum: its lanes add in sequence, so
  ceil(Fmax / 256) stands where a pure tree would have ceil(log2 F).
  A sum of k terms added in sequence (a side of Delta, k = j - i + 1 <= window + 1; the score of an order, k = n) differs
  between the two sides by the terms' errors plus, at each of the k additions, the rounding of a partial sum <= k (M + 22):
      eps_sum(k) = k eps_term + (k + 1) k 2^-53 (M + 22),      eps(Delta) = 2 eps_sum(k)   (two sides; the subtraction's
  rounding of |Delta| <= 2 k (M + 22) is inside the second term), and
      tau = 2 eps(Delta)
  is the bracket around the accept threshold: device log(u) and numpy log(u) differ by an ulp of a value <= 23, far inside
  the factor 2.  CONDITION: in every seeded case every accept decision of the reference has |log u - Delta| > tau; the share
  allowed inside the bracket is zero (tests/test_ordermc_ref.py asserts it on the CPU for every case the back ends run).  Under
  it the device makes the reference's decisions, so order, accepted, kept and best_parents are equal bytewise — and best_score,
  a sum of exact list entries in a stated order, with them — while log_score and trace are within eps_sum(n).
  A kept sample's cell is a sum of w_j = exp(score_j - term) with total <= 1: the exponent carries eps_term and the rounding
  of the subtraction (2^-53 * 2 (M + 22)), exp a few ulp (2^-51), and the sum ceil(Fmax / 256) additions in the lane, 64 in the
  wave and 3 across:
      eps_w = eps_term + 2^-52 (M + 22) + 2^-51 + (ceil(Fmax / 256) + 68) 2^-53
  per kept sample, so sums (values <= kept, added one sample at a time) are within kept eps_w + kept^2 2^-53 and prob (the
  chains' sums in a tree of depth ceil(C / 256) + 8, one division) within eps_w + (kept + ceil(C / 256) + 10) 2^-53.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

from oracle import rng as orng
from tests import exact_corpus as ex
from tests import posterior_corpus as po
from tests.abi_cases import call, entry, run

U64 = np.uint64
INF = float("inf")
SITE, SITE_INIT = 700, 701
FLAG_OFFSETS, FLAG_EMPTY_SET, FLAG_MASK, FLAG_SCORE, FLAG_ORDER = 1, 2, 4, 8, 16


# ---------------------------------------------------------------------------------------------------------------------
# Family lists
# ---------------------------------------------------------------------------------------------------------------------
def make_list(per_var):
    """per_var: for every variable a list of (mask, score), entry 0 the empty set -> namespace(n, offsets, sets, scores)"""
    n = len(per_var)
    offsets = np.zeros(n + 1, np.int64)
    offsets[1:] = np.cumsum([len(p) for p in per_var])
    sets = np.array([m for p in per_var for m, _ in p], U64)
    scores = np.array([s for p in per_var for _, s in p], np.float64)
    return SimpleNamespace(n=n, offsets=offsets, sets=sets, scores=scores, F=int(offsets[-1]))


@functools.lru_cache(maxsize=None)
def subsets_by_size(n, v, cap, candidates=None):
    """the masks of the subsets of v's candidate parents (default: every other variable) of size <= cap: by size, then by mask"""
    others = [u for u in range(n) if u != v and (candidates is None or (candidates >> u) & 1)]
    out = []
    for k in range(min(cap, len(others)) + 1):
        out.extend(sorted(sum(1 << u for u in c) for c in itertools.combinations(others, k)))
    return tuple(out)


def enumerated_list(n, cap, score_of):
    """every subset of size <= cap for every variable; score_of(v, masks u64 array) -> f64 array"""
    per = []
    for v in range(n):
        m = np.array(subsets_by_size(n, v, cap), U64)
        per.append(list(zip(m.tolist(), np.asarray(score_of(v, m), np.float64).tolist())))
    return make_list(per)


def list_from_table(table, max_parents=None, forbidden=None, size_prior=None):
    """the list FamilyScores.from_table must build: v's admissible P by size, then by mask, with the cells f(v, P) of
    posterior_corpus.f_cells bit for bit"""
    rows, n = table.shape
    f = po.f_cells(table, max_parents, forbidden, size_prior)
    pop = ex.popcounts(n)
    per = []
    for v in range(n):
        P = np.nonzero(f[:, v] > -INF)[0]
        P = P[np.lexsort((P, pop[P]))]
        per.append([(int(p), float(f[p, v])) for p in P])
    return make_list(per)


def stats(fam):
    Fmax = int(np.diff(fam.offsets).max())
    M = float(np.abs(fam.scores).max()) if fam.F else 0.0
    return Fmax, M


def eps_term(fam):
    Fmax, M = stats(fam)
    return (-(-Fmax // 256) + 14) * (2.0 ** -53 * M + 2.0 ** -52)


def eps_sum(fam, k):
    _, M = stats(fam)
    return k * eps_term(fam) + (k + 1) * k * 2.0 ** -53 * (M + 22.0)


def tau(fam, k):
    return 4.0 * eps_sum(fam, k)


def eps_w(fam):
    Fmax, M = stats(fam)
    return eps_term(fam) + 2.0 ** -52 * (M + 22.0) + 2.0 ** -51 + (-(-Fmax // 256) + 68) * 2.0 ** -53


def sums_tol(fam, kept):
    return kept * eps_w(fam) + kept * kept * 2.0 ** -53


def prob_tol(fam, kept, chains):
    return eps_w(fam) + (kept + -(-chains // 256) + 10) * 2.0 ** -53


# ---------------------------------------------------------------------------------------------------------------------
# Reference
# ---------------------------------------------------------------------------------------------------------------------
class Terms:
    """term, bestf, arg and the arc row P(. -> v | Q) of a list, memoised by (v, Q)"""

    def __init__(self, fam):
        self.fam, self.memo, self.rows = fam, {}, {}

    def _consistent(self, v, Q):
        lo, hi = int(self.fam.offsets[v]), int(self.fam.offsets[v + 1])
        sets, scores = self.fam.sets[lo:hi], self.fam.scores[lo:hi]
        ok = (sets & ~U64(Q)) == 0
        return sets[ok], scores[ok]

    def __call__(self, v, Q):
        got = self.memo.get((v, Q))
        if got is None:
            sets, scores = self._consistent(v, Q)
            at = int(np.argmax(scores))                          # the first of equal maxima: the lower list index
            top = float(scores[at])
            got = (top + math.log(math.fsum(np.exp(scores - top).tolist())), top, int(sets[at]))
            if len(self.memo) < 200000:
                self.memo[(v, Q)] = got
        return got

    def arc_row(self, v, Q):
        """f64 [n]: [u] = the sum over the consistent families of v that contain u of exp(score - term)"""
        got = self.rows.get((v, Q))
        if got is None:
            sets, scores = self._consistent(v, Q)
            w = np.exp(scores - self(v, Q)[0])
            got = np.array([math.fsum(w[(sets >> U64(u)) & U64(1) == 1].tolist()) for u in range(self.fam.n)])
            if len(self.rows) < 20000:
                self.rows[(v, Q)] = got
        return got


def start_order(n, seed, g):
    key = orng.site_key(seed, SITE_INIT, g)
    order = list(range(n))
    for k in range(n - 1, 0, -1):
        j = (int(orng.draw(key, k)) * (k + 1)) >> 32
        order[k], order[j] = order[j], order[k]
    return order


def proposal(n, window, key, t):
    """(i, j, log u) of global step t"""
    r0, r1, r2 = (int(orng.draw(key, 3 * t + d)) for d in range(3))
    i = (r0 * (n - 1)) >> 32
    m = min(window, n - 1 - i)
    j = i + 1 + ((r1 * m) >> 32)
    return i, j, math.log((r2 + 0.5) * 2.0 ** -32)


def preds_of(order):
    pred, before = {}, 0
    for v in order:
        pred[v] = before
        before |= 1 << v
    return pred


def fresh_state(n, chains):
    """what the caller hands a first call"""
    return SimpleNamespace(order=np.full((chains, n), -7, np.int32), log_score=np.full(chains, -7.0),
                           accepted=np.zeros(chains, np.int32), sums=np.zeros((chains, n, n)), kept=np.zeros(chains, np.int32),
                           best_score=np.full(chains, -INF), best_parents=np.zeros((chains, n), U64))


def ref_run(fam, chains, steps, burn_in, thin, window, seed, chain_offset=0, step_offset=0, init=1, state=None, terms=None):
    """-> namespace(order, log_score, accepted, sums, kept, best_score, best_parents, trace, prob, margins): margins holds
    (|log u - Delta| - tau) of every accept decision, all of which the CONDITION wants positive"""
    n = fam.n
    T = terms or Terms(fam)
    st = state or fresh_state(n, chains)
    out = SimpleNamespace(**{k: np.array(v, copy=True) for k, v in vars(st).items() if k in vars(fresh_state(1, 1))})
    out.trace = np.zeros((chains, steps))
    margins = []
    for c in range(chains):
        g = chain_offset + c
        key = orng.site_key(seed, SITE, g)
        order = start_order(n, seed, g) if init else [int(x) for x in st.order[c]]
        pred = preds_of(order)
        cur = {v: T(v, pred[v]) for v in range(n)}
        best, best_parents = float(out.best_score[c]), out.best_parents[c].copy()

        def consider():
            nonlocal best, best_parents
            bs = 0.0
            for v in range(n):
                bs += cur[v][1]
            if bs > best:
                best, best_parents = bs, np.array([cur[v][2] for v in range(n)], U64)
        consider()
        for s in range(steps):
            t = step_offset + s
            if n > 1:
                i, j, logu = proposal(n, window, key, t)
                new = order[:]
                new[i], new[j] = new[j], new[i]
                Q, prop = pred[order[i]], {}
                for p in range(i, j + 1):
                    prop[new[p]] = (Q, T(new[p], Q))
                    Q |= 1 << new[p]
                s_old = s_new = 0.0
                for p in range(i, j + 1):
                    s_old += cur[order[p]][0]
                    s_new += prop[new[p]][1][0]
                delta = s_new - s_old
                margins.append(abs(logu - delta) - tau(fam, j - i + 1))
                if logu < delta:
                    out.accepted[c] += 1
                    order = new
                    for v, (Q, tv) in prop.items():
                        pred[v], cur[v] = Q, tv
                    consider()
            if t >= burn_in and (t - burn_in) % thin == 0:
                for v in range(n):
                    out.sums[c, :, v] += T.arc_row(v, pred[v])
                out.kept[c] += 1
            sc = 0.0
            for v in range(n):
                sc += cur[v][0]
            out.trace[c, s] = sc
        sc = 0.0
        for v in range(n):
            sc += cur[v][0]
        out.order[c], out.log_score[c], out.best_score[c], out.best_parents[c] = order, sc, best, best_parents
    K = int(out.kept.sum())
    out.prob = out.sums.sum(0) / K if K else np.zeros((n, n))
    out.margins = np.array(margins)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Driver: dvs_order_mcmc and dvs_order_mcmc_finish through the raw C ABI on a back end of scoring_corpus
# ---------------------------------------------------------------------------------------------------------------------
EXACT = ("order", "accepted", "kept", "best_parents")
FIELDS = ("order", "log_score", "accepted", "sums", "kept", "best_score", "best_parents", "trace", "prob", "flags")


class Driver:
    def __init__(self, be):
        self.be, self.lib = be, be.lib

    def run(self, fam, chains, steps, burn_in, thin, window, seed, chain_offset=0, step_offset=0, init=1, state=None, trace=True):
        be, n = self.be, fam.n
        st = state or fresh_state(n, chains)
        h = {k: be.put(np.ascontiguousarray(getattr(st, k))) for k in vars(fresh_state(1, 1))}
        hoff, hsets, hsc = be.put(fam.offsets), be.put(fam.sets), be.put(fam.scores)
        htrace = be.put(np.full((chains, max(steps, 1)), -7.0)) if trace else None
        hprob, hflags = be.put(np.full((n, n), -7.0)), be.put(np.full(1, -7, np.int32))
        call(be, "dvs_order_mcmc", chains=chains, n_vars=n, n_families=fam.F, steps=steps, offsets=hoff, sets=hsets,
             sets_bytes=fam.F * 8, scores=hsc, scores_bytes=fam.F * 8, seed=seed, chain_offset=chain_offset, step_offset=step_offset,
             burn_in=burn_in, thin=thin, window=window, init=init, **h, sums_bytes=chains * n * n * 8, trace=htrace,
             trace_bytes=chains * steps * 8, flags=hflags)                       # h: the state, under the header's names
        call(be, "dvs_order_mcmc_finish", chains=chains, n_vars=n, sums=h["sums"], sums_bytes=chains * n * n * 8, kept=h["kept"],
             prob=hprob)
        out = SimpleNamespace(**{k: be.get(v).copy() for k, v in h.items()})
        out.trace = be.get(htrace).copy()[:, :steps] if trace else np.zeros((chains, 0))
        out.prob, out.flags = be.get(hprob).copy(), be.get(hflags).copy()
        assert be.get(hsets).tobytes() == fam.sets.tobytes() and be.get(hsc).tobytes() == fam.scores.tobytes()
        return out


def same_bytes(a, b, fields=FIELDS):
    return all(np.ascontiguousarray(getattr(a, f)).tobytes() == np.ascontiguousarray(getattr(b, f)).tobytes() for f in fields)


def close(got, want, tol, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, "NaN")
    err = float(np.abs(got - want).max()) if got.size else 0.0
    assert err <= tol, (what, err, tol)
    return err


def assert_matches(got, ref, fam, chains, what):
    """the device against the reference under the CONDITION -> the largest errors (order scores, sums, prob)"""
    n = fam.n
    assert got.flags.tolist() == [0], (what, got.flags)
    for f in EXACT:
        assert np.array_equal(getattr(got, f), getattr(ref, f)), (what, f, getattr(got, f), getattr(ref, f))
    e_score = max(close(got.log_score, ref.log_score, eps_sum(fam, n), (what, "log_score")),
                  close(got.trace, ref.trace, eps_sum(fam, n), (what, "trace")),
                  close(got.best_score, ref.best_score, eps_sum(fam, n), (what, "best_score")))
    kept = int(ref.kept.max()) if chains else 0
    e_sums = close(got.sums, ref.sums, sums_tol(fam, kept), (what, "sums"))
    e_prob = close(got.prob, ref.prob, prob_tol(fam, kept, chains), (what, "prob"))
    assert (np.diagonal(got.prob) == 0.0).all(), (what, "diagonal")
    return e_score, e_sums, e_prob


# ---------------------------------------------------------------------------------------------------------------------
# 1. Trajectories: the sizes and settings at which the kernel can go wrong
# ---------------------------------------------------------------------------------------------------------------------
def _random_scores(seed, scale=2.0):
    def score_of(v, masks):
        return np.random.default_rng(seed * 1000 + v).standard_normal(len(masks)) * scale
    return score_of


def _sparse_list(n, seed):
    """variable 1 holds only the empty set, variable 0 fewer than 256 families, the rest a count that is no multiple of 256"""
    rng = np.random.default_rng(seed)
    per = []
    for v in range(n):
        masks = list(subsets_by_size(n, v, 0 if v == 1 else 1 if v == 0 else 2))
        if v >= 2:
            masks = masks[:len(masks) - (v % 3)]
        per.append([(m, float(s)) for m, s in zip(masks, rng.standard_normal(len(masks)) * 2.0)])
    return make_list(per)


def _long_list(seed):
    """n = 18: variable 0 has the first 66 000 subsets of the others by size (up to 9), past any 16-bit index; the rest <= 1 parent"""
    n = 18
    rng = np.random.default_rng(seed)
    per = []
    for v in range(n):
        masks = list(subsets_by_size(n, v, 9 if v == 0 else 1))[:66000]
        per.append([(m, float(s)) for m, s in zip(masks, rng.standard_normal(len(masks)) * 2.0)])
    return make_list(per)


# name -> (list builder, chains, steps, burn_in, thin, window (None: n - 1), seed, init)
TRAJECTORIES = {
    "n1": (lambda: enumerated_list(1, 2, _random_scores(1)), 4, 20, 4, 1, 1, 11, 1),
    "n2": (lambda: enumerated_list(2, 2, _random_scores(2)), 4, 200, 40, 2, 1, 12, 1),
    "n5": (lambda: enumerated_list(5, 4, _random_scores(3)), 8, 300, 60, 5, 1, 13, 1),
    "n5_wide_window": (lambda: enumerated_list(5, 4, _random_scores(3)), 8, 300, 60, 1, None, 14, 1),
    "n5_identity_start": (lambda: enumerated_list(5, 2, _random_scores(4)), 4, 200, 0, 3, 2, 15, 0),
    "n33": (lambda: enumerated_list(33, 2, _random_scores(5)), 4, 200, 40, 33, 1, 16, 1),
    "n48": (lambda: enumerated_list(48, 2, _random_scores(6)), 4, 200, 40, 48, 1, 17, 1),
    "n48_wide_window": (lambda: enumerated_list(48, 2, _random_scores(6)), 4, 60, 10, 25, None, 18, 1),
    "sparse": (lambda: _sparse_list(12, 7), 6, 300, 50, 4, 3, 19, 1),
    "long": (lambda: _long_list(8), 4, 12, 2, 5, 2, 20, 1),
    "thin_beyond_steps": (lambda: enumerated_list(6, 3, _random_scores(9)), 4, 100, 1, 1000, 1, 21, 1),
    "nothing_kept": (lambda: enumerated_list(6, 3, _random_scores(9)), 4, 100, 100, 1, 5, 22, 1),
}


@functools.lru_cache(maxsize=None)
def trajectory_case(name):
    build, chains, steps, burn_in, thin, window, seed, init = TRAJECTORIES[name]
    fam = build()
    window = max(1, fam.n - 1) if window is None else window
    state = None
    if not init:
        state = fresh_state(fam.n, chains)
        state.order[:] = np.arange(fam.n, dtype=np.int32)
        state.order[1] = state.order[1][::-1]
    args = dict(chains=chains, steps=steps, burn_in=burn_in, thin=thin, window=window, seed=seed, init=init, state=state)
    return fam, args, ref_run(fam, **args)


def check_trajectory(drv, name):
    fam, args, ref = trajectory_case(name)
    assert (ref.margins > 0.0).all(), (name, "a decision of the reference lies inside the bracket")
    got = drv.run(fam, **args)
    worst = assert_matches(got, ref, fam, args["chains"], name)
    if name == "nothing_kept":
        assert not got.kept.any() and not got.prob.any() and not got.sums.any()
    if name == "thin_beyond_steps":
        assert got.kept.tolist() == [1] * args["chains"]
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 2. All-zero scores: every proposal is accepted, P(u -> v | order) in closed form
# ---------------------------------------------------------------------------------------------------------------------
def closed_arc(i, cap):
    """P(u -> v | order) for a predecessor u of a variable with i predecessors, all scores zero, sets of size <= cap"""
    return sum(math.comb(i - 1, k - 1) for k in range(1, min(i, cap) + 1)) / sum(math.comb(i, k) for k in range(min(i, cap) + 1))


def check_all_zero(drv, n=37, cap=2, chains=4, steps=60):
    """the one kept sample is the last step's, so sums is the closed form on the order the call returns"""
    fam = enumerated_list(n, cap, lambda v, m: np.zeros(len(m)))
    got = drv.run(fam, chains, steps, steps - 1, 1, 1, seed=31)
    assert got.flags.tolist() == [0] and got.accepted.tolist() == [steps] * chains and got.kept.tolist() == [1] * chains
    tol = sums_tol(fam, 1)
    for c in range(chains):
        order = [int(x) for x in got.order[c]]
        assert sorted(order) == list(range(n))
        want = np.zeros((n, n))
        for i, v in enumerate(order):
            for u in order[:i]:
                want[u, v] = closed_arc(i, cap)
        close(got.sums[c], want, tol, ("all zero", c))
        log_score = sum(math.log(sum(math.comb(i, k) for k in range(min(i, cap) + 1))) for i in range(n))
        close(got.log_score[c], log_score, eps_sum(fam, n) + 1e-13 * log_score, ("all zero", c, "log_score"))
        assert got.best_score[c] == 0.0 and not got.best_parents[c].any()
    close(got.prob, got.sums.sum(0) / chains, prob_tol(fam, 1, chains), "all zero prob")


# ---------------------------------------------------------------------------------------------------------------------
# 3. Range: scores whose exp underflows; a list in which one DAG dominates
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_case(which, n=6):
    if which == "offsets":
        fam = enumerated_list(n, 3, lambda v, m: -10000.0 * (v + 1) + 3.0 * np.random.default_rng(50 + v).standard_normal(len(m)))
        want = None
    else:
        tables, want = po.dominated(n)
        fam = list_from_table(tables[0])
    args = dict(chains=8, steps=300, burn_in=100, thin=2, window=n - 1, seed=41)
    return fam, args, ref_run(fam, **args), want


def check_range(drv, which):
    fam, args, ref, want = range_case(which)
    assert (ref.margins > 0.0).all()
    got = drv.run(fam, **args)
    for f in ("log_score", "sums", "best_score", "trace", "prob"):
        assert np.isfinite(getattr(got, f)).all(), f
    worst = assert_matches(got, ref, fam, args["chains"], which)
    if which == "offsets":
        assert (np.exp(fam.scores) == 0.0).all() and ((got.prob > 0.01) & (got.prob < 0.99)).sum() >= fam.n
    else:
        top = int(np.argmax(got.best_score))
        assert got.best_parents[top].tobytes() == np.asarray(want, U64).tobytes(), (got.best_parents[top], want)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 4. Cutting: calls with step_offset, shards with chain_offset, two identical calls
# ---------------------------------------------------------------------------------------------------------------------
def check_cutting(drv):
    fam = enumerated_list(7, 3, _random_scores(61))
    kw = dict(burn_in=37, thin=3, window=2, seed=51)
    whole = drv.run(fam, 8, 300, **kw)
    again = drv.run(fam, 8, 300, **kw)
    assert whole.flags.tolist() == [0] and whole.kept.min() > 0 and same_bytes(whole, again)
    first = drv.run(fam, 8, 100, **kw)
    second = drv.run(fam, 8, 200, step_offset=100, init=0, state=first, **kw)
    both = SimpleNamespace(**vars(second))
    both.trace = np.concatenate([first.trace, second.trace], axis=1)
    assert same_bytes(whole, both)
    a = drv.run(fam, 3, 300, **kw)
    b = drv.run(fam, 5, 300, chain_offset=3, **kw)
    for f in ("order", "log_score", "accepted", "sums", "kept", "best_score", "best_parents", "trace"):
        assert np.concatenate([getattr(a, f), getattr(b, f)]).tobytes() == getattr(whole, f).tobytes(), f


# ---------------------------------------------------------------------------------------------------------------------
# 5. Flags: a malformed list sets the word and leaves every other output untouched
# ---------------------------------------------------------------------------------------------------------------------
def check_flags(drv):
    n = 5
    good = enumerated_list(n, 2, _random_scores(71))
    lo = int(good.offsets[2])

    def broken(**at):
        fam = SimpleNamespace(**vars(good))
        fam.sets, fam.scores, fam.offsets = good.sets.copy(), good.scores.copy(), good.offsets.copy()
        for k, (idx, val) in at.items():
            getattr(fam, k)[idx] = val
        return fam
    cases = [(broken(sets=(lo, U64(1))), FLAG_EMPTY_SET), (broken(scores=(lo + 3, float("nan"))), FLAG_SCORE),
             (broken(scores=(3, INF)), FLAG_SCORE), (broken(sets=(lo + 1, U64(0b00101))), FLAG_MASK),
             (broken(sets=(lo + 1, U64(1 << n))), FLAG_MASK), (broken(sets=(good.F - 1, U64(1) << U64(63))), FLAG_MASK),
             (broken(offsets=(2, good.offsets[3])), FLAG_OFFSETS), (broken(offsets=(0, 1)), FLAG_OFFSETS)]
    blank = fresh_state(n, 4)
    for fam, bit in cases:
        got = drv.run(fam, 4, 50, 0, 1, 1, seed=5)
        assert int(got.flags[0]) & bit and not int(got.flags[0]) & FLAG_ORDER, (bit, got.flags)
        for f in vars(blank):
            assert np.array_equal(getattr(got, f), getattr(blank, f)), (bit, f)
        assert (got.trace == -7.0).all() and not got.prob.any()
    # a start order that is no permutation: that chain alone is skipped
    st = fresh_state(n, 3)
    st.order[:] = np.arange(n, dtype=np.int32)
    st.order[1, 2] = 1
    got = drv.run(good, 3, 50, 0, 1, 1, seed=5, init=0, state=st)
    assert got.flags.tolist() == [FLAG_ORDER] and got.kept.tolist() == [50, 0, 50] and got.order[1].tolist() == st.order[1].tolist()
    assert got.log_score[1] == -7.0 and not got.sums[1].any()


# ---------------------------------------------------------------------------------------------------------------------
# 6. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    """(entry point, arguments, return code, text dvs_last_error must contain): every check, and the pairs where two checks
    fail and the earlier one decides.  D: a dummy non-null pointer, never dereferenced."""
    C, n, F, steps = 8, 10, 500, 100
    cases = []
    c = entry("dvs_order_mcmc", cases, chains=C, n_vars=n, n_families=F, steps=steps, offsets=D, sets=D, sets_bytes=F * 8,
              scores=D, scores_bytes=F * 8, seed=7, chain_offset=0, step_offset=0, burn_in=20, thin=10, window=1, init=1,
              order=D, log_score=D, accepted=D, sums=D, sums_bytes=C * n * n * 8, kept=D, best_score=D, best_parents=D,
              trace=D, trace_bytes=C * steps * 8, flags=D, stream=None)
    c(2, "chains must be > 0", chains=0)
    c(2, "steps must be >= 0", steps=-1)
    c(2, "n_families must be in [1, 2^31 - 1]", n_families=0)
    c(2, "n_families must be in [1, 2^31 - 1]", n_families=1 << 31)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "chains * n_vars^2 must be < 2^31", chains=1 << 20, n_vars=48, sums_bytes=1 << 40, trace_bytes=1 << 40)
    for name in ("offsets", "sets", "scores", "order", "log_score", "accepted", "sums", "kept", "best_score", "best_parents",
                 "flags"):
        c(10, "null pointer", **{name: None})
    c(12, "chain_offset and step_offset must be >= 0", chain_offset=-1)
    c(12, "chain_offset and step_offset must be >= 0", step_offset=-1)
    c(13, "window must be in [1, max(1, n_vars - 1)]", window=0)
    c(13, "window must be in [1, max(1, n_vars - 1)]", window=n)
    c(13, "window must be in [1, max(1, n_vars - 1)]", n_vars=1, window=2)
    c(13, "thin must be >= 1", thin=0)
    c(13, "burn_in must be >= 0", burn_in=-1)
    c(13, "init must be 0 or 1", init=2)
    c(13, "3 * (step_offset + steps) must be < 2^32", step_offset=(1 << 32) // 3 - steps + 1)
    c(13, "3 * (step_offset + steps) must be < 2^32", step_offset=1 << 40)
    c(14, f"sets_bytes < n_families * 8 = {F * 8}", sets_bytes=F * 8 - 1)
    c(14, f"scores_bytes < n_families * 8 = {F * 8}", scores_bytes=F * 8 - 1)
    c(14, f"sums_bytes < chains * n_vars^2 * 8 = {C * n * n * 8}", sums_bytes=C * n * n * 8 - 1)
    c(14, f"trace_bytes < chains * steps * 8 = {C * steps * 8}", trace_bytes=C * steps * 8 - 1)
    c(2, "chains must be > 0", chains=0, n_vars=49)                                    # counts before n_vars
    c(2, "steps must be >= 0", steps=-1, n_families=0)                                 # steps before n_families
    c(3, "n_vars must be in [1, 48]", n_vars=49, offsets=None)                         # n_vars before null
    c(10, "null pointer", flags=None, chain_offset=-1)                                 # null before the offsets
    c(12, "chain_offset and step_offset must be >= 0", step_offset=-1, window=0)       # offsets before the arguments
    c(13, "window must be in [1, max(1, n_vars - 1)]", window=0, thin=0)               # window before thin
    c(13, "thin must be >= 1", thin=0, step_offset=1 << 40)                            # thin before the draw bound
    c(13, "3 * (step_offset + steps) must be < 2^32", step_offset=1 << 40, sets_bytes=0)   # arguments before the sizes
    c(14, f"sets_bytes < n_families * 8 = {F * 8}", sets_bytes=0, scores_bytes=0)      # sets before scores
    c(14, f"scores_bytes < n_families * 8 = {F * 8}", scores_bytes=0, sums_bytes=0)    # scores before sums
    c(14, f"sums_bytes < chains * n_vars^2 * 8 = {C * n * n * 8}", sums_bytes=0, trace_bytes=0)   # sums before trace
    c(14, "sets_bytes", trace=None, trace_bytes=0, sets_bytes=0)                       # a null trace takes no size; sets_bytes decides

    c = entry("dvs_order_mcmc_finish", cases, chains=C, n_vars=n, sums=D, sums_bytes=C * n * n * 8, kept=D, prob=D, stream=None)
    c(2, "chains must be > 0", chains=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "chains * n_vars^2 must be < 2^31", chains=1 << 20, n_vars=48)
    for name in ("sums", "kept", "prob"):
        c(10, "null pointer", **{name: None})
    c(14, f"sums_bytes < chains * n_vars^2 * 8 = {C * n * n * 8}", sums_bytes=C * n * n * 8 - 1)
    c(3, "n_vars must be in [1, 48]", n_vars=0, sums=None)                             # n_vars before null
    c(10, "null pointer", prob=None, sums_bytes=0)                                     # null before the size
    return cases


def check_argument_refusals(lib, D):
    run(lib, validation_cases(D))
