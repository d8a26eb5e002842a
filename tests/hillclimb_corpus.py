"""TEST HELPER: cases, references and the checks themselves for the greedy hill climb (csrc/dvs_hillclimb.h:
dvs_bn_toggle_scores, dvs_hc_step; dags_vae_search_amd/hillclimb.py), written once and run by tests/test_emu_hillclimb.py
(emulator build) and tests/test_gpu_hillclimb.py (device).  Data makers and back ends are those of tests/scoring_corpus.py —
imported, not copied.  The two test modules differ only in the driver that runs the loop: on the emulator `Driver`, the
launch sequence of hill_climb through the raw C ABI by argument name (tests/abi_cases.py: call); on the device `GpuDriver`,
which replaces the toggle table and the climb by BNLearnWrapper.toggle_scores and hill_climb themselves.

References
  select_ref    the move rules of include/dvs.h (dvs_hc_step) restated in Python ints and numpy float64: ancestor closure on
                bit rows, the same delta expressions in the same operand order, the same tie-break.  Exact: no tolerance.
                tests/test_hillclimb_ref.py pins it against brute force with Kahn's algorithm on the moved graph.
  oracle_local  a float64 local score that shares no code with the kernel: oracle.bic.local_score for bic, the
                scipy.special.gammaln evaluation of tests/bn_score_corpus.py (second_local) for bde; T_abs is the corpus'
                sum of |terms| + |penalty|.
There is no bnlearn run to pin against (R is not available to this suite; the reference project scores one graph per
Rscript and records no hc trajectory): parity with bnlearn's `hc` rests on the move rules, DESIGN.md §14.

Three layers (see each check): the toggle table is exact against dvs_bn_scores; the step kernel is exact against select_ref
on the device's own table at every traced step; the trajectory is greedy for the float64 oracle within
    tau = 4 * 1e-12 * max T_abs over the families entering the two compared deltas
(1e-12 * T is what the scoring corpus asserts per local score; a reversal delta holds four local scores).
"""
import functools
import math
from collections import namedtuple

import numpy as np
from scipy.special import gammaln

from oracle import bic as obic
from oracle import features as ofeat
from tests import bn_score_corpus as bn
from tests import scoring_corpus as sc
from tests.abi_cases import at, call, call_rc
from tests.helpers import load_npz

U64 = np.uint64
NAN = float("nan")
TAU_RTOL = 4 * sc.BIC_RTOL
OPS = ("add", "delete", "reverse")
# A covered-edge reversal leaves bic and bde unchanged in exact arithmetic; in fp64 its delta is rounding noise of either
# sign (1e-12 on asia), and at min_delta = 0 a climb takes the positive ones: moves that gain nothing and need not raise the
# rounded total.  The cases climb with the square root of the machine epsilon, far above that noise (1e-12 * T) and far
# below any gain the data can show, so "scores strictly increase along the trace" is a property the arithmetic can keep.
MIN_DELTA = 2.0 ** -26


# ---------------------------------------------------------------------------------------------------------------------
# select_ref: the move rules
# ---------------------------------------------------------------------------------------------------------------------
def closure(P):
    """reach[v] = ancestors of v, from bit rows P[v] (Python ints)"""
    n = len(P)
    reach = [int(x) for x in P]
    for k in range(n):
        for v in range(n):
            if (reach[v] >> k) & 1:
                reach[v] |= reach[k]
    return reach


def has_cycle(P):
    return any((r >> v) & 1 for v, r in enumerate(closure(P)))


def legal_moves(P, max_parents=None, forbidden=None):
    """[(code, op, v, u)] of the moves the rules allow on the structure P (scores not looked at), in code order"""
    n = len(P)
    P = [int(x) for x in P]
    reach = closure(P)
    cap = max_parents if (max_parents is not None and max_parents > 0) else None
    forb = [0] * n if forbidden is None else [int(x) for x in forbidden]
    pc = [bin(x).count("1") for x in P]
    out = []
    for v in range(n):
        for u in range(n):
            if u == v:
                continue
            if not (P[v] >> u) & 1:
                if not (reach[u] >> v) & 1 and (cap is None or pc[v] < cap) and not (forb[v] >> u) & 1:
                    out.append((v * n + u, 0, v, u))
            else:
                out.append((n * n + v * n + u, 1, v, u))
                children_u = sum(1 << w for w in range(n) if (P[w] >> u) & 1)
                if not (children_u & ~(1 << v)) & (reach[v] | (1 << v)) and (cap is None or pc[u] < cap) \
                        and not (forb[u] >> v) & 1:
                    out.append((2 * n * n + v * n + u, 2, v, u))
    return sorted(out)


def move_delta(op, v, u, L, T):
    """the delta expressions of include/dvs.h, in that operand order, in float64; NaN when a cell is refused"""
    d = np.float64(T[v, u]) - np.float64(L[v])
    if op == 2:
        d = d + (np.float64(T[u, v]) - np.float64(L[u]))
    return d


def best_move(P, L, T, max_parents=None, forbidden=None):
    """(code, delta) of the best legal move — largest delta, exact ties to the lowest code — or None"""
    best = None
    for code, op, v, u in legal_moves(P, max_parents, forbidden):
        d = move_delta(op, v, u, L, T)
        if np.isnan(d):
            continue
        if best is None or d > best[1]:                     # code order: a tie keeps the lower code
            best = (code, d)
    return best


def select_ref(P, L, T, max_parents=None, forbidden=None, min_delta=0.0):
    """The move dvs_hc_step takes on one structure: (code, delta) or None (converged)."""
    best = best_move(P, L, T, max_parents, forbidden)
    return best if best is not None and best[1] > min_delta else None


def apply_move(P, code):
    n = len(P)
    op, v, u = code // (n * n), (code % (n * n)) // n, code % n
    P = [int(x) for x in P]
    P[v] ^= 1 << u
    if op == 2:
        P[u] |= 1 << v
    return P, op, v, u


# ---------------------------------------------------------------------------------------------------------------------
# oracle_local: float64 scores that share nothing with the kernel
# ---------------------------------------------------------------------------------------------------------------------
_oracle_memo = {}


def oracle_local(data, card, v, parents, typ, arg, _key=None):
    """(score, T_abs) of one family, memoised (pass the data set's name as _key)."""
    parents = tuple(sorted(int(p) for p in parents))
    key = (_key if _key is not None else id(data), v, parents, typ, arg)
    if key in _oracle_memo:
        return _oracle_memo[key]
    if typ == "bic":
        assert arg is None
        score = obic.local_score(data.astype(np.int64), card, v, parents)
        T_abs = sc.reference_local_score(data, card, v, parents)[1]
    else:
        assert typ == "bde"
        c = bn.cell_counts(data, card, v, parents)
        score = bn.second_local(c, typ, arg)
        aj, ajk = bn._prior(typ, arg, c.r, c.q, len(c.nj_row), lambda x, y: float(x) / float(y))
        T_abs = float(np.abs(gammaln(aj + c.nj_row.astype(np.float64))).sum() + len(c.nj_row) * abs(gammaln(float(aj)))
                      + np.abs(gammaln(ajk + c.njk.astype(np.float64))).sum() + len(c.njk) * abs(gammaln(float(ajk))))
    _oracle_memo[key] = (float(score), float(T_abs))
    return _oracle_memo[key]


# ---------------------------------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------------------------------
HcCase = namedtuple("HcCase", "name key data card starts max_steps max_parents forbidden min_delta")
ASIA_KNOWN = {1: [0], 2: [], 3: [], 4: [1], 5: [0, 1], 6: [1, 4], 7: [3, 4, 5]}     # tests/problem/bn/test_bnlearn.py:22-55
CASE_NAMES = ("asia", "sachs", "syn17", "syn33", "syn48", "single", "forbidden", "capped")
TYPES = {"asia": (("bic", None), ("bde", 10.0))}                   # every other case: bic


def case_types(name):
    return TYPES.get(name, (("bic", None),))


def _real(name):
    data = load_npz(f"bn_{name}_data.npz")["data"].astype(np.uint8)
    return data, (data.max(0) + 1).astype(np.uint8)


def _dag_masks(n, count, seed):
    graphs = ofeat.synthetic_dags(n, n, count, seed=seed)
    m = np.zeros((count, n), U64)
    for b, (lab, edges) in enumerate(graphs):
        for u, v in edges:
            m[b, lab[v]] |= U64(1) << U64(lab[u])
    return m


def _random_masks(n, count, seed, max_parents):
    rng = np.random.default_rng(seed)
    return sc.masks_of(n, *[sc._random_dag(rng, n, max_parents) for _ in range(count)])


@functools.lru_cache(maxsize=None)
def hc_case(name):
    if name in ("asia", "single", "forbidden", "capped"):
        data, card = _real("asia")
        starts = np.concatenate([np.zeros((1, 8), U64), _dag_masks(8, 32, seed=11)])
        if name == "asia":
            return HcCase(name, "asia", data, card, starts, 40, None, None, MIN_DELTA)
        if name == "single":
            return HcCase(name, "asia", data, card, starts[7:8], 40, None, None, MIN_DELTA)
        if name == "capped":
            return HcCase(name, "asia", data, card, starts[:5] & U64(0), 40, 1, None, MIN_DELTA)
        # forbid, in both directions, the first edge the unconstrained climb from the empty graph adds, and one more edge
        forb = np.zeros(8, U64)
        forb[4] |= U64(1) << U64(1)
        forb[1] |= U64(1) << U64(4)
        forb[7] |= U64(1) << U64(5)
        return HcCase(name, "asia", data, card, starts[:5], 40, None, forb, MIN_DELTA)
    if name == "sachs":
        data, card = _real("sachs")
        starts = np.concatenate([np.zeros((1, 11), U64), _random_masks(11, 7, 12, 3)])
        return HcCase(name, "sachs", data, card, starts, 80, 3, None, MIN_DELTA)
    n, S, B, mp, steps = {"syn17": (17, 500, 4, 3, 120), "syn33": (33, 300, 3, 2, 160), "syn48": (48, 300, 4, 2, 220)}[name]
    rng = np.random.default_rng(n)
    data, card = sc.synthetic_dataset(n, S, rng.integers(2, 4, n), seed=900 + n)
    assert np.array_equal(card, data.max(0) + 1)
    starts = np.concatenate([np.zeros((1, n), U64), _random_masks(n, B - 1, 13 + n, 2)])
    if name == "syn17":                                  # a parent in the second data word from the first step on
        starts[1, 3] |= U64(1) << U64(16)
        starts[1, 16] = U64(0)
        assert not has_cycle(starts[1])
    return HcCase(name, name, data, card, starts, steps, mp, None, MIN_DELTA)


def any_case(name):
    return refusal_case() if name == "keybits" else hc_case(name)


def _neighbourhood(case, P, typ, arg):
    """(L [n], T [n, n], Tabs_L [n], Tabs_T [n, n]) of one structure from the oracle"""
    n = len(P)
    L, T = np.zeros(n), np.full((n, n), np.nan)
    aL, aT = np.zeros(n), np.zeros((n, n))
    for v in range(n):
        L[v], aL[v] = oracle_local(case.data, case.card, v, sc.mask_bits(P[v]), typ, arg, case.key)
        for u in range(n):
            if u != v:
                T[v, u], aT[v, u] = oracle_local(case.data, case.card, v, sc.mask_bits(int(P[v]) ^ (1 << u)), typ, arg, case.key)
    return L, T, aL, aT


@functools.lru_cache(maxsize=None)
def reference_climb(name, typ, arg):
    """The oracle's own greedy run (select_ref on oracle scores) from every start: steps per row.  Asserts that max_steps is
    enough for every row to converge by itself, and what each case is there to show."""
    case = hc_case(name)
    steps, finals = [], []
    for b in range(len(case.starts)):
        P = [int(x) for x in case.starts[b]]
        assert not has_cycle(P), (name, b)
        k = 0
        while True:
            L, T, _, _ = _neighbourhood(case, P, typ, arg)
            mv = select_ref(P, L, T, case.max_parents, case.forbidden, case.min_delta)
            if mv is None:
                break
            P = apply_move(P, mv[0])[0]
            k += 1
            assert k < case.max_steps, (name, typ, b, "max_steps too small for the reference to converge")
        steps.append(k)
        finals.append(P)
    if case.max_parents:
        assert any(bin(x).count("1") == case.max_parents for P in finals for x in P), (name, "max_parents is never reached")
    if name == "syn17":
        assert any((x >> 16) & 1 for P in finals for x in P)
    return steps, finals


# ---------------------------------------------------------------------------------------------------------------------
# Drivers
# ---------------------------------------------------------------------------------------------------------------------
Climb = namedtuple("Climb", "parents scores steps converged flags codes deltas L T")


class Driver:
    """the raw C ABI on a back end of scoring_corpus, the packed data and the level counts resident on it: the launch
    sequence of hillclimb.hill_climb"""

    def __init__(self, be, case, typ, arg):
        self.be, self.case, self.typ, self.arg = be, case, typ, arg
        self.d, self.c = be.put(sc.pack(case.data)), be.put(np.ascontiguousarray(case.card))

    def local(self, P):
        rc, scratch, out, status = bn.run_bn(self.be, self.case.data, self.case.card, P, self.typ, self.arg)
        assert rc == 0
        return out, scratch, status

    def _toggle_on(self, B, hP, hwl, hL, hT, hstatus):
        """one dvs_bn_toggle_scores on handles of this back end"""
        S, n = self.case.data.shape
        call(self.be, "dvs_bn_toggle_scores", batch=B, n_vars=n, n_samples=S, data=self.d, card=self.c, parents=hP,
             score_type=bn.TYPE_CODE[self.typ], score_arg=NAN if self.arg is None else float(self.arg), worklist=hwl, local=hL,
             local_bytes=B * n * 8, toggles=hT, toggles_bytes=B * n * n * 8, status=hstatus)

    def toggle(self, P, worklist=None, out=None):
        be = self.be
        P = np.ascontiguousarray(P, U64)
        B, n = P.shape
        L, T = out if out is not None else (np.full((B, n), -7.0), np.full((B, n, n), -7.0))
        hP, hwl = be.put(P), None if worklist is None else be.put(worklist)
        hL, hT, status = be.put(L), be.put(T), be.put(np.zeros(1, np.int32))
        self._toggle_on(B, hP, hwl, hL, hT, status)
        L[...], T[...] = be.get(hL), be.get(hT)
        return L, T, int(be.get(status)[0])

    def _step_args(self, P, L, T, max_parents, forbidden, min_delta, step_cap, worklist_fill):
        """the named arguments of one dvs_hc_step on fresh handles, every output at its start value; `active` is the caller's"""
        be = self.be
        P, L, T = np.array(P, U64), np.array(L, np.float64), np.ascontiguousarray(T, np.float64)
        B, n = P.shape
        zeros = lambda: be.put(np.zeros(B, np.int32))
        return dict(batch=B, n_vars=n, parents=be.put(P), local=be.put(L), toggles=be.put(T), toggles_bytes=B * n * n * 8,
                    max_parents=max_parents or 0, min_delta=float(min_delta),
                    forbidden=None if forbidden is None else be.put(np.ascontiguousarray(forbidden, U64)), step_cap=step_cap,
                    worklist=be.put(np.full(2 * B, worklist_fill, np.int32)), steps=zeros(), converged=zeros(), flags=zeros(),
                    trace=be.put(np.zeros((B, step_cap, 2), np.int64)), trace_bytes=B * step_cap * 16)

    def step(self, P, L, T, max_parents=None, forbidden=None, min_delta=0.0, step_cap=1):
        """one dvs_hc_step on given tables -> (P, L, worklist, steps, converged, flags, trace, active)"""
        be = self.be
        h = self._step_args(P, L, T, max_parents, forbidden, min_delta, step_cap, 5)
        act = be.put(np.zeros(1, np.int32))
        call(be, "dvs_hc_step", **h, active=act)
        g = lambda k: be.get(h[k]).copy()
        return g("parents"), g("local"), g("worklist"), g("steps"), g("converged"), g("flags"), g("trace"), int(be.get(act)[0])

    def climb(self, starts, max_steps, max_parents=None, forbidden=None, min_delta=0.0, check_every=8):
        be = self.be
        B, n = np.shape(starts)
        h = self._step_args(starts, np.full((B, n), -7.0), np.full((B, n, n), -7.0), max_parents, forbidden, min_delta, max_steps, -1)
        act, status = be.put(np.zeros(max_steps, np.int32)), be.put(np.zeros(1, np.int32))
        self._toggle_on(B, h["parents"], None, h["local"], h["toggles"], status)
        for t in range(max_steps):
            call(be, "dvs_hc_step", **h, active=at(be, act, 4 * t))
            self._toggle_on(B, h["parents"], h["worklist"], h["local"], h["toggles"], status)
            if (t + 1) % check_every == 0 and be.get(act)[t] == 0:
                break
        g = lambda k: be.get(h[k]).copy()
        P, fl, tr = g("parents"), g("flags"), g("trace")
        scores = self.local(P)[0] if not fl.any() else np.full(B, np.nan)
        return Climb(P, scores, g("steps"), g("converged"), fl, tr[..., 0].copy(), tr[..., 1].copy().view(np.float64), g("local"),
                     g("toggles"))


class GpuDriver(Driver):
    """the package itself where it has the call: BNLearnWrapper.toggle_scores and hill_climb on cuda:0"""

    def __init__(self, be, case, typ, arg):
        from dags_vae_search_amd import BNLearnWrapper
        super().__init__(be, case, typ, arg)
        self.torch = be.torch
        kw = {} if arg is None else ({"iss": arg} if typ in ("bde", "bds") else {"k": arg})
        assert np.array_equal(case.card, case.data.max(0) + 1)                  # the wrapper takes card from the data
        self.ev = BNLearnWrapper(case.name, typ, data=case.data, **kw)

    def _t(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, U64).view(np.int64).copy()).cuda()

    def toggle(self, P, worklist=None, out=None):
        t = self.torch
        if out is not None:
            Ld, Td = t.from_numpy(out[0]).cuda(), t.from_numpy(out[1]).cuda()
            self.ev.toggle_scores(self._t(P), worklist=t.from_numpy(worklist).cuda(), out=(Ld, Td))
            out[0][...] = Ld.cpu().numpy()
            out[1][...] = Td.cpu().numpy()
            return out[0], out[1], 0
        L, T, status = self.ev.toggle_scores(self._t(P), return_status=True)
        return L.cpu().numpy(), T.cpu().numpy(), int(status.item())

    def climb(self, starts, max_steps, max_parents=None, forbidden=None, min_delta=0.0, check_every=8):
        from dags_vae_search_amd import hill_climb
        forb = None if forbidden is None else self._t(forbidden)
        r = hill_climb(self.ev, self._t(starts), max_steps=max_steps, max_parents=max_parents, min_delta=min_delta,
                       forbidden=forb, check_every=check_every, trace=True)
        c = lambda x: x.cpu().numpy()
        # the tables the loop ended with are the driver's own business: recomputed for the checks that want them
        return Climb(c(r.parents).view(U64), c(r.scores), c(r.steps), c(r.converged), c(r.flags), c(r.trace[0]),
                     c(r.trace[1]), None, None)


@functools.lru_cache(maxsize=None)
def _climb_cached(make_driver, name, typ, arg):
    case = hc_case(name)
    drv = make_driver(name, typ, arg)
    return drv, drv.climb(case.starts, case.max_steps, case.max_parents, case.forbidden, case.min_delta)


# ---------------------------------------------------------------------------------------------------------------------
# Layer 1: the toggle table, exact
# ---------------------------------------------------------------------------------------------------------------------
TOGGLE_VARIANTS = (("bic", None), ("aic", 0.3), ("bde", 10.0), ("k2", None))
TOGGLE_CASES = ("asia", "syn17")


def toggle_masks(name):
    """a few structures of the case with parent sets of 0 .. 3: enough for both counting outcomes of a flip (add, delete)"""
    case = hc_case(name)
    return case.starts[:3] if name == "asia" else case.starts[:2]


def check_toggle_exact(drv, P):
    """L is dvs_bn_scores' local scores; T[:, v, u] is dvs_bn_scores' local score column v of the batch with bit u of row
    v flipped; the diagonal is NaN; all bitwise."""
    P = np.ascontiguousarray(P, U64)
    B, n = P.shape
    L, T, status = drv.toggle(P)
    _, loc, st0 = drv.local(P)
    assert status == st0 == 0
    assert L.tobytes() == loc.tobytes()
    for v in range(n):
        assert np.isnan(T[:, v, v]).all()
        for u in range(n):
            if u == v:
                continue
            Q = P.copy()
            Q[:, v] ^= U64(1) << U64(u)
            _, locq, _ = drv.local(Q)
            assert T[:, v, u].tobytes() == locq[:, v].tobytes(), (v, u)
    return L, T


@functools.lru_cache(maxsize=None)
def refusal_case():
    """n = 17, sixteen 16-level columns and one 8-level column (scoring_corpus' keybits64 data): variable 0 with parents
    1 .. 14 and 16 holds 63 key bits; adding 15 makes 64 and is refused."""
    data, card = sc.synthetic_dataset(17, 512, [16] * 16 + [8], seed=55)
    P = sc.masks_of(17, {0: list(range(1, 15)) + [16], 5: [16]}, {3: [1, 2], 16: [0]})
    return HcCase("keybits", "keybits", data, card, P, 6, None, None, MIN_DELTA)


def check_toggle_refusal(drv):
    case = drv.case
    P = case.starts
    L, T, status = drv.toggle(P)
    assert status == 16
    want_nan = np.zeros(T.shape, bool)
    for b in range(len(P)):
        for v in range(17):
            for u in range(17):
                ps = [x for x in sc.mask_bits(int(P[b, v]) ^ (1 << u)) if x != v]
                c = sc._case("x", case.data, case.card, sc.masks_of(17, {v: ps}))
                want_nan[b, v, u] = u == v or sc.expected_path(c, 0, v) == "refused"
    assert want_nan[0, 0, 15] and want_nan.sum() == 2 * 17 + 1                  # the diagonals and exactly that one cell
    assert np.array_equal(np.isnan(T), want_nan)
    assert not np.isnan(L).any()
    _, loc, _ = drv.local(P)
    assert L.tobytes() == loc.tobytes()
    Q = P.copy()
    Q[0, 0] ^= U64(1) << U64(3)                                                 # a neighbour of the refused cell's row
    _, locq, _ = drv.local(Q)
    assert T[0, 0, 3].tobytes() == locq[0, 0].tobytes()
    # the climb never takes the refused move, although nothing else bars it
    r = drv.climb(P, case.max_steps)
    assert not r.flags.any()
    n = 17
    for b in range(len(P)):
        assert r.steps[b] > 0
        for k in range(r.steps[b]):
            assert int(r.codes[b, k]) != 0 * n * n + 0 * n + 15
    return r


def check_incremental_equals_full(drv, P, max_parents=None):
    """one applied move (every structure its own best one), then the incremental pass on the worklist the step wrote: the
    tables equal a full pass on the new masks, bitwise, all rows."""
    P = np.ascontiguousarray(P, U64)
    L, T, _ = drv.toggle(P)
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T, max_parents=max_parents)
    assert act > 0 and not fl.any()
    assert not np.array_equal(P1, P)
    L1 = L1.copy()
    T1 = T.copy()
    drv.toggle(P1, worklist=wl, out=(L1, T1))
    Lf, Tf, _ = drv.toggle(P1)
    assert L1.tobytes() == Lf.tobytes() and T1.tobytes() == Tf.tobytes()
    moved = {(b, int(w)) for b in range(len(P)) for w in wl[2 * b:2 * b + 2] if w >= 0}
    assert moved == {(b, v) for b in range(len(P)) for v in range(P.shape[1]) if P1[b, v] != P[b, v]}
    return len(moved)


# ---------------------------------------------------------------------------------------------------------------------
# Layer 2: the step kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
FULL_REPLAY_CELLS = 6000       # B n^2 up to which every replayed step takes a full toggle pass


def check_replay(drv, case, r):
    """Replays the trace: at every step the test's own table of the masks so far and select_ref give exactly the traced
    (code, delta bits); at the end they give no move for converged rows; steps, converged and the final masks follow.
    The table is a full toggle pass per step where that is affordable (B n^2 <= FULL_REPLAY_CELLS); above, it is kept up
    by incremental passes on a worklist the TEST derives from the traced move, and compared with a full pass on the final
    masks at the end (layer 1 shows the two passes equal).  Returns per-step totals (k_bic_sum's order) for layer 3."""
    B, n = case.starts.shape
    P = case.starts.copy()
    full = B * n * n <= FULL_REPLAY_CELLS
    L, T, _ = drv.toggle(P)
    steps = np.zeros(B, np.int64)
    done = np.zeros(B, bool)
    totals = [[] for _ in range(B)]
    for k in range(case.max_steps + 1):
        wl = np.full(2 * B, -1, np.int32)
        for b in range(B):
            tot = 0.0
            for v in range(n):
                tot = tot + L[b, v]
            if not done[b]:
                totals[b].append(tot)
            if done[b]:
                continue
            mv = select_ref(P[b], L[b], T[b], case.max_parents, case.forbidden, case.min_delta) if k < case.max_steps else None
            if mv is None:
                done[b] = True
                assert steps[b] == r.steps[b], (case.name, b, k)
                assert r.converged[b] == (1 if k < case.max_steps else 0)
                continue
            assert int(r.codes[b, k]) == mv[0], (case.name, b, k, int(r.codes[b, k]), mv)
            assert np.float64(r.deltas[b, k]).tobytes() == np.float64(mv[1]).tobytes(), (case.name, b, k)
            newP, op, v, u = apply_move(P[b], mv[0])
            P[b] = np.asarray(newP, U64)
            L[b, v] = T[b, v, u]
            wl[2 * b] = v
            if op == 2:
                L[b, u] = T[b, u, v]
                wl[2 * b + 1] = u
            steps[b] += 1
        if done.all():
            break
        if full:
            L, T, _ = drv.toggle(P)
        else:
            drv.toggle(P, worklist=wl, out=(L, T))
    assert done.all()
    assert np.array_equal(P, r.parents) and np.array_equal(steps, r.steps)
    Lf, Tf, _ = drv.toggle(P)
    assert L.tobytes() == Lf.tobytes() and T.tobytes() == Tf.tobytes()
    assert not any(has_cycle(P[b]) for b in range(B))
    out, _, _ = drv.local(P)
    assert out.tobytes() == r.scores.tobytes()
    assert all(totals[b][-1] == out[b] for b in range(B))
    for b in range(B):
        assert all(x < y for x, y in zip(totals[b], totals[b][1:])), (case.name, b, "scores not strictly increasing")
    return totals


HAND_N = 5


def hand_tables(P, gains):
    """L = 0 and T = -1 everywhere (every move loses) except the given {(v, u): value} cells: with L = 0 a cell is the
    move's delta (a reversal adds T[u][v])."""
    L = np.zeros((1, HAND_N))
    T = np.full((1, HAND_N, HAND_N), -1.0)
    for (v, u), x in gains.items():
        T[0, v, u] = x
    for v in range(HAND_N):
        T[0, v, v] = np.nan
    return np.ascontiguousarray(P, U64), L, T


def check_hand_made(drv):
    a, b, c = 0, 1, 2
    n = HAND_N
    # chain a -> b -> c plus a -> c: reversing a -> c would close c -> a -> b -> c and is illegal although it gains most;
    # reversing b -> c is legal
    P = sc.masks_of(n, {b: [a], c: [a, b]})
    P, L, T = hand_tables(P, {(c, a): 5.0, (a, c): 5.0, (c, b): 2.0, (b, c): 1.5})
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    # legal candidates: delete a -> c (5.0, code n^2 + c n + a), reverse b -> c (3.5); reverse a -> c (10.0) is barred
    assert select_ref(P[0], L[0], T[0]) == (n * n + c * n + a, 5.0)
    assert int(tr[0, 0, 0]) == n * n + c * n + a and act == 1 and st[0] == 1 and list(wl) == [c, -1]
    assert int(P1[0, c]) == 1 << b and L1[0, c] == 5.0
    T[0, c, a] = -1.0                                    # now deleting a -> c loses: the legal reversal of b -> c wins
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert select_ref(P[0], L[0], T[0]) == (2 * n * n + c * n + b, 3.5)
    assert int(tr[0, 0, 0]) == 2 * n * n + c * n + b and tr[0, 0, 1:].view(np.float64)[0] == 3.5
    assert int(P1[0, c]) == 1 << a and int(P1[0, b]) == (1 << a) | (1 << c) and sorted(wl) == [b, c]
    assert L1[0, c] == 2.0 and L1[0, b] == 1.5
    # an add that would close a 3-cycle: a -> b -> c, adding c -> a gains most and is illegal; adding a -> c is taken
    P = sc.masks_of(n, {b: [a], c: [b]})
    P, L, T = hand_tables(P, {(a, c): 9.0, (c, a): 1.0})
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert select_ref(P[0], L[0], T[0]) == (c * n + a, 1.0)
    assert int(tr[0, 0, 0]) == c * n + a and int(P1[0, c]) == (1 << a) | (1 << b) and int(P1[0, a]) == 0
    # nothing gains: converged, untouched, both slots cleared
    P, L, T = hand_tables(P, {})
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert np.array_equal(P1, P) and cv[0] == 1 and st[0] == 0 and act == 0 and list(wl) == [-1, -1] and fl[0] == 0
    # an exact tie goes to the lowest code: add 4 -> 3 (code 3 n + 4) before add 3 -> 4 (4 n + 3) before the delete (n^2 + ...)
    P = sc.masks_of(n, {b: [a]})
    P, L, T = hand_tables(P, {(4, 3): 2.0, (b, a): 2.0, (3, 4): 2.0})
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert select_ref(P[0], L[0], T[0])[0] == 3 * n + 4 == int(tr[0, 0, 0])
    # a gain equal to min_delta is not taken (strict)
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T, min_delta=2.0)
    assert cv[0] == 1 and act == 0 and select_ref(P[0], L[0], T[0], min_delta=2.0) is None
    # a start with a cycle: flag 1, untouched; an L cell that is NaN: flag 2, untouched
    P = sc.masks_of(n, {a: [c], b: [a], c: [b]})
    P, L, T = hand_tables(P, {(4, 3): 2.0})
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert fl[0] == 1 and np.array_equal(P1, P) and st[0] == 0 and cv[0] == 0 and act == 0 and list(wl) == [-1, -1]
    P, L, T = hand_tables(sc.masks_of(n, {b: [a]}), {(4, 3): 2.0})
    L[0, 2] = np.nan
    P1, L1, wl, st, cv, fl, tr, act = drv.step(P, L, T)
    assert fl[0] == 2 and np.array_equal(P1, P) and st[0] == 0 and act == 0


# ---------------------------------------------------------------------------------------------------------------------
# Layer 3: the device's trajectory against the float64 oracle
# ---------------------------------------------------------------------------------------------------------------------
def check_against_oracle(case, typ, arg, r):
    """Follows the device's trace (a second trajectory would fork at near-ties).  Returns the worst margin used / tau."""
    B, n = case.starts.shape
    worst = 0.0

    def tabs(op, v, u, aL, aT):
        return max([aT[v, u], aL[v]] + ([aT[u, v], aL[u]] if op == 2 else []))

    for b in range(B):
        P = [int(x) for x in case.starts[b]]
        for k in range(int(r.steps[b]) + 1):
            L, T, aL, aT = _neighbourhood(case, P, typ, arg)
            moves = legal_moves(P, case.max_parents, case.forbidden)
            scored = [(move_delta(op, v, u, L, T), code, op, v, u) for code, op, v, u in moves]
            top = max(scored) if scored else None
            if k == int(r.steps[b]):
                if r.converged[b] and top is not None:
                    tau = TAU_RTOL * tabs(top[2], top[3], top[4], aL, aT)
                    assert top[0] <= case.min_delta + tau, (case.name, typ, b, "converged below a gaining move", top)
                    if top[0] > case.min_delta:
                        worst = max(worst, (top[0] - case.min_delta) / tau)
                break
            code = int(r.codes[b, k])
            mine = next(s for s in scored if s[1] == code)                  # StopIteration: the device took an illegal move
            tau = TAU_RTOL * max(tabs(mine[2], mine[3], mine[4], aL, aT), tabs(top[2], top[3], top[4], aL, aT))
            assert mine[0] >= top[0] - tau and mine[0] > case.min_delta - tau, (case.name, typ, b, k, mine, top, tau)
            worst = max(worst, (top[0] - mine[0]) / tau, (case.min_delta - mine[0]) / tau)
            P = apply_move(P, code)[0]
        assert P == [int(x) for x in r.parents[b]] and not has_cycle(P)
    return worst


def asia_known_score(typ, arg):
    case = hc_case("asia")
    return math.fsum(oracle_local(case.data, case.card, v, ps, typ, arg, "asia")[0] for v, ps in
                     {0: [], **ASIA_KNOWN}.items()), \
        max(oracle_local(case.data, case.card, v, ps, typ, arg, "asia")[1] for v, ps in {0: [], **ASIA_KNOWN}.items())


# ---------------------------------------------------------------------------------------------------------------------
# Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def check_argument_refusals(lib, ptr):
    be, p = sc.EmuBackend(lib), ptr                          # nothing is moved: dummy pointers as they are, the null stream
    tog = lambda B=4, n=8, S=100, code=2, arg=NAN, lb=4 * 8 * 8, tb=4 * 8 * 8 * 8, d=p, st=p: call_rc(
        be, "dvs_bn_toggle_scores", batch=B, n_vars=n, n_samples=S, data=d, card=p, parents=p, score_type=code, score_arg=arg,
        worklist=None, local=p, local_bytes=lb, toggles=p, toggles_bytes=tb, status=st)
    last = lambda: lib.dvs_last_error().decode()
    for code in (-1, 7, 100):
        assert tog(code=code) == 12 and "score_type" in last()
    assert tog(code=bn.TYPE_CODE["bde"], arg=0.0) == 13 and "iss" in last()
    assert tog(code=bn.TYPE_CODE["aic"], arg=-1.0) == 13 and "k must" in last()
    assert tog(code=bn.TYPE_CODE["k2"], arg=1.0) == 13
    assert tog(lb=4 * 8 * 8 - 1) == 14 and "local_bytes" in last() and str(4 * 8 * 8) in last()
    assert tog(tb=4 * 8 * 8 * 8 - 1) == 14 and "toggles_bytes" in last() and str(4 * 8 * 8 * 8) in last()
    assert tog(B=0) == 2 and tog(S=0) == 2 and tog(n=0) == 3 and tog(n=49) == 3
    assert tog(B=1 << 20, n=48, lb=1 << 40, tb=1 << 40) == 2
    assert tog(d=None) == 10 and tog(st=None) == 10
    hc = lambda B=4, n=8, tb=4 * 8 * 8 * 8, md=0.0, cap=10, tr=p, trb=4 * 10 * 16, P=p, act=p: call_rc(
        be, "dvs_hc_step", batch=B, n_vars=n, parents=P, local=p, toggles=p, toggles_bytes=tb, max_parents=0, min_delta=md,
        forbidden=None, step_cap=cap, worklist=p, steps=p, converged=p, flags=p, trace=tr, trace_bytes=trb, active=act)
    assert hc(tb=4 * 8 * 8 * 8 - 1) == 14 and "toggles_bytes" in last() and str(4 * 8 * 8 * 8) in last()
    assert hc(trb=4 * 10 * 16 - 1) == 14 and "trace_bytes" in last() and str(4 * 10 * 16) in last()
    assert hc(md=NAN) == 13 and "min_delta" in last()
    assert hc(cap=0) == 13 and "step_cap" in last()
    assert hc(B=0) == 2 and hc(n=0) == 3 and hc(n=49) == 3
    assert hc(P=None) == 10 and hc(act=None) == 10
