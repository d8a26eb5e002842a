"""TEST HELPER: cases, references and the checks themselves for tabu search and random restarts (csrc/dvs_tabu.h:
dvs_tabu_step, dvs_hc_perturb; dags_vae_search_amd/tabu.py), written once and run by tests/test_emu_tabu.py (emulator build)
and tests/test_gpu_tabu.py (device).  Move rules, oracle scores, cases and drivers are those of tests/hillclimb_corpus.py —
imported, not copied; the drivers are subclassed for the two new calls.

References
  tabu_select_ref  the rules of include/dvs.h (dvs_tabu_step) restated on Python ints and numpy float64: the ring as a list of
                   structures compared row for row with what each legal move produces (not the kernel's reduction of the ring
                   to barred codes), the push slot, the left-to-right total, stall / best bookkeeping.  Exact: no tolerance.
  perturb_ref      move number (r M) >> 32 of hillclimb_corpus.legal_moves without the NaN-cell moves, r from oracle/rng.py.
  oracle_local     hillclimb_corpus' float64 scores that share no code with the kernel.
There is no bnlearn run to pin against (R is not available to this suite): parity with bnlearn's `tabu` rests on the rules,
DESIGN.md §15.

Tolerance of the oracle layer: hillclimb_corpus' rule, 1e-12 * T_abs per local score.  Two deltas hold up to eight local
scores, tau = TAU_RTOL * max T_abs over their families as there; two totals hold 2 n local scores, so
    tau_total = (n / 2) * TAU_RTOL * max T_abs over the families of both structures.
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from oracle import rng as orng
from tests import scoring_corpus as sc
from tests.abi_cases import call, call_rc
from tests.hillclimb_corpus import (HAND_N, MIN_DELTA, NAN, TAU_RTOL, U64, Driver, GpuDriver, _neighbourhood, apply_move,
                                    closure, hand_tables, has_cycle, hc_case, legal_moves, move_delta, oracle_local, select_ref)

INF = float("inf")
SITE_PERTURB = 400


# ---------------------------------------------------------------------------------------------------------------------
# tabu_select_ref: the rules
# ---------------------------------------------------------------------------------------------------------------------
def total(L):
    """S = L[0] + L[1] + ... left to right in float64"""
    s = np.float64(0.0)
    for x in L:
        s = s + np.float64(x)
    return s


class TabuState:
    """what dvs_tabu_step keeps per structure between calls, as the caller initialises it"""

    def __init__(self, n, tabu_len, ring=None):
        self.tabu_len = tabu_len
        self.ring = np.zeros((tabu_len, n), U64) if ring is None else np.array(ring, U64)
        self.visited, self.stall, self.converged, self.steps = 0, 0, 0, 0
        self.best_score = np.float64(-INF)
        self.best_parents = np.zeros(n, U64)


def tabu_select_ref(P, L, T, st, max_stall, max_parents=None, forbidden=None, min_delta=0.0):
    """One dvs_tabu_step on one structure that is neither flagged nor converged: updates `st`, returns (code, delta, new P,
    new L) or None (no legal move that is not tabu)."""
    P = [int(x) for x in P]
    L = np.array(L, np.float64)
    if st.visited == 0:
        st.best_score, st.best_parents = total(L), np.array(P, U64)
    st.ring[st.visited % st.tabu_len] = np.array(P, U64)
    st.visited += 1
    entries = [[int(x) for x in st.ring[e]] for e in range(min(st.visited, st.tabu_len))]
    best = None
    for code, op, v, u in legal_moves(P, max_parents, forbidden):
        d = move_delta(op, v, u, L, T)
        if np.isnan(d) or apply_move(P, code)[0] in entries:
            continue
        if best is None or d > best[1]:                     # code order: a tie keeps the lower code
            best = (code, d)
    if best is None:
        st.converged = 1
        return None
    Q, op, v, u = apply_move(P, best[0])
    L[v] = T[v, u]
    if op == 2:
        L[u] = T[u, v]
    s_new = total(L)
    if s_new - st.best_score > min_delta:
        st.best_score, st.best_parents, st.stall = s_new, np.array(Q, U64), 0
    else:
        st.stall += 1
        if st.stall >= max_stall:
            st.converged = 1
    st.steps += 1
    return best[0], best[1], Q, L


# ---------------------------------------------------------------------------------------------------------------------
# Drivers: the two new calls through the raw C ABI on the driver's own back end (numpy in place on the emulator, torch
# tensors on the device), and the launch sequence of tabu.tabu_search with everything the kernel keeps handed back
# ---------------------------------------------------------------------------------------------------------------------
TabuClimb = namedtuple("TabuClimb", "parents best_parents best_score steps converged flags codes deltas stall visited ring")


class TabuDriver(Driver):
    def _tabu_args(self, P, L, T, worklist_fill, step_cap, tabu_len, max_stall, max_parents, forbidden, min_delta, ring=None,
                   visited=0, stall=0, best_score=-INF, best_parents=None, steps=0):
        """the named arguments of one dvs_tabu_step on fresh handles: those of dvs_hc_step and the state; `active` is the caller's"""
        be = self.be
        B, n = np.shape(P)
        full = lambda x, dt: be.put(np.full(B, x, dt) if np.isscalar(x) else np.array(x, dt))
        return dict(
            self._step_args(P, L, T, max_parents, forbidden, min_delta, step_cap, worklist_fill), steps=full(steps, np.int32),
            tabu_len=tabu_len, ring_bytes=B * tabu_len * n * 8, max_stall=max_stall, best_bytes=B * n * 8,
            ring=be.put(np.zeros((B, tabu_len, n), U64) if ring is None else np.array(ring, U64).reshape(B, tabu_len, n)),
            visited=full(visited, np.int32), stall=full(stall, np.int32), best_score=full(best_score, np.float64),
            best_parents=be.put(np.zeros((B, n), U64) if best_parents is None else np.array(best_parents, U64).reshape(B, n)))

    def tabu_step(self, P, L, T, *, tabu_len, max_stall, ring=None, visited=0, stall=0, best_score=-INF, best_parents=None,
                  max_parents=None, forbidden=None, min_delta=0.0, step_cap=4, steps=0):
        """one dvs_tabu_step on given tables and state -> everything it writes"""
        be = self.be
        a = self._tabu_args(P, L, T, 5, step_cap, tabu_len, max_stall, max_parents, forbidden, min_delta, ring, visited, stall,
                            best_score, best_parents, steps)
        a["active"] = be.put(np.zeros(1, np.int32))
        call(be, "dvs_tabu_step", **a)
        g = lambda k: be.get(a[k]).copy()
        return SimpleNamespace(P=g("parents"), L=g("local"), T=g("toggles"), wl=g("worklist"), **{k: g(k) for k in (
            "steps", "converged", "flags", "trace", "active", "ring", "visited", "stall", "best_score", "best_parents")})

    def perturb(self, P, L, T, seed, draw_index, max_parents=None, forbidden=None, flags=None):
        """one dvs_hc_perturb -> (P, L, worklist, flags)"""
        be = self.be
        P, L, T = np.array(P, U64), np.array(L, np.float64), np.ascontiguousarray(T, np.float64)
        B, n = P.shape
        hP, hL, hT, wl = be.put(P), be.put(L), be.put(T), be.put(np.full(2 * B, 5, np.int32))
        fl = be.put(np.zeros(B, np.int32) if flags is None else np.array(flags, np.int32))
        forb = None if forbidden is None else be.put(np.ascontiguousarray(forbidden, U64))
        call(be, "dvs_hc_perturb", batch=B, n_vars=n, parents=hP, local=hL, toggles=hT, toggles_bytes=T.nbytes,
             max_parents=max_parents or 0, forbidden=forb, worklist=wl, flags=fl, seed=seed, draw_index=draw_index)
        g = lambda x: be.get(x).copy()
        return g(hP), g(hL), g(wl), g(fl)

    def tabu_climb(self, starts, max_steps, tabu_len, max_stall, max_parents=None, forbidden=None, min_delta=0.0, check_every=8):
        """the launch sequence of tabu.tabu_search (restarts = 0) on the raw ABI"""
        be = self.be
        B, n = np.shape(starts)
        a = self._tabu_args(starts, np.full((B, n), -7.0), np.full((B, n, n), -7.0), -1, max_steps, tabu_len, max_stall,
                            max_parents, forbidden, min_delta)
        act, status = [be.put(np.zeros(1, np.int32)) for _ in range(max_steps)], be.put(np.zeros(1, np.int32))
        self._toggle_on(B, a["parents"], None, a["local"], a["toggles"], status)
        for t in range(max_steps):
            call(be, "dvs_tabu_step", **a, active=act[t])
            self._toggle_on(B, a["parents"], a["worklist"], a["local"], a["toggles"], status)
            if (t + 1) % check_every == 0 and int(be.get(act[t])[0]) == 0:
                break
        g = lambda k: be.get(a[k]).copy()
        tr = g("trace")
        return TabuClimb(g("parents"), g("best_parents"), g("best_score"), g("steps"), g("converged"), g("flags"), tr[..., 0].copy(),
                         tr[..., 1].copy().view(np.float64), g("stall"), g("visited"), g("ring"))


class GpuTabuDriver(TabuDriver, GpuDriver):
    def search(self, starts, **kw):
        """the package's own tabu_search on the same evaluator -> TabuResult"""
        from dags_vae_search_amd import tabu_search
        if kw.get("forbidden") is not None:
            kw["forbidden"] = self._t(kw["forbidden"])
        return tabu_search(self.ev, self._t(starts), **kw)

    def tabu_climb(self, starts, max_steps, tabu_len, max_stall, max_parents=None, forbidden=None, min_delta=0.0, check_every=8):
        """the raw launch sequence, and tabu_search itself: equal bytes wherever the result has the field"""
        r = super().tabu_climb(starts, max_steps, tabu_len, max_stall, max_parents, forbidden, min_delta, check_every)
        s = self.search(starts, max_steps=max_steps, tabu=tabu_len, max_tabu=max_stall, max_parents=max_parents,
                        forbidden=forbidden, min_delta=min_delta, check_every=check_every, trace=True)
        c = lambda x: x.cpu().numpy()
        assert c(s.parents).view(U64).tobytes() == r.best_parents.tobytes()
        assert c(s.last_parents).view(U64).tobytes() == r.parents.tobytes()
        assert c(s.scores).tobytes() == r.best_score.tobytes()
        assert c(s.steps).tobytes() == r.steps.tobytes() and c(s.converged).tobytes() == r.converged.tobytes()
        assert c(s.trace[0]).tobytes() == r.codes.tobytes() and c(s.trace[1]).tobytes() == r.deltas.tobytes()
        assert s.rounds == 0 and not c(s.flags).any()
        return r


# ---------------------------------------------------------------------------------------------------------------------
# Cases: the hill-climb cases with a ring length, a stall limit and a step budget a few tens beyond the greedy length
# ---------------------------------------------------------------------------------------------------------------------
TabuCase = namedtuple("TabuCase", "name hc typ arg starts tabu max_tabu max_steps cut")
TABU_CASES = ("asia_bic", "asia_bde", "sachs", "syn17", "syn48", "asia_cut")


@functools.lru_cache(maxsize=None)
def tabu_case(name):
    mk = lambda hcname, typ, arg, rows, tabu, max_tabu, max_steps, cut=False: TabuCase(
        name, hc_case(hcname), typ, arg, hc_case(hcname).starts[rows], tabu, max_tabu, max_steps, cut)
    return {
        "asia_bic": lambda: mk("asia", "bic", None, slice(0, 33), 10, 10, 40),
        "asia_bde": lambda: mk("asia", "bde", 10.0, slice(0, 9), 3, 5, 40),
        "sachs": lambda: mk("sachs", "bic", None, slice(0, 8), 10, 10, 80),
        "syn17": lambda: mk("syn17", "bic", None, slice(0, 4), 1, 2, 70),
        # lanes >= 32; cut by max_steps well before the climb ends, so the emulator stays within seconds
        "syn48": lambda: mk("syn48", "bic", None, slice(0, 4), 3, 3, 10, True),
        "asia_cut": lambda: mk("asia", "bic", None, slice(0, 5), 10, 10, 3, True),
    }[name]()


@functools.lru_cache(maxsize=None)
def _tabu_cached(make_driver, name):
    tc = tabu_case(name)
    drv = make_driver(tc.hc.name, tc.typ, tc.arg)
    return drv, drv.tabu_climb(tc.starts, tc.max_steps, tc.tabu, tc.max_tabu, tc.hc.max_parents, tc.hc.forbidden, tc.hc.min_delta)


# ---------------------------------------------------------------------------------------------------------------------
# 1. The step kernel, exact
# ---------------------------------------------------------------------------------------------------------------------
FULL_REPLAY_CELLS = 6000


def check_tabu_replay(drv, tc, r):
    """Replays the trace: at every step the test's own table of the masks so far, its own ring and tabu_select_ref give
    exactly the traced (code, delta bits); at the end steps, converged, stall, visited, the best and the ring match, and the
    best score is dvs_bn_scores of the best structure, bitwise.  Tables as in hillclimb_corpus.check_replay.  Returns the
    number of moves that lowered the score."""
    case = tc.hc
    B, n = tc.starts.shape
    P = tc.starts.copy()
    full = B * n * n <= FULL_REPLAY_CELLS
    L, T, _ = drv.toggle(P)
    states = [TabuState(n, tc.tabu) for _ in range(B)]
    downhill = 0
    for k in range(tc.max_steps):
        wl = np.full(2 * B, -1, np.int32)
        for b, st in enumerate(states):
            if st.converged:
                continue
            mv = tabu_select_ref(P[b], L[b], T[b], st, tc.max_tabu, case.max_parents, case.forbidden, case.min_delta)
            if mv is None:
                continue
            code, d, Q, Lb = mv
            assert int(r.codes[b, k]) == code, (tc.name, b, k, int(r.codes[b, k]), mv[:2])
            assert np.float64(r.deltas[b, k]).tobytes() == np.float64(d).tobytes(), (tc.name, b, k)
            downhill += d < 0
            _, op, v, u = apply_move(P[b], code)
            P[b], L[b] = np.asarray(Q, U64), Lb
            wl[2 * b] = v
            if op == 2:
                wl[2 * b + 1] = u
        if full:
            L, T, _ = drv.toggle(P)
        else:
            drv.toggle(P, worklist=wl, out=(L, T))
        if all(st.converged for st in states):
            break
    Lf, Tf, _ = drv.toggle(P)
    assert L.tobytes() == Lf.tobytes() and T.tobytes() == Tf.tobytes()
    col = lambda f, dt: np.array([getattr(st, f) for st in states], dt)
    assert np.array_equal(P, r.parents) and not r.flags.any()
    assert np.array_equal(col("steps", np.int32), r.steps) and np.array_equal(col("converged", np.int32), r.converged)
    assert np.array_equal(col("stall", np.int32), r.stall) and np.array_equal(col("visited", np.int32), r.visited)
    assert col("best_score", np.float64).tobytes() == r.best_score.tobytes()
    assert np.stack([st.best_parents for st in states]).tobytes() == r.best_parents.tobytes()
    assert np.stack([st.ring for st in states]).tobytes() == r.ring.tobytes()
    assert not any(has_cycle(x) for x in r.parents) and not any(has_cycle(x) for x in r.best_parents)
    out, _, _ = drv.local(r.best_parents)
    assert out.tobytes() == r.best_score.tobytes()
    if tc.cut:
        assert not r.converged.any() and (r.steps == tc.max_steps).all()
    else:
        assert r.converged.all()
    return int(downhill)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Hand-made, n = 5
# ---------------------------------------------------------------------------------------------------------------------
def check_tabu_hand_made(drv):
    a, b, c = 0, 1, 2
    n = HAND_N
    m = lambda d: sc.masks_of(n, d)
    add, dele, rev = (lambda v, u: v * n + u), (lambda v, u: n * n + v * n + u), (lambda v, u: 2 * n * n + v * n + u)
    step = lambda P, L, T, **kw: drv.tabu_step(P, L, T, **{"tabu_len": 3, "max_stall": 5, **kw})

    def ref(P, L, T, ring, visited, max_stall=5, tabu_len=3, best_score=-INF, stall=0, **kw):
        st = TabuState(n, tabu_len, ring)
        st.visited, st.best_score, st.stall = visited, np.float64(best_score), stall
        return tabu_select_ref(P[0], L[0], T[0], st, max_stall, **kw), st

    def ring3(*entries, tabu_len=3):
        r = np.zeros((tabu_len, n), U64)
        for i, e in enumerate(entries):
            r[i] = e
        return r

    # a. the ring holds current + edge 3 -> 4: the top-gaining add is tabu, the next best (add 4 -> 3) is taken
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): 5.0, (3, 4): 2.0})
    ring = ring3(m({b: [a], 4: [3]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0)
    mv, st = ref(P, L, T, ring, 1, best_score=0.0)
    assert mv[0] == add(3, 4) == int(o.trace[0, 0, 0]) and o.trace[0, 0, 1:].view(np.float64)[0] == 2.0
    assert int(o.P[0, 3]) == 1 << 4 and list(o.wl) == [3, -1] and o.visited[0] == 2 and o.active[0] == 1
    assert o.ring.tobytes() == st.ring.tobytes() and o.ring[0, 1].tolist() == P[0].tolist()      # pushed into slot 1
    assert o.best_score[0] == 2.0 and o.best_parents.tobytes() == o.P.tobytes() and o.stall[0] == 0
    assert int(step(P, L, T, visited=0).trace[0, 0, 0]) == add(4, 3)                    # without the entry: the top add
    # b. a tabu delete: a -> b -> c, the ring holds the structure without a -> b; the next best is an add
    P, L, T = hand_tables(m({b: [a], c: [b]}), {(b, a): 5.0, (4, 3): 4.5})
    ring = ring3(m({c: [b]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0)
    assert ref(P, L, T, ring, 1, best_score=0.0)[0][0] == add(4, 3) == int(o.trace[0, 0, 0])
    assert int(step(P, L, T, visited=0).trace[0, 0, 0]) == dele(b, a)
    #    a tabu reversal: the ring holds the structure with a -> b reversed; the delete (3.0 against 6.0) is taken
    P, L, T = hand_tables(m({b: [a], c: [b]}), {(b, a): 3.0, (a, b): 3.0})
    ring = ring3(m({a: [b], c: [b]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0)
    assert ref(P, L, T, ring, 1, best_score=0.0)[0][0] == dele(b, a) == int(o.trace[0, 0, 0])
    assert int(step(P, L, T, visited=0).trace[0, 0, 0]) == rev(b, a)
    #    and with the child below the parent (c -> b): the other of the two differing rows holds the edge
    P, L, T = hand_tables(m({b: [c]}), {(b, c): 3.0, (c, b): 3.0})
    ring = ring3(m({c: [b]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0)
    assert ref(P, L, T, ring, 1, best_score=0.0)[0][0] == dele(b, c) == int(o.trace[0, 0, 0])
    assert int(step(P, L, T, visited=0).trace[0, 0, 0]) == rev(b, c)
    # c. entries that differ by two adds bar nothing: in two rows, in one row, and as the 2-cycle 3 <-> 4
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): 5.0, (3, 4): 2.0})
    ring = ring3(m({b: [a], 4: [3], 3: [c]})[0], m({b: [a], 4: [3, c]})[0], m({b: [a], 4: [3], 3: [4]})[0])
    o = step(P, L, T, ring=ring, visited=3, best_score=0.0)
    assert ref(P, L, T, ring, 3, best_score=0.0)[0][0] == add(4, 3) == int(o.trace[0, 0, 0])
    # d. bytes beyond min(visited, tabu_len) bar nothing: slot 2 holds current + 3 -> 4, one structure was pushed so far
    ring = ring3(m({c: [a]})[0], m({})[0], m({b: [a], 4: [3]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0)
    mv, st = ref(P, L, T, ring, 1, best_score=0.0)
    assert mv[0] == add(4, 3) == int(o.trace[0, 0, 0]) and o.ring.tobytes() == st.ring.tobytes()
    assert o.ring[0, 2].tolist() == ring[2].tolist() and o.ring[0, 1].tolist() == P[0].tolist()
    # e. every move loses: the least-losing one is taken, stall becomes 1; with max_stall = 1 that converges, and the move
    #    and the worklist are still written
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): -0.25})
    for max_stall in (2, 1):
        o = step(P, L, T, visited=0, max_stall=max_stall)
        mv, st = ref(P, L, T, None, 0, max_stall=max_stall)
        assert mv[0] == add(4, 3) == int(o.trace[0, 0, 0]) and o.trace[0, 0, 1:].view(np.float64)[0] == -0.25
        assert o.stall[0] == 1 == st.stall and o.converged[0] == st.converged == (1 if max_stall == 1 else 0)
        assert int(o.P[0, 4]) == 1 << 3 and o.L[0, 4] == -0.25 and list(o.wl) == [4, -1] and o.steps[0] == 1 and o.active[0] == 1
        assert o.best_score[0] == 0.0 and o.best_parents.tobytes() == P.tobytes()       # the first call's: the start
    # f. all legal moves tabu: only 3 -> 4 is not forbidden, and the ring holds it: converged, untouched
    forb = np.full(n, (1 << n) - 1, U64)
    forb[4] ^= U64(1 << 3)
    P, L, T = hand_tables(m({}), {(4, 3): 5.0})
    ring = ring3(m({4: [3]})[0])
    o = step(P, L, T, ring=ring, visited=1, best_score=0.0, forbidden=forb)
    mv, st = ref(P, L, T, ring, 1, best_score=0.0, forbidden=forb)
    assert mv is None and st.converged == 1 == o.converged[0] and o.P.tobytes() == P.tobytes() and o.L.tobytes() == L.tobytes()
    assert list(o.wl) == [-1, -1] and o.steps[0] == 0 and o.active[0] == 0 and o.visited[0] == 2 and o.stall[0] == 0
    assert int(step(P, L, T, visited=0, forbidden=forb).trace[0, 0, 0]) == add(4, 3)
    # g. a gain equal to min_delta: the move is taken, the best is not updated (strict)
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): 2.0})
    o = step(P, L, T, visited=0, min_delta=2.0)
    assert int(o.trace[0, 0, 0]) == add(4, 3) and o.best_score[0] == 0.0 and o.best_parents.tobytes() == P.tobytes()
    assert o.stall[0] == 1 and o.converged[0] == 0 and int(o.P[0, 4]) == 1 << 3
    o = step(P, L, T, visited=0, min_delta=1.5)
    assert o.best_score[0] == 2.0 and o.best_parents.tobytes() == o.P.tobytes() and o.stall[0] == 0
    # h. the ring wraps: A = {a -> b}, reversed to B = {b -> a}, deleted to C = {}; with tabu_len = 2 the third push
    #    overwrites A in slot 0 and adding a -> b is legal again (b -> a, which gains more, leads to B: still barred);
    #    with tabu_len = 3 A is still there and both are barred
    for tabu_len, third in ((2, add(b, a)), (3, add(4, 3))):
        kw = dict(tabu_len=tabu_len, max_stall=9)
        P, L, T = hand_tables(m({b: [a]}), {(b, a): 3.0, (a, b): 3.0})
        o = drv.tabu_step(P, L, T, visited=0, **kw)
        assert int(o.trace[0, 0, 0]) == rev(b, a) and o.P[0].tolist() == m({a: [b]})[0].tolist()
        carry = lambda o: dict(ring=o.ring, visited=o.visited, stall=o.stall, best_score=o.best_score, best_parents=o.best_parents)
        P, L, T = hand_tables(o.P, {(a, b): 1.0})
        o = drv.tabu_step(P, L, T, **carry(o), **kw)
        assert int(o.trace[0, 0, 0]) == dele(a, b) and not o.P.any() and o.visited[0] == 2
        P, L, T = hand_tables(o.P, {(b, a): 5.0, (a, b): 6.0, (4, 3): 0.5})
        ring_before = o.ring.copy()
        o = drv.tabu_step(P, L, T, **carry(o), **kw)
        assert int(o.trace[0, 0, 0]) == third and o.visited[0] == 3
        st = TabuState(n, tabu_len, ring_before[0])
        st.visited, st.best_score = 2, np.float64(6.0)
        assert tabu_select_ref(P[0], L[0], T[0], st, 9)[0] == third and o.ring[0].tobytes() == st.ring.tobytes()
        assert o.ring[0, 2 % tabu_len].tolist() == P[0].tolist()
    # flags as dvs_hc_step: a cycle, a NaN local score; frozen before anything is pushed
    P, L, T = hand_tables(m({a: [c], b: [a], c: [b]}), {(4, 3): 2.0})
    o = step(P, L, T, visited=0)
    assert o.flags[0] == 1 and o.P.tobytes() == P.tobytes() and o.visited[0] == 0 and list(o.wl) == [-1, -1] and o.active[0] == 0
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): 2.0})
    L[0, 2] = np.nan
    o = step(P, L, T, visited=0)
    assert o.flags[0] == 2 and o.P.tobytes() == P.tobytes() and o.visited[0] == 0 and o.best_score[0] == -INF
    # left alone: at the step cap
    P, L, T = hand_tables(m({b: [a]}), {(4, 3): 2.0})
    o = step(P, L, T, visited=0, steps=4, step_cap=4)
    assert o.P.tobytes() == P.tobytes() and list(o.wl) == [-1, -1] and o.visited[0] == 0 and o.active[0] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. Tabu does something greedy cannot: the oracle's own runs, then the device along its own trace
# ---------------------------------------------------------------------------------------------------------------------
ESCAPE = {"asia_bic": (1, 8), "sachs": (0, 4)}              # rows of the case's starts, picked on the CPU for the reference alone


def _tau_total(case, typ, arg, *structures):
    n = len(structures[0])
    t = max(oracle_local(case.data, case.card, v, sc.mask_bits(int(P[v])), typ, arg, case.key)[1] for P in structures
            for v in range(n))
    return 0.5 * n * TAU_RTOL * t


@functools.lru_cache(maxsize=None)
def reference_tabu(name):
    """tabu_select_ref and select_ref on oracle scores from the ESCAPE rows: {row: (greedy final, tabu best, its score
    gain)}.  Asserts what the case is there to show: the tabu best exceeds the greedy final by more than tau_total, and no
    structure is stood on twice within `tabu` steps."""
    tc = tabu_case(name)
    case = tc.hc
    out = {}
    for b in ESCAPE[name]:
        P = [int(x) for x in tc.starts[b]]
        G = list(P)
        while True:
            L, T, _, _ = _neighbourhood(case, G, tc.typ, tc.arg)
            mv = select_ref(G, L, T, case.max_parents, case.forbidden, case.min_delta)
            if mv is None:
                break
            G = apply_move(G, mv[0])[0]
        st = TabuState(len(P), tc.tabu)
        path = []
        while not st.converged:
            assert len(path) < tc.max_steps, (name, b, "max_steps too small for the reference to stop by itself")
            path.append(list(P))
            L, T, _, _ = _neighbourhood(case, P, tc.typ, tc.arg)
            mv = tabu_select_ref(P, L, T, st, tc.max_tabu, case.max_parents, case.forbidden, case.min_delta)
            if mv is not None:
                P = mv[2]
        for i, X in enumerate(path):
            assert X not in path[max(0, i - tc.tabu):i], (name, b, i, "a structure was revisited within the tabu length")
        score = lambda X: sum(oracle_local(case.data, case.card, v, sc.mask_bits(X[v]), tc.typ, tc.arg, case.key)[0]
                              for v in range(len(X)))
        best = [int(x) for x in st.best_parents]
        gain = score(best) - score(G)
        assert gain > _tau_total(case, tc.typ, tc.arg, best, G), (name, b, gain, "tabu finds nothing greedy does not")
        out[b] = (G, best, gain)
    return out


def check_tabu_against_oracle(tc, r, greedy_scores):
    """Follows the device's trace: every move taken is within tau of the oracle's best legal move that is not tabu for the
    device's own ring (the structures it stood on: exact, no scores involved), and on the ESCAPE rows the device's best
    beats the device's greedy final (hill-climb result of the same rows) by more than tau_total.  Returns the worst margin
    used / tau."""
    case = tc.hc
    worst = 0.0
    tabs = lambda op, v, u, aL, aT: max([aT[v, u], aL[v]] + ([aT[u, v], aL[u]] if op == 2 else []))
    for b in ESCAPE[tc.name]:
        P = [int(x) for x in tc.starts[b]]
        path = []
        for k in range(int(r.steps[b])):
            path.append(list(P))
            entries = path[-tc.tabu:]
            L, T, aL, aT = _neighbourhood(case, P, tc.typ, tc.arg)
            scored = [(move_delta(op, v, u, L, T), code, op, v, u) for code, op, v, u in
                      legal_moves(P, case.max_parents, case.forbidden) if apply_move(P, code)[0] not in entries]
            top = max(scored)
            mine = next(s for s in scored if s[1] == int(r.codes[b, k]))    # StopIteration: an illegal or a tabu move
            tau = TAU_RTOL * max(tabs(*mine[2:], aL, aT), tabs(*top[2:], aL, aT))
            assert mine[0] >= top[0] - tau, (tc.name, b, k, mine, top, tau)
            worst = max(worst, (top[0] - mine[0]) / tau)
            P = apply_move(P, mine[1])[0]
        assert P == [int(x) for x in r.parents[b]]
        best = [int(x) for x in r.best_parents[b]]
        assert r.best_score[b] - greedy_scores[b] > _tau_total(case, tc.typ, tc.arg, best), (tc.name, b)
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# 4. Perturb
# ---------------------------------------------------------------------------------------------------------------------
DRAWS = ((0, 0), (7, 1), (0xDEADBEEF12345678, 5), (7, 0xFFFFFFFF))


def perturb_ref(P, T, b, seed, draw_index, max_parents=None, forbidden=None):
    """(code, M) of the move dvs_hc_perturb takes on structure b of a batch, or (None, 0)"""
    moves = [mv for mv in legal_moves(P, max_parents, forbidden)
             if not np.isnan(T[mv[2], mv[3]]) and not (mv[1] == 2 and np.isnan(T[mv[3], mv[2]]))]
    if not moves:
        return None, 0
    r = int(orng.draw(orng.site_key(seed, SITE_PERTURB, b), draw_index))
    return moves[(r * len(moves)) >> 32][0], len(moves)


def check_perturb_one(drv, P, L, T, seed, di, max_parents=None, forbidden=None):
    """one launch against perturb_ref, row by row -> (new P, new L, worklist, the codes taken)"""
    P1, L1, wl, fl = drv.perturb(P, L, T, seed, di, max_parents, forbidden)
    assert not fl.any()
    codes = []
    for b in range(len(P)):
        code, M = perturb_ref(P[b], T[b], b, seed, di, max_parents, forbidden)
        codes.append(code)
        if code is None:
            assert P1[b].tobytes() == np.asarray(P[b], U64).tobytes() and L1[b].tobytes() == L[b].tobytes()
            assert list(wl[2 * b:2 * b + 2]) == [-1, -1]
            continue
        Q, op, v, u = apply_move(P[b], code)
        assert P1[b].tolist() == Q, (b, seed, di, code, M)
        want = np.array(L[b])
        want[v] = T[b, v, u]
        if op == 2:
            want[u] = T[b, u, v]
        assert L1[b].tobytes() == want.tobytes() and list(wl[2 * b:2 * b + 2]) == [v, u if op == 2 else -1]
        assert not has_cycle(P1[b])
    return P1, L1, wl, codes


def check_perturb_case(drv, name):
    """real starts: the move is number (r M) >> 32 of the legal moves; the incremental pass afterwards equals a full one"""
    case = hc_case(name)
    P = case.starts
    L, T, _ = drv.toggle(P)
    taken = {}
    for seed, di in DRAWS:
        P1, L1, wl, taken[seed, di] = check_perturb_one(drv, P, L, T, seed, di, case.max_parents, case.forbidden)
    T1 = T.copy()
    drv.toggle(P1, worklist=wl, out=(L1, T1))
    Lf, Tf, _ = drv.toggle(P1)
    assert L1.tobytes() == Lf.tobytes() and T1.tobytes() == Tf.tobytes()
    return taken


def check_perturb_hand_made(drv):
    n, B = HAND_N, 33
    m = lambda d: sc.masks_of(n, d)

    def run(P1, forbidden=None, max_parents=None, nan=(), want_ops=None):
        P, L, T = hand_tables(P1, {})
        for v, u in nan:
            T[0, v, u] = np.nan
        P, L, T = np.repeat(P, B, 0), np.repeat(L, B, 0), np.repeat(T, B, 0)
        codes = check_perturb_one(drv, P, L, T, 3, 2, max_parents, forbidden)[3]
        M = perturb_ref(P[0], T[0], 0, 3, 2, max_parents, forbidden)[1]
        if want_ops is not None:
            got = [mv[1] for mv in legal_moves(P[0], max_parents, forbidden)
                   if not np.isnan(T[0, mv[2], mv[3]]) and not (mv[1] == 2 and np.isnan(T[0, mv[3], mv[2]]))]
            assert [got.count(op) for op in range(3)] == list(want_ops), got
        return M, codes

    chain = m({1: [0], 2: [1]})                                           # 0 -> 1 -> 2, 3 and 4 apart
    # adds: 20 ordered pairs - 2 present - 3 that close a cycle (1 -> 0, 2 -> 1, 2 -> 0); deletes 2; reversals 2
    M0, codes = run(chain, want_ops=(15, 2, 2))
    assert M0 == 19 and len(set(codes)) > 1
    forb = np.zeros(n, U64)
    forb[3] = U64(0b10111)                                               # nothing into 3 ...
    forb[0] = U64(1 << 1)                                                # ... and not 1 -> 0: the reversal of 0 -> 1 goes
    assert run(chain, forbidden=forb, want_ops=(11, 2, 1))[0] == 14
    # max_parents = 1: no add into 1 or 2, no reversal of 1 -> 2 (1 has a parent); reversing 0 -> 1 stays
    assert run(chain, max_parents=1, want_ops=(15 - 3 - 2, 2, 1))[0] == 13
    # a NaN cell removes the moves that read it: the add 4 -> 3; the delete of 0 -> 1 and, with it, its reversal
    assert run(chain, nan=((3, 4),), want_ops=(14, 2, 2))[0] == 18
    assert run(chain, nan=((1, 0),), want_ops=(15, 1, 1))[0] == 17
    assert run(chain, nan=((0, 1),), want_ops=(15, 2, 1))[0] == 18          # the cell only the reversal reads
    # a complete order with every absent edge forbidden but 1 -> 0 and 3 -> 2: ten deletes and those two reversals (of
    # the four covered edges u -> u + 1)
    order = m({v: list(range(v)) for v in range(n)})
    forb = np.array([~int(order[0, v]) & ((1 << n) - 1) & ~(1 << v) for v in range(n)], U64)
    forb[0] ^= U64(1 << 1)
    forb[2] ^= U64(1 << 3)
    M, codes = run(order, forbidden=forb, want_ops=(0, 10, 2))
    assert M == 12 and all(c >= n * n for c in codes)
    assert run(order, want_ops=(0, 10, 4))[0] == 14
    # M = 0: the empty graph with everything forbidden is left alone
    M, codes = run(m({}), forbidden=np.full(n, (1 << n) - 1, U64))
    assert M == 0 and codes == [None] * B
    # a flagged structure is left alone; a cycle is flagged
    P, L, T = hand_tables(chain, {})
    P1, L1, wl, fl = drv.perturb(P, L, T, 3, 2, flags=[2])
    assert P1.tobytes() == P.tobytes() and list(wl) == [-1, -1] and fl[0] == 2
    P, L, T = hand_tables(m({0: [2], 1: [0], 2: [1]}), {})
    P1, L1, wl, fl = drv.perturb(P, L, T, 3, 2)
    assert P1.tobytes() == P.tobytes() and list(wl) == [-1, -1] and fl[0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 6. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def check_argument_refusals(lib, ptr):
    be, p = sc.EmuBackend(lib), ptr                          # nothing is moved: dummy pointers as they are, the null stream
    last = lambda: lib.dvs_last_error().decode()
    tb, trb, rb, bb = 4 * 8 * 8 * 8, 4 * 10 * 16, 4 * 3 * 8 * 8, 4 * 8 * 8
    ts = lambda B=4, n=8, tb=tb, md=0.0, cap=10, tr=p, trb=trb, P=p, act=p, tl=3, ring=p, rb=rb, ms=5, best=p, bb=bb, vis=p: \
        call_rc(be, "dvs_tabu_step", batch=B, n_vars=n, parents=P, local=p, toggles=p, toggles_bytes=tb, max_parents=0, min_delta=md,
                forbidden=None, step_cap=cap, worklist=p, steps=p, converged=p, flags=p, trace=tr, trace_bytes=trb, active=act,
                tabu_len=tl, ring=ring, ring_bytes=rb, visited=vis, max_stall=ms, stall=p, best_score=p, best_parents=best,
                best_bytes=bb)
    assert ts(tb=tb - 1) == 14 and "toggles_bytes" in last() and str(tb) in last()
    assert ts(trb=trb - 1) == 14 and "trace_bytes" in last() and str(trb) in last()
    assert ts(rb=rb - 1) == 14 and "ring_bytes" in last() and str(rb) in last()
    assert ts(tl=4) == 14 and "ring_bytes" in last() and str(4 * 4 * 8 * 8) in last()
    assert ts(bb=bb - 1) == 14 and "best_bytes" in last() and str(bb) in last()
    assert ts(md=NAN) == 13 and "min_delta" in last()
    assert ts(cap=0) == 13 and "step_cap" in last()
    assert ts(tl=0) == 13 and "tabu_len" in last()
    assert ts(ms=0) == 13 and "max_stall" in last()
    assert ts(B=0) == 2 and ts(n=0) == 3 and ts(n=49) == 3
    assert ts(B=1 << 20, n=48, tb=1 << 40, trb=1 << 40, rb=1 << 40, bb=1 << 40) == 2
    assert ts(P=None) == 10 and ts(act=None) == 10 and ts(ring=None) == 10 and ts(best=None) == 10 and ts(vis=None) == 10
    pt = lambda B=4, n=8, tb=tb, P=p, wl=p, fl=p: call_rc(
        be, "dvs_hc_perturb", batch=B, n_vars=n, parents=P, local=p, toggles=p, toggles_bytes=tb, max_parents=0, forbidden=None,
        worklist=wl, flags=fl, seed=1, draw_index=0)
    assert pt(tb=tb - 1) == 14 and "toggles_bytes" in last() and str(tb) in last()
    assert pt(B=0) == 2 and pt(n=0) == 3 and pt(n=49) == 3 and pt(B=1 << 20, n=48, tb=1 << 40) == 2
    assert pt(P=None) == 10 and pt(wl=None) == 10 and pt(fl=None) == 10


# ---------------------------------------------------------------------------------------------------------------------
# 5. Two runs, and a batch is its rows
# ---------------------------------------------------------------------------------------------------------------------
def check_tabu_deterministic(drv, tc, r, head=5):
    case = tc.hc
    args = (tc.max_steps, tc.tabu, tc.max_tabu, case.max_parents, case.forbidden, case.min_delta)
    again = drv.tabu_climb(tc.starts, *args)
    for x, y in zip(r, again):
        assert x.tobytes() == y.tobytes()
    part = drv.tabu_climb(tc.starts[:head], *args)
    for x, y in zip(r, part):
        assert x[:head].tobytes() == y.tobytes()
