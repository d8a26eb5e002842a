"""select_ref (tests/hillclimb_corpus.py), the reference the hill-climb kernels are pinned against, pinned itself: against
brute force over all moves at n = 4 with acyclicity decided by Kahn's algorithm on the moved graph, plus the tie-break
order and the forbidden / max_parents rules.  Plain Python, no library."""
import itertools

import numpy as np

from tests import hillclimb_corpus as hc


def kahn_acyclic(P):
    n = len(P)
    indeg = [bin(int(P[v]) & ((1 << n) - 1)).count("1") for v in range(n)]
    todo = [v for v in range(n) if indeg[v] == 0]
    seen = 0
    while todo:
        u = todo.pop()
        seen += 1
        for v in range(n):
            if (int(P[v]) >> u) & 1:
                indeg[v] -= 1
                if indeg[v] == 0:
                    todo.append(v)
    return seen == n


def brute_moves(P, max_parents, forbidden):
    """every (code, op, v, u) whose moved graph is a DAG (Kahn) and respects the cap and the forbidden edges"""
    n = len(P)
    out = []
    for op, v, u in itertools.product(range(3), range(n), range(n)):
        if u == v:
            continue
        has = (int(P[v]) >> u) & 1
        if (op == 0) == bool(has):
            continue
        Q = [int(x) for x in P]
        Q[v] ^= 1 << u
        grown, edge = None, None
        if op == 0:
            grown, edge = v, (u, v)
        if op == 2:
            Q[u] |= 1 << v
            grown, edge = u, (v, u)
        if not kahn_acyclic(Q):
            continue
        if grown is not None:
            if max_parents and bin(int(P[grown])).count("1") >= max_parents:
                continue
            if forbidden is not None and (int(forbidden[edge[1]]) >> edge[0]) & 1:
                continue
        out.append((op * n * n + v * n + u, op, v, u))
    return sorted(out)


def all_dags(n):
    pairs = [(u, v) for u in range(n) for v in range(n) if u != v]
    for bits in range(1 << len(pairs)):
        P = [0] * n
        for i, (u, v) in enumerate(pairs):
            if (bits >> i) & 1:
                P[v] |= 1 << u
        if kahn_acyclic(P):
            yield P


def test_legal_moves_equal_brute_force_on_every_dag_of_four_vertices():
    count = 0
    forb = [0b0100, 0, 0b0001, 0b0010]
    for P in all_dags(4):
        count += 1
        assert not hc.has_cycle(P)
        for mp, fb in ((None, None), (1, None), (2, forb), (None, forb)):
            assert hc.legal_moves(P, mp, fb) == brute_moves(P, mp, fb), (P, mp, fb)
    assert count == 543                                  # labelled DAGs on 4 vertices


def test_closure_flags_exactly_the_cyclic_graphs():
    pairs = [(u, v) for u in range(4) for v in range(4) if u != v]
    for bits in range(0, 1 << len(pairs), 7):
        P = [0] * 4
        for i, (u, v) in enumerate(pairs):
            if (bits >> i) & 1:
                P[v] |= 1 << u
        assert hc.has_cycle(P) == (not kahn_acyclic(P))
    assert hc.has_cycle([0b0001, 0, 0, 0])               # a self-loop


def test_select_ref_takes_the_brute_force_argmax_with_the_tie_break():
    rng = np.random.default_rng(4)
    dags = list(all_dags(4))
    for i in range(300):
        P = dags[int(rng.integers(len(dags)))]
        L = rng.integers(-3, 4, 4).astype(np.float64)                  # small integers: exact ties are frequent
        T = rng.integers(-3, 4, (4, 4)).astype(np.float64)
        if i % 3 == 0:
            T[rng.integers(4), rng.integers(4)] = np.nan               # a refused cell: moves reading it are unavailable
        mp = (None, 1, 2)[i % 3]
        cand = []
        for code, op, v, u in brute_moves(P, mp, None):
            d = (T[v, u] - L[v]) + (T[u, v] - L[u]) if op == 2 else T[v, u] - L[v]
            if not np.isnan(d):
                cand.append((-d, code))
        got = hc.select_ref(P, L, T, mp, None, 0.0)
        want = min(cand) if cand and -min(cand)[0] > 0.0 else None
        assert (got is None) == (want is None), (P, L, T)
        if got is not None:
            assert got[0] == want[1] and got[1] == -want[0]


def test_tie_break_order_is_add_delete_reverse_then_child_then_parent():
    n = 4
    P = [0, 0b0001, 0, 0]                                # 0 -> 1
    L = np.zeros(n)
    T = np.full((n, n), -1.0)
    T[1, 0] = 2.0                                        # delete 0 -> 1: 2
    T[0, 1] = 0.0                                        # reverse 0 -> 1: 2 + 0 = 2
    T[3, 2] = 2.0                                        # add 2 -> 3: 2
    T[2, 3] = 2.0                                        # add 3 -> 2: 2
    assert hc.select_ref(P, L, T) == (2 * n + 3, 2.0)    # op 0 first, then the lower child
    T[2, 3] = -1.0
    assert hc.select_ref(P, L, T) == (3 * n + 2, 2.0)
    T[3, 2] = -1.0
    assert hc.select_ref(P, L, T) == (n * n + 1 * n + 0, 2.0)         # delete before reverse
    T[1, 0], T[0, 1] = 1.0, 1.0
    assert hc.select_ref(P, L, T) == (2 * n * n + 1 * n + 0, 2.0)
    assert hc.select_ref(P, L, T, min_delta=2.0) is None              # strict


def test_forbidden_and_max_parents_rules():
    n = 4
    P = [0, 0b0001, 0b0011, 0]                           # 0 -> 1, 0 -> 2, 1 -> 2
    codes = lambda mp=None, fb=None: {c for c, _, _, _ in hc.legal_moves(P, mp, fb)}
    add = lambda u, v: v * n + u
    rev = lambda u, v: 2 * n * n + v * n + u
    assert add(3, 2) in codes() and add(3, 2) not in codes(mp=2) and add(3, 1) in codes(mp=2)
    assert add(3, 2) not in codes(fb=[0, 0, 0b1000, 0]) and add(3, 1) in codes(fb=[0, 0, 0b1000, 0])
    assert rev(1, 2) in codes() and rev(1, 2) not in codes(mp=1)      # 1 would get a second parent
    assert rev(1, 2) not in codes(fb=[0, 0b0100, 0, 0])               # the reversed edge 2 -> 1 is forbidden
    assert rev(0, 2) not in codes()                                   # 0 -> 1 -> 2 remains: 2 -> 0 would close a cycle
    assert all(c // (n * n) != 1 or True for c in codes(mp=1))
    assert {n * n + 1 * n + 0, n * n + 2 * n + 0, n * n + 2 * n + 1} <= codes(mp=1, fb=[15] * 4)   # deletes are always legal
