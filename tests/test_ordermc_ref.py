"""CPU pins of the reference of tests/ordermc_corpus.py, before any kernel is trusted against it: the sampler it restates has
the order-modular posterior as its stationary distribution (the exact Metropolis transition matrix over all orders at n = 3
and 4; 256 chains at n = 5 against brute force over every DAG), every seeded case of the corpus meets the bracket condition,
and the list built from a table holds the cells of the exact posterior."""
import itertools
import math

import numpy as np
import pytest

from tests import ordermc_corpus as oc
from tests import posterior_corpus as po


def _table_case(n, kind, seed):
    table = po.make_tables(kind, 1, n, seed=seed, scale=1.5)[0]
    cap, forb, prior = po.settings(kind, n, seed)
    return table, cap, forb, prior


@pytest.mark.parametrize("window", [1, None])
@pytest.mark.parametrize("n,kind", [(3, "random"), (3, "ties"), (4, "random"), (4, "ties"), (4, "prior")])
def test_the_order_posterior_is_stationary_and_its_arcs_are_brute_force(n, kind, window):
    """T[s, s'] = P(i, j) min(1, exp(Delta)) from the definitions; pi ~ exp(order score); pi T = pi, and pi's Rao-Blackwellised
    arc probabilities are those of the enumeration over all DAGs"""
    table, cap, forb, prior = _table_case(n, kind, 7 * n)
    fam = oc.list_from_table(table, cap, forb, prior)
    T = oc.Terms(fam)
    window = n - 1 if window is None else window
    orders = list(itertools.permutations(range(n)))
    index = {o: k for k, o in enumerate(orders)}

    def score(o):
        pred = oc.preds_of(o)
        return sum(T(v, pred[v])[0] for v in range(n))
    S = np.array([score(o) for o in orders])
    pi = np.exp(S - S.max())
    pi /= pi.sum()
    P = np.zeros((len(orders), len(orders)))
    for k, o in enumerate(orders):
        for i in range(n - 1):
            m = min(window, n - 1 - i)
            for j in range(i + 1, i + m + 1):
                new = list(o)
                new[i], new[j] = new[j], new[i]
                k2 = index[tuple(new)]
                a = (1.0 / (n - 1)) * (1.0 / m) * min(1.0, math.exp(S[k2] - S[k]))
                P[k, k2] += a
                P[k, k] -= a
        P[k, k] += 1.0
    assert np.abs(P.sum(1) - 1.0).max() <= 1e-14 and np.abs(pi @ P - pi).max() <= 1e-14
    # irreducible: adjacent swaps reach every order; the proposal's pair probabilities do not depend on the order
    arcs = np.zeros((n, n))
    for k, o in enumerate(orders):
        pred = oc.preds_of(o)
        for v in range(n):
            arcs[:, v] += pi[k] * T.arc_row(v, pred[v])
    brute = po.ref_brute(table, cap, forb, prior)
    assert np.abs(arcs - brute.prob).max() <= 1e-12, (arcs, brute.prob)


def test_the_draws_give_every_pair_of_positions_its_stated_share():
    """i = (r0 (n - 1)) >> 32, j = i + 1 + ((r1 m) >> 32): 30 000 steps of one chain at n = 5, window 2"""
    key = oc.orng.site_key(3, oc.SITE, 0)
    n, w, N = 5, 2, 30000
    counts = {}
    for t in range(N):
        i, j, logu = oc.proposal(n, w, key, t)
        assert 0 <= i < j <= min(n - 1, i + w) and logu < 0.0
        counts[(i, j)] = counts.get((i, j), 0) + 1
    for i in range(n - 1):
        m = min(w, n - 1 - i)
        for j in range(i + 1, i + m + 1):
            p = 1.0 / (n - 1) / m
            assert abs(counts[(i, j)] / N - p) <= 5 * math.sqrt(p * (1 - p) / N), (i, j)
    assert sorted(oc.start_order(9, 1, 2)) == list(range(9)) and oc.start_order(9, 1, 2) != oc.start_order(9, 1, 3)


@pytest.mark.parametrize("kind,seed", [("random", 101), ("ties", 102), ("prior", 103)])
def test_256_chains_at_n5_agree_with_brute_force(kind, seed):
    """the chain mean within 5 between-chain standard errors of the enumeration's prob: plain, capped and blacklisted, and
    size-prior tables"""
    n, chains = 5, 256
    table, cap, forb, prior = _table_case(n, kind, seed)
    fam = oc.list_from_table(table, cap, forb, prior)
    ref = oc.ref_run(fam, chains, 240, 40, 4, 1, seed)
    assert ref.kept.tolist() == [50] * chains
    per_chain = ref.sums / ref.kept[:, None, None]
    se = per_chain.std(0, ddof=1) / math.sqrt(chains)
    brute = po.ref_brute(table, cap, forb, prior)
    assert (np.abs(ref.prob - brute.prob) <= 5 * se + 1e-12).all(), (np.abs(ref.prob - brute.prob).max(), se.max())
    assert se.max() > 0.0 and 0.05 < ref.accepted.mean() / 240 < 1.0
    if forb is not None:
        for v in range(n):
            for u in range(n):
                if (int(forb[v]) >> u) & 1:
                    assert ref.prob[u, v] == 0.0


@pytest.mark.parametrize("name", sorted(oc.TRAJECTORIES))
def test_every_seeded_case_keeps_its_decisions_outside_the_bracket(name):
    """the CONDITION of the corpus: no accept decision of the reference within tau of its threshold, so the back ends may be
    asked for the reference's trajectory exactly"""
    fam, args, ref = oc.trajectory_case(name)
    assert fam.n == 1 or len(ref.margins) == args["chains"] * args["steps"]
    assert (ref.margins > 0.0).all(), (name, float(ref.margins.min()))
    for c in range(args["chains"]):
        assert sorted(ref.order[c].tolist()) == list(range(fam.n))
    if fam.n > 1 and name not in ("long",):
        assert 0 < ref.accepted.sum() < args["chains"] * args["steps"]


def test_range_cases_meet_the_condition_and_the_dominant_dag_is_found():
    for which in ("offsets", "dominated"):
        fam, args, ref, want = oc.range_case(which)
        assert (ref.margins > 0.0).all() and np.isfinite(ref.prob).all()
        if want is not None:
            assert ref.best_parents[int(np.argmax(ref.best_score))].tobytes() == np.asarray(want, np.uint64).tobytes()


def test_list_from_table_holds_the_cells_of_the_exact_posterior():
    table, cap, forb, prior = _table_case(5, "ties", 5)
    table[0b00110, 0] = np.nan
    fam = oc.list_from_table(table, cap, forb, prior)
    f = po.f_cells(table, cap, forb, prior)
    assert fam.F == int((f > -np.inf).sum()) and fam.offsets[0] == 0
    for v in range(5):
        lo, hi = int(fam.offsets[v]), int(fam.offsets[v + 1])
        sets = fam.sets[lo:hi].astype(np.int64)
        assert sets[0] == 0 and fam.scores[lo:hi].tobytes() == f[sets, v].tobytes()
        keys = [(bin(int(s)).count("1"), int(s)) for s in sets]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)


def test_tolerances_at_the_scale_of_the_derivation():
    fam = oc.enumerated_list(5, 4, lambda v, m: np.full(len(m), 3.0))
    assert oc.stats(fam) == (16, 3.0)
    assert oc.eps_term(fam) == 15 * (2.0 ** -53 * 3.0 + 2.0 ** -52) and oc.tau(fam, 2) == 4 * oc.eps_sum(fam, 2) < 1e-12
    assert oc.closed_arc(1, 2) == 0.5 and oc.closed_arc(3, 2) == 3 / 7
