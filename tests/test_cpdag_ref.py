"""CPU: the references of tests/cpdag_corpus.py pinned before anything is compared against them — cpdag_ref against brute
force over all labelled DAGs on up to 5 vertices and against Chickering's covered-edge enumeration at n = 8 .. 10, compare_ref
against hand-made pairs."""
import pytest

from tests import cpdag_corpus as cp
from tests import scoring_corpus as sc
from tests.hillclimb_corpus import ASIA_KNOWN

CLASS_LIMIT = 20000
REVERSAL_INPUTS = [("asia", None, None)] + [(f"n{n}s{seed}", n, seed) for n in (8, 9, 10) for seed in (1, 2, 3, 4)]


@pytest.mark.parametrize("n", [3, 4, 5])
def test_cpdag_ref_equals_brute_force_on_all_labelled_dags(n):
    """(a) classes by skeleton and v-structures, an arc compelled iff its direction is constant in the class"""
    brute, n_classes = cp.brute_cpdags(n)
    assert len(brute) == cp.DAG_COUNTS[n] and n_classes == cp.CLASS_COUNTS[n]
    ref = cp.ref_all(n)
    wrong = [P for P, (rows, _) in zip(cp.all_dags(n), ref) if tuple(rows) != brute[P]]
    assert not wrong, (n, len(wrong), wrong[:3])
    assert len({tuple(rows) for rows, _ in ref}) == n_classes             # the rows are a key of the class
    if n >= 4:
        assert set().union(*(f for _, f in ref)) == set(cp.RULES)


def test_every_rule_is_needed_at_n_4():
    """without R1, R2 or R3 the reference misses the brute-force compelled set on 36, 24 and 36 of the 543 DAGs"""
    brute, _ = cp.brute_cpdags(4)
    missed = {}
    for drop in cp.RULES:
        rules = tuple(r for r in cp.RULES if r != drop)
        missed[drop] = sum(tuple(cp.cpdag_ref(P, rules)[0]) != brute[P] for P in cp.all_dags(4))
    print(f"\nDAGs of n = 4 missed without a rule: {missed}")
    assert missed == {"R1": 36, "R2": 24, "R3": 36}


@pytest.mark.parametrize("name,n,seed", REVERSAL_INPUTS)
def test_cpdag_ref_equals_the_class_enumerated_by_covered_edge_reversals(name, n, seed):
    """(b) the second route: breadth-first covered-edge reversals reach the whole class (Chickering); the compelled arcs
    are those with one direction in it.  Every input is used: none has a class above the limit."""
    if n is None:
        P = [int(x) for x in sc.masks_of(8, ASIA_KNOWN)[0]]
    else:
        P = [int(x) for x in cp.random_dags(n, 1, cp.SPARSE(n), seed=100 * n + seed)[0]]
    members = cp.class_by_reversals(P, CLASS_LIMIT)
    assert members is not None, (name, "class above the limit: choose another seed")
    assert all(cp.class_key(m) == cp.class_key(P) for m in members)
    rows, _ = cp.cpdag_ref(P)
    assert rows == cp.compelled_rows(members), name
    assert all(cp.cpdag_ref(m)[0] == rows for m in members[:50])
    print(f"\n{name}: {len(members)} members, {cp.n_edges(rows)} edges")


def test_compare_ref_on_hand_made_pairs_and_its_identities():
    for name, a, t, want in cp.hand_pairs():
        assert cp.compare_ref(a, t) == want, name
        assert cp.compare_ref(t, a) == (want[0], want[1], want[3], want[2], want[4]), name
    for n in (5, 33, 48):
        A, T = cp.random_pdags(n, 8, seed=40 + n), cp.random_pdags(n, 8, seed=90 + n)
        for a, t in zip(A, T):
            shd, tp, fp, fn, ham = cp.compare_ref(a, t)
            assert tp + fn == cp.n_edges(t) and tp + fp == cp.n_edges(a)
            assert ham <= shd <= tp + fp + fn and cp.compare_ref(a, a) == (0, cp.n_edges(a), 0, 0, 0)


def test_flags_ref_and_the_inputs():
    assert cp.flags_ref([0b10, 0b01]) == 1 and cp.flags_ref([0b01, 0]) == 2 and cp.flags_ref([0b100, 0]) == 2
    assert cp.flags_ref([0, 0b01]) == 0
    for n in cp.RANDOM_SIZES:
        for k, density in enumerate((cp.SPARSE(n), 0.5)):
            assert not any(cp.flags_ref(row) for row in cp.random_dags(n, 8, density, seed=1000 * n + k))
