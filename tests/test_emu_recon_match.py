"""CPU: dvs_match_decoded (csrc/dvs_match.h, the device-side reconstruction judge) on the host emulator, against the host's
LabeledDag.is_valid_graph / graph_equals on the same pairs; and the pure-Python judge of the GPU tests against networkx."""
import ctypes

import numpy as np
import pytest

from dags_vae_search_amd import LabeledDag, LabeledGraph
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd.pace import graphs_from_states
from dags_vae_search_amd.recon import DEFAULT_BUDGET, judge_on_host
from dags_vae_search_amd.records import encode_graphs
from tests import iso_ref
from tests import recon_corpus as rc
from tests.emu.harness import emu, ptr

try:
    import networkx  # noqa: F401
    HAVE_NX = True
except ImportError:
    HAVE_NX = False


class _Judge(LabeledDag):
    """The toolkit, with the pure-Python judge standing in for networkx where networkx is missing."""

    def graph_equals(self, g1, g2, attributes_match=True):
        if HAVE_NX:
            return super().graph_equals(g1, g2, attributes_match)
        return iso_ref.graph_equals(g1, g2, attributes_match)


def judge_fn(g1, g2, attributes_match=True):
    return _Judge(1, 1).graph_equals(g1, g2, attributes_match)


def run_match(targets, raw, repeats, n, card, budget=DEFAULT_BUDGET):
    lib = emu()
    cb = encode_graphs(targets, n)
    labels = np.ascontiguousarray(cb.labels.numpy())
    preds = np.ascontiguousarray(cb.preds.numpy())
    flags = np.full(raw.shape[0], 0xFF, np.uint8)
    dl.check(lib, lib.dvs_match_decoded(len(targets), n, card, repeats, 1 if n > 13 else 0, ptr(labels), ptr(preds),
                                        ptr(raw), raw.nbytes, budget, ptr(flags), None), "dvs_match_decoded")
    return flags


def expected_flags(toolkit, targets, raw, repeats, n):
    out = []
    for k, g in enumerate(graphs_from_states(raw, n + 3)):
        t = targets[k // repeats]
        s = toolkit.graph_equals(t, g, attributes_match=False)
        out.append(int(toolkit.is_valid_graph(g)) | 2 * int(s) | 4 * int(toolkit.graph_equals(t, g)))
    return np.asarray(out, np.uint8)


def check_pairs(pairs, n, card):
    toolkit = _Judge(n, card)
    targets = [t for t, _ in pairs]
    raw = rc.states_of([g for _, g in pairs], n)
    got = run_match(targets, raw, 1, n, card)
    want = expected_flags(toolkit, targets, raw, 1, n)
    bad = [(k, int(got[k]), int(want[k])) for k in range(len(pairs)) if got[k] != want[k]]
    assert not bad, f"n={n} card={card}: (pair, device, host) {bad[:8]}"
    return got


CORPUS = rc.corpus(judge_fn)


@pytest.mark.parametrize("key", sorted(CORPUS), ids=[f"n{n}c{c}" for n, c in sorted(CORPUS)])
def test_flags_equal_host_judge(key):
    n, card = key
    got = check_pairs(CORPUS[key], n, card)
    assert not (got & 8).any()
    assert ((got & 4) == 0).all() or ((got[(got & 4) != 0] & 2) != 0).all()          # labelled implies structure
    assert (got & 2).any() and not (got & 2).all()                                     # both answers occur


def test_wl_equivalent_pairs_are_told_apart():
    """Equal degree sequences and equal 1-WL colourings, not isomorphic: decided by the search, not by refinement."""
    for k, n in ((6, 12), (7, 14)):
        pairs = rc.wl_equivalent_pairs(judge_fn, k, 7 + (k - 6))
        assert len(pairs) >= 1
        for a, b in pairs:
            assert rc.wl_histogram(a) == rc.wl_histogram(b)
        got = check_pairs(pairs, n, 1)
        assert ((got & 2) == 0).all() and not (got & 8).any()


def test_symmetric_n45_decided_under_default_budget():
    pairs = rc.symmetric_pairs(np.random.default_rng(3))
    got = check_pairs(pairs, 45, 1)
    assert not (got & 8).any()
    assert ((got[:7] & 6) == 6).all()          # the renumbered copies


def test_short_rows_and_out_of_range_labels():
    rng = np.random.default_rng(5)
    n, card = 12, 3
    toolkit = _Judge(n, card)
    g = rc.random_dag(rng, n, card)
    low = LabeledGraph([-2] + list(g.labels[1:]), list(g.edges))             # PACE label 1 at user vertex 0
    neg = LabeledGraph([x - 3 for x in g.labels], list(g.edges))              # every label in -3 .. -1
    dec = [g, rc.topo_permuted(rng, g), low, neg, g]
    raw = rc.states_of(dec, n, nv=[n + 3, n + 2, n + 3, n + 3, 5])
    targets = [g]
    got = run_match(targets, raw, len(dec), n, card)
    want = expected_flags(toolkit, targets, raw, len(dec), n)
    assert list(got) == list(want)
    assert list(got) == [7, 0, 2, 2, 0]


def test_repeats_group_rows_by_target():
    rng = np.random.default_rng(9)
    n, card, R = 8, 2, 3
    toolkit = _Judge(n, card)
    targets = [rc.random_dag(rng, n, card) for _ in range(4)]
    dec = []
    for t in targets:
        dec += [rc.topo_permuted(rng, t), rc.one_edge_changed(rng, t), t]
    raw = rc.states_of(dec, n)
    got = run_match(targets, raw, R, n, card)
    assert list(got) == list(expected_flags(toolkit, targets, raw, R, n))


def test_budget_one_is_undecided_and_host_fallback_answers():
    rng = np.random.default_rng(13)
    n, card = 13, 1
    toolkit = _Judge(n, card)
    pairs = [(g, rc.topo_permuted(rng, g)) for g in (rc.random_dag(rng, n, card) for _ in range(3))]
    pairs += [(t, rc.one_edge_changed(rng, t)) for t, _ in pairs[:1]]
    targets = [t for t, _ in pairs]
    raw = rc.states_of([g for _, g in pairs], n)
    got = run_match(targets, raw, 1, n, card, budget=1)
    want = expected_flags(toolkit, targets, raw, 1, n)
    und = (got & 8) != 0
    assert und[:3].all()
    assert ((got & 1) == (want & 1)).all()
    rows = np.nonzero(und)[0]
    host = judge_on_host(raw[rows], [targets[k] for k in rows], toolkit, n + 3)
    assert host == [int(want[k]) & 6 for k in rows]


def test_abi_argument_checks_without_a_gpu():
    lib = dl.load()
    d = ctypes.c_void_p(16)                 # dummy pointers: every check runs before anything is enqueued
    need = 4 * 3 * dl.DECODE_STATE_BYTES
    assert lib.dvs_match_decoded(4, 12, 1, 3, 0, None, d, d, need, 64, d, None) == 10
    assert lib.dvs_match_decoded(4, 12, 1, 3, 0, d, d, d, need, 64, None, None) == 10
    assert lib.dvs_match_decoded(0, 12, 1, 3, 0, d, d, d, need, 64, d, None) == 2
    assert lib.dvs_match_decoded(4, 12, 1, 0, 0, d, d, d, need, 64, d, None) == 2
    assert lib.dvs_match_decoded(4, 46, 1, 3, 1, d, d, d, need, 64, d, None) == 3
    assert lib.dvs_match_decoded(4, 12, 0, 3, 0, d, d, d, need, 64, d, None) == 3
    assert lib.dvs_match_decoded(4, 12, 46, 3, 0, d, d, d, need, 64, d, None) == 3
    assert lib.dvs_match_decoded(4, 12, 1, 3, 0, d, d, d, need - 1, 64, d, None) == 14
    assert str(need).encode() in lib.dvs_last_error()


@pytest.mark.skipif(not HAVE_NX, reason="networkx is optional")
def test_iso_ref_agrees_with_networkx():
    tk = LabeledDag(1, 1)
    n_pairs = 0
    for pairs in CORPUS.values():
        for a, b in pairs:
            for attr in (False, True):
                assert iso_ref.graph_equals(a, b, attr) == tk.graph_equals(a, b, attr)
            n_pairs += 1
    assert n_pairs > 100
