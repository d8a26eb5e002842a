"""TEST HELPER: hand-made dvs_decode_state rows for the search-candidate kernels (dvs_decoded_structures,
dvs_structset_filter), independent of any model, and the host functions that define what the kernels must compute."""
import types

import numpy as np

from dags_vae_search_amd import LabeledDag, LabeledGraph
from dags_vae_search_amd.bic import BNLearnWrapper
from dags_vae_search_amd.features import LABEL_KEY
from dags_vae_search_amd.pace import graphs_from_states
from dags_vae_search_amd.records import encode_graphs
from dags_vae_search_amd.search import is_search_valid, new_structures, structure_key
from tests import recon_corpus as rc

SHAPES = (4, 8, 12, 13, 14, 37, 45)
KINDS = ("base", "reordered", "edge", "swap", "short", "low", "high", "repeat", "extra")
PER_KIND = 20
ALL_ONES = 0xFFFFFFFFFFFFFFFF
HASH_INVALID = 0x7FFFFFFFFFFFFFFF


def permutation_dag(rng, n):
    g = rc.random_dag(rng, n, 1)
    return LabeledGraph([int(x) for x in rng.permutation(n)], list(g.edges))


def _changed(rng, g, change):
    """``change`` applied until the Bayesian-network structure differs (a swap of two interchangeable vertices does not)."""
    for _ in range(200):
        h = change(rng, g)
        if h is not None and structure_key(h) != structure_key(g):
            return h
    raise AssertionError("no structure-changing variant found")


def corpus(n, seed=11):
    """(raw states uint8 [B, 440], kind name per row, base index per row): PER_KIND rows of every kind in KINDS.  Rows
    b, b + PER_KIND, ... are variants of base graph b."""
    rng = np.random.default_rng(seed * 1000 + n)
    bases = [permutation_dag(rng, n) for _ in range(PER_KIND)]
    graphs, kinds, nv = [], [], []

    def add(kind, g, rows=n + 3):
        graphs.append(g)
        kinds.append(kind)
        nv.append(rows)

    for g in bases:
        add("base", g)
    for g in bases:
        add("reordered", rc.topo_permuted(rng, g))
    for g in bases:
        add("edge", _changed(rng, g, rc.one_edge_changed) if n > 1 else g)
    for g in bases:
        add("swap", _changed(rng, g, rc.labels_swapped))
    for g in bases:
        add("short", g, int(rng.integers(2, n + 3)))
    for g in bases:                                  # a PACE label 0 / 1 / 2 at a user vertex
        lab = list(g.labels)
        lab[int(rng.integers(0, n))] = int(rng.integers(-3, 0))
        add("low", LabeledGraph(lab, list(g.edges)))
    for g in bases:                                  # a PACE label >= n_vars + 3
        lab = list(g.labels)
        lab[int(rng.integers(0, n))] = int(rng.integers(n, 253))
        add("high", LabeledGraph(lab, list(g.edges)))
    for g in bases:
        lab = list(g.labels)
        a, b = rng.choice(n, 2, replace=False)
        lab[a] = lab[b]
        add("repeat", LabeledGraph(lab, list(g.edges)))
    for g in bases:
        add("extra", g)
    raw = rc.states_of(graphs, n, nv=nv)
    # "extra": edges from PACE vertices 0 / 1 into every vertex and edges from everything into the closing vertex
    parents = np.ascontiguousarray(raw[:, :384]).view(np.uint64).reshape(len(graphs), 48)
    for b, kind in enumerate(kinds):
        if kind == "extra":
            parents[b, 2:n + 2] |= rng.integers(1, 4, n).astype(np.uint64)
            parents[b, 2] |= np.uint64(3)
            parents[b, n + 2] = np.uint64((1 << (n + 2)) - 1) & np.uint64(int(rng.integers(1, 1 << 62)) | 5)
    raw[:, :384] = parents.view(np.uint8).reshape(len(graphs), 384)
    base_of = [b % PER_KIND for b in range(len(graphs))]
    assert all(kinds.count(k) >= PER_KIND for k in KINDS)
    return raw, kinds, base_of


def host_view(raw, n):
    """What the host stage makes of the rows: (graphs, valid bool [B])."""
    graphs = graphs_from_states(raw, n + 3)
    dag = LabeledDag(n, n)
    return graphs, np.asarray([is_search_valid(g, dag) for g in graphs])


def host_parent_masks(graphs, n):
    return BNLearnWrapper._parent_masks(types.SimpleNamespace(n_vars=n), graphs, LABEL_KEY)


def check_rows(raw, n, flags, labels, preds, keys):
    """Flags bit 0, codec and key of every row against the host functions.  Returns (graphs, valid)."""
    graphs, valid = host_view(raw, n)
    assert np.array_equal((flags & 1).astype(bool), valid), np.nonzero((flags & 1).astype(bool) != valid)[0][:8]
    rows = np.nonzero(valid)[0]
    if len(rows):
        cb = encode_graphs([graphs[i] for i in rows], n)
        assert cb.labels.numpy().tobytes() == labels[rows].tobytes()
        want_preds = cb.preds.numpy()
        assert preds.dtype.itemsize == want_preds.dtype.itemsize
        assert want_preds.tobytes() == preds[rows].tobytes()
        assert np.array_equal(host_parent_masks([graphs[i] for i in rows], n), keys[rows])
    bad = np.nonzero(~valid)[0]
    assert not labels[bad].any() and not preds[bad].any() and not keys[bad].any()
    assert ((flags[bad] & 1) == 0).all() and (flags[bad] != 0).all()
    return graphs, valid


def host_new_mask(graphs, n, seen):
    """search.new_structures on the rows in order, as a bool mask; ``seen`` (a set of structure_key) is updated."""
    # one object per row (the caller may pass the same object for several rows; the mask below goes by identity)
    graphs = [None if g is None else LabeledGraph(list(g.labels), list(g.edges)) for g in graphs]
    out, _ = new_structures(graphs, LabeledDag(n, n), seen)
    ids = {id(g) for g in out}
    return np.asarray([g is not None and id(g) in ids for g in graphs])
