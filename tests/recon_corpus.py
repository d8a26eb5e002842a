"""TEST HELPER: pairs (target, decoded graph) for the reconstruction judge (dvs_match_decoded), built on the host.

Decoded rows are written as dvs_decode_state records the way dvs_decode leaves them: PACE vertex 0 start (label 2),
1 input (0), user vertex i at PACE i + 2 with label + 3, the output vertex last, parent bits shifted by 2."""
import numpy as np

from dags_vae_search_amd import LabeledGraph
from dags_vae_search_amd import _lib as dl


def random_dag(rng, n, card, density=None):
    p = density if density is not None else min(0.5, 2.5 / max(n - 1, 1))
    edges = [(u, v) for v in range(n) for u in range(v) if rng.random() < p]
    labels = [int(x) for x in rng.integers(0, card, n)]
    return LabeledGraph(labels, edges)


def topo_permuted(rng, g):
    """The same graph with its vertices permuted, then renumbered in a (random) topological order."""
    n = len(g.labels)
    perm = rng.permutation(n)
    edges = [(int(perm[u]), int(perm[v])) for u, v in g.edges]
    labels = [0] * n
    for v in range(n):
        labels[perm[v]] = g.labels[v]
    indeg = [0] * n
    succ = [[] for _ in range(n)]
    for u, v in edges:
        succ[u].append(v)
        indeg[v] += 1
    ready = [v for v in range(n) if indeg[v] == 0]
    order = []
    while ready:
        v = ready.pop(int(rng.integers(0, len(ready))))
        order.append(v)
        for w in succ[v]:
            indeg[w] -= 1
            if indeg[w] == 0:
                ready.append(w)
    pos = {v: i for i, v in enumerate(order)}
    return LabeledGraph([labels[v] for v in order], sorted((pos[u], pos[v]) for u, v in edges))


def one_edge_changed(rng, g):
    n = len(g.labels)
    slots = [(u, v) for v in range(n) for u in range(v)]
    e = slots[int(rng.integers(0, len(slots)))]
    edges = set(g.edges)
    edges.symmetric_difference_update({e})
    return LabeledGraph(list(g.labels), sorted(edges))


def labels_swapped(rng, g):
    """Two vertices with different labels exchange them (same structure); None when all labels are equal."""
    pairs = [(a, b) for a in range(len(g.labels)) for b in range(a) if g.labels[a] != g.labels[b]]
    if not pairs:
        return None
    a, b = pairs[int(rng.integers(0, len(pairs)))]
    lab = list(g.labels)
    lab[a], lab[b] = lab[b], lab[a]
    return LabeledGraph(lab, list(g.edges))


_WL_TABLE = {}


def wl_histogram(g):
    """Directed 1-WL colour multiset after n rounds (canonical: every round's signature is renamed through one table
    shared by all graphs, so equal colours mean equal signatures)."""
    n = len(g.labels)
    par = [[] for _ in range(n)]
    chi = [[] for _ in range(n)]
    for u, v in g.edges:
        par[v].append(u)
        chi[u].append(v)
    col = [_WL_TABLE.setdefault((len(par[v]), len(chi[v])), len(_WL_TABLE)) for v in range(n)]
    for _ in range(n):
        sig = [(col[v], tuple(sorted(col[u] for u in par[v])), tuple(sorted(col[u] for u in chi[v]))) for v in range(n)]
        col = [_WL_TABLE.setdefault(s, len(_WL_TABLE)) for s in sig]
    return sorted(col)


def regular_bipartite(rng, k):
    """Sources 0..k-1, sinks k..2k-1, every source with 2 children and every sink with 2 parents (a union of cycles)."""
    while True:
        a, b = rng.permutation(k), rng.permutation(k)
        if all(a[i] != b[i] for i in range(k)):
            edges = sorted({(i, k + int(a[i])) for i in range(k)} | {(i, k + int(b[i])) for i in range(k)})
            return LabeledGraph([0] * (2 * k), edges)


def wl_equivalent_pairs(judge, k, seed, want=2):
    """Seeded search: 2-regular bipartite DAGs on 2k vertices have equal 1-WL colourings; keep pairs that are not
    isomorphic (different cycle structure)."""
    rng = np.random.default_rng(seed)
    pool = [regular_bipartite(rng, k) for _ in range(12)]
    out = []
    for i in range(len(pool)):
        for j in range(i):
            if len(out) < want and wl_histogram(pool[i]) == wl_histogram(pool[j]) and not judge(pool[i], pool[j], False):
                out.append((pool[i], topo_permuted(rng, pool[j])))
    return out


def layered(sizes):
    """Complete bipartite edges between consecutive layers."""
    edges, start = [], 0
    for a, b in zip(sizes, sizes[1:]):
        edges += [(start + i, start + a + j) for i in range(a) for j in range(b)]
        start += a
    return LabeledGraph([0] * sum(sizes), edges)


def chains(count, length):
    return LabeledGraph([0] * (count * length), [(c * length + i, c * length + i + 1) for c in range(count)
                                                for i in range(length - 1)])


def symmetric_pairs(rng, n=45):
    """Highly symmetric n = 45 card = 1 graphs against renumbered copies and against non-isomorphic look-alikes."""
    base = [LabeledGraph([0] * n, []), layered([15, 15, 15]), layered([5] * 9), layered([3, 12, 12, 3, 15]),
            chains(5, 9), chains(9, 5), chains(15, 3)]
    pairs = [(g, topo_permuted(rng, g)) for g in base]
    # (non-isomorphic pairs with equal degree sequences made of many equal components are left out: networkx's VF2, the
    # host judge they are compared with, takes exponential time on them)
    pairs += [(chains(5, 9), chains(9, 5)), (layered([15, 15, 15]), layered([15, 14, 16]))]
    return pairs


def states_of(graphs, n, nv=None):
    """dvs_decode_state records (numpy uint8 [B, DECODE_STATE_BYTES]) of decoded user graphs (labels may be -3..-1)."""
    B = len(graphs)
    parents = np.zeros((B, 48), np.uint64)
    labels = np.zeros((B, 48), np.uint8)
    for b, g in enumerate(graphs):
        labels[b, 0], labels[b, 1] = 2, 0
        for i, lab in enumerate(g.labels):
            labels[b, i + 2] = lab + 3
        labels[b, n + 2] = 1
        for u, v in g.edges:
            assert u < v
            parents[b, v + 2] |= np.uint64(1 << (u + 2))
    raw = np.zeros((B, dl.DECODE_STATE_BYTES), np.uint8)
    raw[:, :384] = parents.view(np.uint8).reshape(B, 384)
    raw[:, 384:432] = labels
    nvs = np.full(B, n + 3 if nv is None else nv, np.int32) if np.isscalar(nv) or nv is None else np.asarray(nv, np.int32)
    raw[:, 432:436] = nvs.view(np.uint8).reshape(B, 4)
    raw[:, 436:440] = np.ones(B, np.int32).view(np.uint8).reshape(B, 4)
    return raw


def corpus(judge, seed=7):
    """{(n, card): [(target, decoded)]}: random DAGs with an identical copy, a renumbered copy, one changed edge and two
    swapped labels, plus the WL-equivalent and symmetric families."""
    rng = np.random.default_rng(seed)
    out = {}
    for n in (4, 8, 12, 13, 14, 37, 45):
        for card in sorted({1, 2, 5, n}):
            pairs = []
            for _ in range(2):
                g = random_dag(rng, n, card)
                pairs += [(g, LabeledGraph(list(g.labels), list(g.edges))), (g, topo_permuted(rng, g)),
                          (g, one_edge_changed(rng, g))]
                sw = labels_swapped(rng, g)
                if sw is not None:
                    pairs.append((g, topo_permuted(rng, sw)))
            out[(n, card)] = pairs
    out[(12, 1)] += wl_equivalent_pairs(judge, 6, seed)
    out[(14, 1)] += wl_equivalent_pairs(judge, 7, seed + 1)
    out[(45, 1)] += symmetric_pairs(rng)
    return out
