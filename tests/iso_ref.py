"""TEST HELPER: a small exact isomorphism judge for labelled directed graphs, pure Python (no networkx).

Same contract as ``LabeledDag.graph_equals`` / ``is_valid_graph``: graphs are LabeledGraph objects or (labels, edges) pairs,
None is never equal.  Backtracking over target vertices, most-constrained first, with candidates filtered by (in-degree,
out-degree[, label]) and consistency with the partial mapping; a complete mapping is an isomorphism by construction."""
from dags_vae_search_amd.features import _as_labels_edges


def graph_equals(g1, g2, attributes_match=True):
    if g1 is None or g2 is None:
        return False
    l1, e1 = _as_labels_edges(g1)
    l2, e2 = _as_labels_edges(g2)
    n = len(l1)
    if n != len(l2) or len(e1) != len(e2):
        return False
    if attributes_match and sorted(l1) != sorted(l2):
        return False
    E1, E2 = set(map(tuple, e1)), set(map(tuple, e2))
    if len(E1) != len(E2):
        return False

    def adj(E):
        par = [set() for _ in range(n)]
        chi = [set() for _ in range(n)]
        for u, v in E:
            chi[u].add(v)
            par[v].add(u)
        return par, chi

    p1, c1 = adj(E1)
    p2, c2 = adj(E2)

    def sig(i, par, chi, lab):
        return (len(par[i]), len(chi[i]), lab[i] if attributes_match else 0)

    s1 = [sig(i, p1, c1, l1) for i in range(n)]
    s2 = [sig(i, p2, c2, l2) for i in range(n)]
    if sorted(s1) != sorted(s2):
        return False
    m, inv = {}, {}

    def order():
        seq, placed = [], set()
        while len(seq) < n:
            best = min((v for v in range(n) if v not in placed),
                       key=lambda v: (-len((p1[v] | c1[v]) & placed), sum(x == s1[v] for x in s1), v))
            seq.append(best)
            placed.add(best)
        return seq

    seq = order()

    def ok(v, w):
        if s1[v] != s2[w] or ((v, v) in E1) != ((w, w) in E2):
            return False
        for u, x in m.items():
            if ((u, v) in E1) != ((x, w) in E2) or ((v, u) in E1) != ((w, x) in E2):
                return False
        return True

    def rec(d):
        if d == n:
            return True
        v = seq[d]
        for w in range(n):
            if w not in inv and ok(v, w):
                m[v], inv[w] = w, v
                if rec(d + 1):
                    return True
                del m[v], inv[w]
        return False

    return rec(0)

