"""TEST HELPER: cases, references and the checks themselves for structure comparison (csrc/dvs_cpdag.h: dvs_cpdag,
dvs_pdag_compare; dags_vae_search_amd/compare.py), written once and run by tests/test_emu_cpdag.py (emulator build) and
tests/test_gpu_cpdag.py (device).  tests/test_cpdag_ref.py pins the references themselves on the CPU.

References (Python ints, no numpy arithmetic, nothing shared with the kernels)
  cpdag_ref     the rules of include/dvs.h (dvs_cpdag) restated: skeleton, v-structures, Meek's R1 - R3 to a fixpoint with a
                round's orientations applied together.  Also reports which of the rules fired.  R2 is stated with the
                directed-out rows (the kernel states it with the parents of the parents).
  brute_cpdags  all labelled DAGs on n <= 5 vertices grouped by (skeleton, v-structures) (Verma and Pearl: that is Markov
                equivalence); an arc is compelled iff it has one direction in the whole class.
  class_by_reversals  the class of one DAG enumerated by breadth-first covered-edge reversals (Chickering 1995): the second,
                independent route, for n = 8 .. 10.
  compare_ref   the pair states of include/dvs.h (dvs_pdag_compare), pair by pair.
Everything is integers: every device comparison is equality of bytes, there are no tolerances.  There is no R run to pin
against (R is not available to this suite): parity with bnlearn's cpdag / shd / compare rests on the definitions, DESIGN.md
§16.
"""
import functools
import itertools

import numpy as np

from tests import scoring_corpus as sc
from tests.abi_cases import call, entry, run

U64 = np.uint64
RULES = ("R1", "R2", "R3")
CLASS_COUNTS = {3: 11, 4: 185, 5: 8782}
DAG_COUNTS = {3: 25, 4: 543, 5: 29281}


def bits(m):
    m = int(m)
    while m:
        low = m & -m
        yield low.bit_length() - 1
        m ^= low


def children_rows(P):
    n = len(P)
    return [sum(1 << w for w in range(n) if (int(P[w]) >> v) & 1) for v in range(n)]


# ---------------------------------------------------------------------------------------------------------------------
# cpdag_ref
# ---------------------------------------------------------------------------------------------------------------------
def cpdag_ref(P, rules=RULES):
    """(pdag rows as ints, the set of rules that fired).  `rules`: the rules in force (the pins drop one to show that each is
    needed)."""
    n = len(P)
    P = [int(x) for x in P]
    ch = children_rows(P)
    adj = [P[v] | ch[v] for v in range(n)]
    D = [0] * n                                                  # directed in
    for v in range(n):
        for u in bits(P[v]):
            if P[v] & ~adj[u] & ~(1 << u):
                D[v] |= 1 << u
    Dout = children_rows(D)
    U = [adj[v] & ~D[v] & ~Dout[v] for v in range(n)]
    fired = set()
    for _ in range(n * (n - 1) // 2 + 1):
        O = [0] * n
        for v in range(n):
            for u in bits(U[v]):
                S = U[u] & D[v]
                why = []
                if D[u] & ~adj[v] & ~(1 << v):
                    why.append("R1")
                if Dout[u] & D[v]:
                    why.append("R2")
                if any(S & ~adj[w] & ~(1 << w) for w in bits(S)):
                    why.append("R3")
                why = [r for r in why if r in rules]
                if why:
                    fired.update(why)
                    O[v] |= 1 << u
        if not any(O):
            break
        for v in range(n):
            D[v] |= O[v]
            U[v] &= ~O[v]
            for u in bits(O[v]):
                U[u] &= ~(1 << v)
        Dout = children_rows(D)
    else:
        raise AssertionError("cpdag_ref: no fixpoint within n (n - 1) / 2 + 1 rounds")
    return [D[v] | U[v] for v in range(n)], fired


def flags_ref(P):
    """dvs_cpdag's flag of one row set"""
    n = len(P)
    P = [int(x) for x in P]
    if any(P[v] >> n or (P[v] >> v) & 1 for v in range(n)):
        return 2
    reach = list(P)
    for k in range(n):
        for v in range(n):
            if (reach[v] >> k) & 1:
                reach[v] |= reach[k]
    return 1 if any((reach[v] >> v) & 1 for v in range(n)) else 0


# ---------------------------------------------------------------------------------------------------------------------
# Brute force, n <= 5
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_dags(n):
    """every labelled DAG on n vertices as a tuple of parent rows, in a fixed order"""
    pairs = list(itertools.combinations(range(n), 2))
    out = []
    for states in itertools.product(range(3), repeat=len(pairs)):
        P = [0] * n
        for (u, v), s in zip(pairs, states):
            if s == 1:
                P[v] |= 1 << u
            elif s == 2:
                P[u] |= 1 << v
        if flags_ref(P) == 0:
            out.append(tuple(P))
    assert len(out) == DAG_COUNTS[n], (n, len(out))
    return out


def class_key(P):
    """(skeleton, v-structures): equal exactly for Markov equivalent DAGs"""
    n = len(P)
    ch = children_rows(P)
    adj = tuple(int(P[v]) | ch[v] for v in range(n))
    vs = frozenset((a, v, b) for v in range(n) for a in bits(P[v]) for b in bits(P[v]) if a < b and not (adj[a] >> b) & 1)
    return adj, vs


def compelled_rows(members):
    """the CPDAG rows of a class given all its members: u -> v stays directed iff every member has it"""
    n = len(members[0])
    every = [functools.reduce(lambda x, y: x & y, (m[v] for m in members)) for v in range(n)]
    ch = children_rows(members[0])
    adj = [int(members[0][v]) | ch[v] for v in range(n)]
    every_out = children_rows(every)
    return [every[v] | (adj[v] & ~every[v] & ~every_out[v]) for v in range(n)]


@functools.lru_cache(maxsize=None)
def brute_cpdags(n):
    """{dag: its CPDAG rows} over all_dags(n), and the number of classes"""
    classes = {}
    for P in all_dags(n):
        classes.setdefault(class_key(P), []).append(P)
    out = {}
    for members in classes.values():
        rows = tuple(compelled_rows(members))
        for P in members:
            out[P] = rows
    return out, len(classes)


@functools.lru_cache(maxsize=None)
def ref_all(n):
    """[(rows, fired)] of cpdag_ref over all_dags(n), computed once"""
    return [cpdag_ref(P) for P in all_dags(n)]


# ---------------------------------------------------------------------------------------------------------------------
# Chickering: the class by covered-edge reversals
# ---------------------------------------------------------------------------------------------------------------------
def covered_edges(P):
    """[(u, v)] with u -> v and P[v] = P[u] + {u}"""
    return [(u, v) for v in range(len(P)) for u in bits(P[v]) if int(P[v]) == int(P[u]) | (1 << u)]


def reverse_edge(P, u, v):
    Q = [int(x) for x in P]
    Q[v] &= ~(1 << u)
    Q[u] |= 1 << v
    return Q


def class_by_reversals(P, limit=20000):
    """all members of P's class, or None when there are more than `limit`"""
    start = tuple(int(x) for x in P)
    seen, frontier = {start}, [start]
    while frontier:
        nxt = []
        for Q in frontier:
            for u, v in covered_edges(Q):
                R = tuple(reverse_edge(Q, u, v))
                if R not in seen:
                    seen.add(R)
                    nxt.append(R)
        if len(seen) > limit:
            return None
        frontier = nxt
    return sorted(seen)


# ---------------------------------------------------------------------------------------------------------------------
# compare_ref
# ---------------------------------------------------------------------------------------------------------------------
def pair_state(M, u, v):
    """0 none, 1 u -> v, 2 v -> u, 3 undirected, for u < v"""
    return ((int(M[v]) >> u) & 1) | (((int(M[u]) >> v) & 1) << 1)


def compare_ref(A, T):
    """(shd, tp, fp, fn, hamming) of the learned rows A against the target rows T"""
    n = len(A)
    shd = tp = fp = fn = ham = 0
    for u, v in itertools.combinations(range(n), 2):
        a, t = pair_state(A, u, v), pair_state(T, u, v)
        shd += a != t
        tp += a != 0 and a == t
        fp += a != 0 and a != t
        fn += t != 0 and a != t
        ham += (a != 0) != (t != 0)
    return shd, tp, fp, fn, ham


def n_edges(M):
    return sum(pair_state(M, u, v) != 0 for u, v in itertools.combinations(range(len(M)), 2))


# ---------------------------------------------------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------------------------------------------------
def random_dags(n, count, density, seed):
    """u64 [count, n]: each edge of a random topological order with probability `density`, the order a random permutation
    of the variable indices (a parent's index may be above its child's)"""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, n), U64)
    for b in range(count):
        order = [int(x) for x in rng.permutation(n)]
        for k in range(1, n):
            for j in range(k):
                if rng.random() < density:
                    out[b, order[k]] |= U64(1) << U64(order[j])
    return out


def random_pdags(n, count, seed):
    """u64 [count, n]: every pair in one of the four states, absent about half the time"""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, n), U64)
    for b in range(count):
        for u, v in itertools.combinations(range(n), 2):
            s = int(rng.choice([0, 0, 0, 1, 2, 3]))
            if s & 1:
                out[b, v] |= U64(1) << U64(u)
            if s & 2:
                out[b, u] |= U64(1) << U64(v)
    return out


SPARSE = lambda n: min(0.5, 2.5 / max(n - 1, 1))                   # about 1.25 n edges
RANDOM_SIZES = (1, 2, 17, 33, 48)
RANDOM_COUNT = 64


def as_rows(list_of_rows):
    return np.array([[int(x) for x in rows] for rows in list_of_rows], U64)


# ---------------------------------------------------------------------------------------------------------------------
# Drivers: the two calls through the raw C ABI on a back end of scoring_corpus (numpy in place on the emulator, torch
# tensors on the device)
# ---------------------------------------------------------------------------------------------------------------------
class Driver:
    def __init__(self, be):
        self.be, self.lib = be, be.lib

    def cpdag(self, P):
        """one dvs_cpdag -> (pdag u64 [B, n], flags i32 [B]); the output buffers start as garbage"""
        be = self.be
        P = np.ascontiguousarray(P, U64)
        B, n = P.shape
        hP, out, fl = be.put(P), be.put(np.full((B, n), 0xA5A5A5A5A5A5A5A5, U64)), be.put(np.full(B, -7, np.int32))
        call(be, "dvs_cpdag", batch=B, n_vars=n, parents=hP, pdag=out, pdag_bytes=B * n * 8, flags=fl)
        res = be.get(out).copy(), be.get(fl).copy()
        assert be.get(hP).tobytes() == P.tobytes()                 # the input is not written
        return res

    def compare(self, A, T):
        """one dvs_pdag_compare -> counts i32 [B, 5]; T is [B, n] or [1, n]"""
        be = self.be
        A, T = np.ascontiguousarray(A, U64), np.ascontiguousarray(T, U64)
        B, n = A.shape
        hA, hT, out = be.put(A), be.put(T), be.put(np.full((B, 5), -7, np.int32))
        call(be, "dvs_pdag_compare", batch=B, n_vars=n, a=hA, b=hT, b_rows=T.shape[0], counts=out, counts_bytes=B * 20)
        return be.get(out).copy()


# ---------------------------------------------------------------------------------------------------------------------
# 1. dvs_cpdag against cpdag_ref, bytewise
# ---------------------------------------------------------------------------------------------------------------------
def check_all_dags(drv, n):
    """every labelled DAG of n vertices in one launch; by the reference's report each rule fires among them"""
    dags, ref = all_dags(n), ref_all(n)
    P = as_rows(dags)
    assert len(P) % 4 != 0                                         # 543 and 29 281: a ragged last workgroup
    assert set().union(*(f for _, f in ref)) == set(RULES)
    got, fl = drv.cpdag(P)
    assert not fl.any()
    want = as_rows([r[0] for r in ref])
    bad = np.nonzero((got != want).any(1))[0]
    assert got.tobytes() == want.tobytes(), (n, len(bad), [(P[b].tolist(), got[b].tolist(), want[b].tolist()) for b in bad[:3]])
    return len(P)


def check_random(drv, n):
    """seeded random DAGs in permuted variable order, sparse and density 0.5; from n = 5 on every rule fires at this size"""
    fired = set()
    for k, density in enumerate((SPARSE(n), 0.5)):
        P = random_dags(n, RANDOM_COUNT, density, seed=1000 * n + k)
        ref = [cpdag_ref(row) for row in P]
        got, fl = drv.cpdag(P)
        assert not fl.any()
        assert got.tobytes() == as_rows([r[0] for r in ref]).tobytes(), (n, density)
        fired.update(*(r[1] for r in ref))
    if n >= 5:
        assert fired == set(RULES), (n, fired)
    return fired


def check_extremes(drv):
    """the complete order on 48 vertices: everything is undirected; the empty graph"""
    n = 48
    order = np.array([[(1 << v) - 1 for v in range(n)]], U64)
    got, fl = drv.cpdag(order)
    full = (1 << n) - 1
    assert fl[0] == 0 and got[0].tolist() == [full & ~(1 << v) for v in range(n)] == cpdag_ref(order[0])[0]
    for m in (1, 5, 48):
        got, fl = drv.cpdag(np.zeros((3, m), U64))
        assert not fl.any() and not got.any()


def check_covered_edge(drv, n):
    """reversing one covered edge (P[v] = P[u] + {u}) stays in the class: the output bytes do not change"""
    P = random_dags(n, 24, SPARSE(n), seed=77 + n)
    Q = P.copy()
    reversed_rows = 0
    for b in range(len(P)):
        cov = covered_edges(P[b])
        if cov:
            u, v = cov[b % len(cov)]
            Q[b] = np.array(reverse_edge(P[b], u, v), U64)
            reversed_rows += 1
    assert reversed_rows >= len(P) // 2 and not np.array_equal(P, Q)
    a, fa = drv.cpdag(P)
    c, fc = drv.cpdag(Q)
    assert not fa.any() and not fc.any() and a.tobytes() == c.tobytes()


def check_flags(drv):
    """a 2-cycle (flag 1), a self-loop (2), a bit >= n (2), a longer cycle (1), each between clean rows whose output is that
    of a launch without the bad rows; flagged rows give zero output"""
    for n in (5, 33):
        clean = random_dags(n, 9, 0.5 if n == 5 else SPARSE(n), seed=300 + n)
        alone, fl = drv.cpdag(clean)
        assert not fl.any()
        P = clean.copy()
        P[1] = 0
        P[1, 0], P[1, 1] = U64(1 << 1), U64(1 << 0)                        # 0 <-> 1
        P[3, 2] |= U64(1 << 2)                                              # a self-loop
        P[5, n - 1] |= U64(1) << U64(n)                                     # a bit >= n
        P[7] = 0
        P[7, 0], P[7, n - 1], P[7, 2] = U64(1) << U64(n - 1), U64(1 << 2), U64(1 << 0)   # 0 -> 2 -> n-1 -> 0
        bad = {1: 1, 3: 2, 5: 2, 7: 1}
        got, fl = drv.cpdag(P)
        assert fl.tolist() == [bad.get(b, 0) for b in range(9)] == [flags_ref(row) for row in P]
        for b in range(9):
            assert got[b].tobytes() == (np.zeros(n, U64) if b in bad else alone[b]).tobytes(), (n, b)
    P = np.array([[1 << 63], [0], [1]], U64)                              # n = 1: a high bit, clean, a self-loop
    got, fl = drv.cpdag(P)
    assert fl.tolist() == [2, 0, 2] and not got.any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. dvs_pdag_compare against compare_ref
# ---------------------------------------------------------------------------------------------------------------------
def hand_pairs():
    """[(name, learned rows, target rows, (shd, tp, fp, fn, hamming))] on 4 vertices around the target 0 -> 1, 1 - 2, 2 -> 3"""
    m = lambda d: sc.masks_of(4, d)[0]
    target = m({1: [0, 2], 2: [1], 3: [2]})
    return [
        ("identical", target, target, (0, 3, 0, 0, 0)),
        ("one reversed", m({0: [1], 1: [2], 2: [1], 3: [2]}), target, (1, 2, 1, 1, 0)),
        ("directed against undirected", m({1: [0, 2], 3: [2]}), target, (1, 2, 1, 1, 0)),
        ("undirected against directed", m({1: [0, 2], 2: [1, 3], 3: [2]}), target, (1, 2, 1, 1, 0)),
        ("missing", m({1: [0, 2], 2: [1]}), target, (1, 2, 0, 1, 1)),
        ("extra", m({1: [0, 2], 2: [1], 3: [2, 0]}), target, (1, 3, 1, 0, 1)),
        ("nothing learned", m({}), target, (3, 0, 0, 3, 3)),
    ]


def check_compare_hand(drv):
    cases = hand_pairs()
    A, T = np.stack([c[1] for c in cases]), np.stack([c[2] for c in cases])
    got = drv.compare(A, T)
    for b, (name, a, t, want) in enumerate(cases):
        assert compare_ref(a, t) == want, name
        assert tuple(got[b].tolist()) == want, (name, got[b].tolist())


def check_compare_random(drv, n, count=37):
    A, T = random_pdags(n, count, seed=40 + n), random_pdags(n, count, seed=90 + n)
    want = np.array([compare_ref(a, t) for a, t in zip(A, T)], np.int32)
    got = drv.compare(A, T)
    assert got.tobytes() == want.tobytes(), n
    assert all(want[b, 1] + want[b, 3] == n_edges(T[b]) and want[b, 1] + want[b, 2] == n_edges(A[b]) for b in range(count))
    # one target for the batch is the tiled target
    assert drv.compare(A, T[:1]).tobytes() == drv.compare(A, np.repeat(T[:1], count, 0)).tobytes()
    assert drv.compare(A, T[:1]).tobytes() == np.array([compare_ref(a, T[0]) for a in A], np.int32).tobytes()
    # the sides swapped: shd and hamming stay, fp and fn change places, tp stays
    assert drv.compare(T, A).tobytes() == want[:, [0, 1, 3, 2, 4]].tobytes()
    # stray bits >= n and the diagonal change nothing
    A2, T2 = A.copy(), T.copy()
    for v in range(n):
        A2[:, v] |= U64(1) << U64(v)
        T2[::2, v] |= U64(1) << U64(v)
    A2[:, 0] |= U64(0xFFFF) << U64(48)
    T2[:, n - 1] |= ~U64(0) << U64(n)
    assert drv.compare(A2, T2).tobytes() == want.tobytes()
    return int(want[:, 0].max())


# ---------------------------------------------------------------------------------------------------------------------
# 4. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    """(entry point, arguments, return code, text dvs_last_error must contain): every check of both entry points, and the
    pairs where two checks fail and the earlier one decides.  D: a dummy non-null pointer, never dereferenced."""
    cases = []

    c = entry("dvs_cpdag", cases, batch=8, n_vars=12, parents=D, pdag=D, pdag_bytes=768, flags=D, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(2, "batch must be > 0", batch=-3)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars must be < 2^31", batch=1 << 26, n_vars=32, pdag_bytes=1 << 40)
    c(10, "null pointer", parents=None)
    c(10, "null pointer", pdag=None)
    c(10, "null pointer", flags=None)
    c(14, "pdag_bytes < batch * n_vars * 8 = 768", pdag_bytes=767)
    c(2, "batch must be > 0", batch=0, n_vars=49)                                      # batch before n_vars
    c(3, "n_vars must be in [1, 48]", batch=1 << 30, n_vars=49)                        # n_vars before the product
    c(2, "batch * n_vars must be < 2^31", batch=1 << 26, n_vars=32, parents=None)      # the product before null
    c(10, "null pointer", flags=None, pdag_bytes=0)                                    # null before pdag_bytes

    c = entry("dvs_pdag_compare", cases, batch=8, n_vars=12, a=D, b=D, b_rows=8, counts=D, counts_bytes=160, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars must be < 2^31", batch=1 << 26, n_vars=32, b_rows=1, counts_bytes=1 << 40)
    c(10, "null pointer", a=None)
    c(10, "null pointer", b=None)
    c(10, "null pointer", counts=None)
    c(12, "b_rows must be 1 or batch", b_rows=0)
    c(12, "b_rows must be 1 or batch", b_rows=7)
    c(14, "counts_bytes < batch * 20 = 160", counts_bytes=159)
    c(14, "counts_bytes < batch * 20 = 160", b_rows=1, counts_bytes=159)
    c(2, "batch must be > 0", batch=0, n_vars=49)                                      # batch before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, a=None)                               # range before null
    c(2, "batch * n_vars must be < 2^31", batch=1 << 26, n_vars=32, b=None)            # the product before null
    c(10, "null pointer", b=None, b_rows=3)                                            # null before b_rows
    c(12, "b_rows must be 1 or batch", b_rows=2, counts_bytes=0)                       # b_rows before counts_bytes
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_cpdag", "dvs_pdag_compare"}
    run(lib, cases)
