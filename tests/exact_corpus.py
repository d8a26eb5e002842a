"""TEST HELPER: cases, references and the checks themselves for exact structure search (csrc/dvs_exact.h:
dvs_exact_workspace_bytes, dvs_exact_search; dags_vae_search_amd/exact.py), written once and run by tests/test_emu_exact.py
(emulator build) and tests/test_gpu_exact.py (device).  tests/test_exact_ref.py pins the references themselves on the CPU.

References (numpy and plain Python, nothing shared with the kernels)
  ref_best_brute  the best-parents definition of include/dvs.h by direct enumeration of the subsets of S, n <= 8.
  ref_dp          the whole dynamic programme restated with the same orders and the same single additions; its best-parents
                  stage is the vectorised sweep over the bits, pinned against ref_best_brute.
  ref_all_dags    the maximum over every labelled DAG (tests/cpdag_corpus.all_dags) of the sum of its table cells, filtered
                  by the cap and the blacklist, n <= 5.
Every device comparison is equality of bytes.  The only tolerance is that of the real-data checks,
    tau = 2 (n - 1) 2^-53 sum_v |L_v|,
the bound on two fp64 sums of the same n terms in different orders ((n - 1) additions each, every one rounding a partial sum
of magnitude <= sum |L_v| by half an ulp).  fp64 addition is monotone, so the programme's value dominates the sink-order sum
of any admissible DAG's cells; tau covers the reordering.  There is no external exact solver to pin against.

Sizes of the byte checks (BYTES_SIZES): k_exact_best takes ceil(n / 8) LDS passes, so 8 is the last size whose whole table
is one tile and 9 the first with a cross-tile pass (5 + 4 bits), 17 the first with three (6 + 6 + 5); k_exact_sinks walks all
levels in one workgroup up to n = 9 and takes one launch per level from 10 on; 6, 12 and 14 are sizes the issue names.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

from tests import bn_score_corpus as bn
from tests import cpdag_corpus as cp
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc
from tests.abi_cases import call, entry, run

U64 = np.uint64
NO_ARG = 0xFFFFFFFF
INF = float("inf")
MAX_VARS = 20
BYTES_SIZES = (6, 8, 9, 10, 12, 14, 17)
BIG = 17                     # only the plain random table, batch 1: 2.2 M cells
KINDS = ("random", "ties", "nan")
SETTINGS = {"random": (None, False), "ties": (3, True), "nan": (None, False)}        # kind -> (max_parents, a blacklist)


def popcounts(n):
    S = np.arange(1 << n, dtype=np.int64)
    return sum((S >> u) & 1 for u in range(n))


def admissible(n, max_parents, forbidden, table):
    """bool [2^n, n]: P = row is admissible for v = column"""
    S = np.arange(1 << n, dtype=np.int64)
    ok = ~np.isnan(table)
    for v in range(n):
        ok[:, v] &= ((S >> v) & 1) == 0
        if forbidden is not None:
            ok[:, v] &= (S & np.int64(int(forbidden[v]) & ((1 << n) - 1))) == 0
    if max_parents is not None and max_parents > 0:
        ok &= (popcounts(n) <= max_parents)[:, None]
    return ok


# ---------------------------------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------------------------------
def ref_best_brute(table, max_parents=None, forbidden=None):
    """(best f64 [2^n, n], arg int64 [2^n, n]) by enumerating the subsets of every S; cells with v in S are (nan, -1)"""
    rows, n = table.shape
    assert rows == 1 << n and n <= 8
    ok = admissible(n, max_parents, forbidden, table)
    best, arg = np.full((rows, n), np.nan), np.full((rows, n), -1, np.int64)
    for S in range(rows):
        for v in range(n):
            if (S >> v) & 1:
                continue
            top, at = -INF, NO_ARG
            P = S
            while True:                                   # every subset of S
                if ok[P, v] and (table[P, v] > top or (table[P, v] == top and P < at)):
                    top, at = table[P, v], P
                if P == 0:
                    break
                P = (P - 1) & S
            best[S, v], arg[S, v] = top, at
    return best, arg


def ref_dp(table, max_parents=None, forbidden=None):
    """the dynamic programme of include/dvs.h (dvs_exact_search) -> namespace(best, arg, R, sink, parents, order, score, flag)"""
    rows, n = table.shape
    assert rows == 1 << n
    ok = admissible(n, max_parents, forbidden, table)
    S = np.arange(rows, dtype=np.int64)
    best = np.where(ok, table, -INF)
    arg = np.where(ok, S[:, None], NO_ARG)
    for i in range(n):
        into = S[(S >> i) & 1 == 1]
        src = into ^ (1 << i)
        take = (best[src] > best[into]) | ((best[src] == best[into]) & (arg[src] < arg[into]))
        best[into] = np.where(take, best[src], best[into])
        arg[into] = np.where(take, arg[src], arg[into])
    pop = popcounts(n)
    R, sink = np.zeros(rows), np.full(rows, -1, np.int32)
    for k in range(1, n + 1):
        W = S[pop == k]
        top, at = np.zeros(len(W)), np.full(len(W), -1, np.int32)
        for s in range(n):
            has = (W >> s) & 1 == 1
            prev = W[has] ^ (1 << s)
            cand = R[prev] + best[prev, s]
            take = (at[has] < 0) | (cand > top[has])
            idx = np.nonzero(has)[0][take]
            top[idx], at[idx] = cand[take], s
        R[W], sink[W] = top, at
    W = rows - 1
    score = R[W]
    parents, order = np.zeros(n, U64), np.full(n, -1, np.int32)
    flag = int(score == -INF)
    if not flag:
        for k in range(n - 1, -1, -1):
            s = int(sink[W])
            W ^= 1 << s
            order[k] = s
            parents[s] = U64(int(arg[W, s]))
    return SimpleNamespace(best=best, arg=arg.astype(np.uint32), R=R, sink=sink, parents=parents, order=order, score=score, flag=flag)


@functools.lru_cache(maxsize=None)
def dag_rows(n):
    """int64 [DAGs, n]: every labelled DAG on n vertices (tests/cpdag_corpus.all_dags; its count table starts at 3)"""
    if n in cp.DAG_COUNTS:
        return np.array(cp.all_dags(n), np.int64)
    pairs = list(itertools.combinations(range(n), 2))
    out = []
    for states in itertools.product(range(3), repeat=len(pairs)):
        P = [0] * n
        for (u, v), s in zip(pairs, states):
            if s == 1:
                P[v] |= 1 << u
            elif s == 2:
                P[u] |= 1 << v
        if cp.flags_ref(P) == 0:
            out.append(P)
    assert len(out) == {1: 1, 2: 3}[n]
    return np.array(out, np.int64)


def ref_all_dags(table, max_parents=None, forbidden=None):
    """the largest sum of cells over all labelled DAGs that respect the cap and the blacklist (tables of small integers: every
    sum is exact whatever its order)"""
    rows, n = table.shape
    D = dag_rows(n)
    ok = admissible(n, max_parents, forbidden, table)
    fine = np.ones(len(D), bool)
    total = np.zeros(len(D))
    for v in range(n):
        fine &= ok[D[:, v], v]
        total += table[D[:, v], v]
    return float(total[fine].max())


# ---------------------------------------------------------------------------------------------------------------------
# Driver: dvs_exact_search through the raw C ABI on a back end of scoring_corpus
# ---------------------------------------------------------------------------------------------------------------------
def layout(batch, n):
    """byte offsets of best, arg, R, sink and the total, as include/dvs.h documents them"""
    up = lambda x: (x + 255) & ~255
    subsets = batch << n
    cells = subsets * n
    arg = up(cells * 8)
    R = arg + up(cells * 4)
    sink = R + up(subsets * 8)
    return 0, arg, R, sink, sink + up(subsets * 4)


class Driver:
    def __init__(self, be):
        self.be, self.lib = be, be.lib

    def search(self, tables, max_parents=None, forbidden=None):
        """one dvs_exact_search on f64 [B, 2^n, n] -> every output and every stage of the workspace; all buffers start as
        a byte pattern"""
        be, lib = self.be, self.lib
        tables = np.ascontiguousarray(tables, np.float64)
        B, rows, n = tables.shape
        assert rows == 1 << n
        o_best, o_arg, o_R, o_sink, total = layout(B, n)
        assert lib.dvs_exact_workspace_bytes(B, n) == total
        hT, ws = be.put(tables), be.put(np.full(total, 0xA5, np.uint8))
        hp, ho = be.put(np.full((B, n), 0xA5A5A5A5A5A5A5A5, U64)), be.put(np.full((B, n), -7, np.int32))
        hs, hf = be.put(np.full(B, -7.0)), be.put(np.full(B, -7, np.int32))
        forb = None if forbidden is None else be.put(np.ascontiguousarray(forbidden, U64))
        call(be, "dvs_exact_search", batch=B, n_vars=n, table=hT, table_bytes=tables.nbytes, max_parents=max_parents or 0,
             forbidden=forb, workspace=ws, workspace_bytes=total, parents=hp, order=ho, score=hs, flags=hf)
        w = be.get(ws).copy()
        assert be.get(hT).tobytes() == tables.tobytes()                    # the input is not written
        cells = B * rows * n
        return SimpleNamespace(
            ws=w, best=w[o_best:o_best + cells * 8].view(np.float64).reshape(B, rows, n),
            arg=w[o_arg:o_arg + cells * 4].view(np.uint32).reshape(B, rows, n),
            R=w[o_R:o_R + B * rows * 8].view(np.float64).reshape(B, rows),
            sink=w[o_sink:o_sink + B * rows * 4].view(np.int32).reshape(B, rows),
            parents=be.get(hp).copy(), order=be.get(ho).copy(), score=be.get(hs).copy(), flags=be.get(hf).copy())


OUTPUTS = ("ws", "parents", "order", "score", "flags")


def same_bytes(a, b, fields=OUTPUTS):
    return all(getattr(a, f).tobytes() == getattr(b, f).tobytes() for f in fields)


def row_of(r, t):
    """table t of a batched result, as a result of batch 1 (the workspace itself is laid out by batch: not comparable)"""
    return SimpleNamespace(**{f: getattr(r, f)[t:t + 1] for f in ("best", "arg", "R", "sink", "parents", "order", "score", "flags")})


STAGES = ("best", "arg", "R", "sink", "parents", "order", "score", "flags")


def free_cells(n):
    """bool [2^n, n]: v not in S, the cells of best / arg that are specified"""
    S = np.arange(1 << n, dtype=np.int64)
    return ((S[:, None] >> np.arange(n)[None, :]) & 1) == 0


def assert_equals_ref(got, t, ref, n, what):
    free = free_cells(n)
    assert got.best[t][free].tobytes() == ref.best[free].tobytes(), (what, "best")
    assert got.arg[t][free].tobytes() == ref.arg[free].tobytes(), (what, "arg")
    assert got.R[t].tobytes() == ref.R.tobytes(), (what, "R")
    assert got.sink[t].tobytes() == ref.sink.tobytes(), (what, "sink")
    assert got.parents[t].tobytes() == ref.parents.tobytes(), (what, "parents")
    assert got.order[t].tobytes() == ref.order.tobytes(), (what, "order")
    assert got.score[t:t + 1].tobytes() == np.array([ref.score]).tobytes() and int(got.flags[t]) == ref.flag, (what, "score")


# ---------------------------------------------------------------------------------------------------------------------
# Tables
# ---------------------------------------------------------------------------------------------------------------------
def random_forbidden(rng, n, p=0.25):
    f = np.zeros(n, U64)
    for v in range(n):
        for u in range(n):
            if u != v and rng.random() < p:
                f[v] |= U64(1) << U64(u)
    return f


def make_tables(kind, batch, n, seed):
    rng = np.random.default_rng(seed)
    shape = (batch, 1 << n, n)
    if kind == "integers":
        return rng.integers(-9, 10, shape).astype(np.float64)
    if kind == "ties":                                     # three values: ties in nearly every comparison of both stages
        return rng.choice(np.array([-1.5, 0.25, 2.0]), shape)
    t = rng.standard_normal(shape) * 100.0
    if kind == "nan":
        t[rng.random(shape) < 0.15] = np.nan
        t[:, 0, :] = rng.standard_normal((batch, n))      # the empty parent set stays available: no flag here
    return t


# ---------------------------------------------------------------------------------------------------------------------
# 1. Optimality against brute force, exactly
# ---------------------------------------------------------------------------------------------------------------------
OPT_TABLES = 36


def check_optimal(drv, n):
    """integer tables, one batched call per (cap, blacklist): score == ref_all_dags bytewise, parents acyclic, admissible and
    attaining score, order topological"""
    rng = np.random.default_rng(50 + n)
    tables = make_tables("integers", OPT_TABLES, n, seed=60 + n)
    runs = 0
    for cap in (None, 1, 2):
        for forb in (None, random_forbidden(rng, n)):
            got = drv.search(tables, cap, forb)
            assert not got.flags.any()
            for t in range(OPT_TABLES):
                want = ref_all_dags(tables[t], cap, forb)
                assert np.array([want]).tobytes() == got.score[t:t + 1].tobytes(), (n, cap, t, want, got.score[t])
                P = [int(x) for x in got.parents[t]]
                assert cp.flags_ref(P) == 0
                ok = admissible(n, cap, forb, tables[t])
                assert all(ok[P[v], v] for v in range(n))
                assert sum(tables[t][P[v], v] for v in range(n)) == want
                seen = 0
                for k in range(n):
                    v = int(got.order[t, k])
                    assert 0 <= v < n and not (seen >> v) & 1 and P[v] & ~seen == 0, (n, cap, t, got.order[t], P)
                    seen |= 1 << v
            runs += 1
    return runs


# ---------------------------------------------------------------------------------------------------------------------
# 2. Bytes against ref_dp; a batch is its rows; 6. determinism
# ---------------------------------------------------------------------------------------------------------------------
def check_bytes(drv, n, kind):
    """batch 3 and batch 1 (n = 17: batch 1 only): every stage equals ref_dp, a batch's outputs equal its rows run alone, and
    a second call gives equal bytes in every output and in the whole workspace"""
    cap, with_forb = SETTINGS[kind]
    batch = 1 if n >= BIG else 3
    tables = make_tables(kind, batch, n, seed=1000 * n + KINDS.index(kind))
    forb = random_forbidden(np.random.default_rng(n), n, 0.15) if with_forb else None
    got = drv.search(tables, cap, forb)
    assert not got.flags.any()
    refs = [ref_dp(tables[t], cap, forb) for t in range(batch)]
    for t in range(batch):
        assert_equals_ref(got, t, refs[t], n, (n, kind, t))
    assert same_bytes(got, drv.search(tables, cap, forb))
    if batch > 1:
        for t in range(batch):
            alone = drv.search(tables[t:t + 1], cap, forb)
            assert same_bytes(row_of(got, t), alone, STAGES), (n, kind, t)
    if kind == "ties":
        # both tie rules decided something: S itself attains best[S][v] and a smaller mask was taken; a sink above the lowest bit
        ok = admissible(n, cap, forb, tables[0]) & (tables[0] == refs[0].best)
        assert (refs[0].arg[ok] != np.nonzero(ok)[0]).any()
        assert (refs[0].sink[1:] != [int(W & -W).bit_length() - 1 for W in range(1, 1 << n)]).any()
    return batch


# ---------------------------------------------------------------------------------------------------------------------
# 3. Flags
# ---------------------------------------------------------------------------------------------------------------------
def check_flags(drv, n):
    """Table 1 of 3 has no available family for one variable v (its whole column is NaN, table[0][v] included): flag 1, -inf,
    zero parents, order -1, for that table alone.  With only table[0][v] NaN and n > 1 the definitions of include/dvs.h give
    best[0][v] = -inf alone: v still has admissible non-empty parent sets, so a DAG exists, v is not the first of the order
    and no flag is set; at n = 1 that one cell is the whole column."""
    v = n // 2
    tables = make_tables("random", 3, n, seed=7 + n)
    clean = drv.search(tables)
    free = free_cells(n)[:, v]
    tables[1, 0, v] = np.nan
    got = drv.search(tables)
    assert_equals_ref(got, 1, ref_dp(tables[1]), n, ("empty set only", n))
    assert got.best[1][0, v] == -INF and got.arg[1][0, v] == NO_ARG
    if n > 1:
        assert got.flags.tolist() == [0, 0, 0] and got.order[1, 0] != v and np.isfinite(got.best[1][1:, v][free[1:]]).all()
    tables[1, :, v] = np.nan
    got = drv.search(tables)
    assert got.flags.tolist() == [0, 1, 0]
    assert got.score[1] == -INF and not got.parents[1].any() and (got.order[1] == -1).all()
    assert (got.best[1][:, v][free] == -INF).all() and (got.arg[1][:, v][free] == NO_ARG).all()
    for t in (0, 2):
        assert same_bytes(row_of(got, t), row_of(clean, t), STAGES)
    assert_equals_ref(got, 1, ref_dp(tables[1]), n, ("flags", n))


# ---------------------------------------------------------------------------------------------------------------------
# 4. Real data.  A `Real` driver builds the local-score table, scores masks, searches and runs the two heuristics: on the
#    emulator through the raw C ABI (EmuReal), on the device through the package (test_gpu_exact.GpuReal).
# ---------------------------------------------------------------------------------------------------------------------
REAL_TYPES = (("bic", None), ("bde", 10.0), ("k2", None), ("loglik", None))
REAL_CAP = {"asia": 2, "sachs": 3}
SCORED_ROWS = {"asia": 93, "sachs": 562}                     # popcount(S) <= cap + 1
SAMPLE_CELLS = 300
TABU_LEN, TABU_STEPS = 10, 60


def scored_rows(n, cap):
    return np.nonzero(popcounts(n) <= cap + 1)[0] if cap is not None and cap + 1 < n else np.arange(1 << n)


def row_masks(rows, n):
    """u64 [len(rows), n]: row S holds parents[v] = S & ~(1 << v)"""
    return (np.asarray(rows, np.int64)[:, None] & ~(np.int64(1) << np.arange(n, dtype=np.int64))[None, :]).astype(U64)


class EmuReal:
    """raw C ABI of the emulator build: the table by dvs_bn_scores over the scored rows, the searches by the launch sequences
    of tests/hillclimb_corpus.py and tests/tabu_corpus.py"""

    def __init__(self, lib, name, typ, arg):
        from tests import tabu_corpus as tb
        self.case, self.typ, self.arg = hc.hc_case(name), typ, arg
        self.be, self.n = sc.EmuBackend(lib), self.case.data.shape[1]
        self.search_drv = tb.TabuDriver(self.be, self.case, typ, arg)
        self.exact = Driver(self.be)

    def local(self, masks):
        """-> (scores [B], local [B, n])"""
        rc, scratch, out, _ = bn.run_bn(self.be, self.case.data, self.case.card, np.ascontiguousarray(masks, U64), self.typ, self.arg)
        assert rc == 0
        return out, scratch

    def table(self, cap):
        rows = scored_rows(self.n, cap)
        t = np.full((1 << self.n, self.n), np.nan)
        t[rows] = self.local(row_masks(rows, self.n))[1]
        return t

    def search(self, table, cap, forbidden):
        """-> (parents u64 [n], score, rescored, order)"""
        got = self.exact.search(table[None], cap, forbidden)
        assert not got.flags.any()
        return got.parents[0], float(got.score[0]), float(self.local(got.parents)[0][0]), got.order[0]

    def heuristics(self, cap, forbidden):
        """best scores of the greedy climb and of tabu search from the empty graph"""
        start = np.zeros((1, self.n), U64)
        g = self.search_drv.climb(start, self.case.max_steps, cap, forbidden, self.case.min_delta)
        t = self.search_drv.tabu_climb(start, TABU_STEPS, TABU_LEN, TABU_LEN, cap, forbidden, self.case.min_delta)
        return float(g.scores[0]), float(t.best_score[0])


def known_asia(typ, arg):
    """(parent masks u64 [8], float64 oracle score) of the reference's asia network"""
    if typ in ("bic", "bde"):
        score = hc.asia_known_score(typ, arg)[0]
    else:                                                   # the same second evaluation, for the types oracle_local does not take
        case = hc.hc_case("asia")
        score = math.fsum(bn.second_local(bn.cell_counts(case.data, case.card, v, ps), typ, arg) for v, ps in
                          {0: [], **hc.ASIA_KNOWN}.items())
    return sc.masks_of(8, hc.ASIA_KNOWN)[0], score


def tau_of(L, n):
    return 2 * (n - 1) * 2.0 ** -53 * float(np.abs(L).sum())


def check_real(real, name, sample_seed=3):
    """the table cell by cell, the search against ref_dp on that table, the two summation orders, and the optimum against
    hill climbing, tabu search and (asia) the known network"""
    n, cap = real.n, REAL_CAP[name]
    table = real.table(cap)
    rows = scored_rows(n, cap)
    assert len(rows) == SCORED_ROWS[name] and np.isnan(np.delete(table, rows, 0)).all() and not np.isnan(table[rows]).any()
    # sampled cells against score_masks(local=True) of a row holding that parent set in column v and others elsewhere
    rng = np.random.default_rng(sample_seed)
    S, V = rng.choice(rows, SAMPLE_CELLS), rng.integers(0, n, SAMPLE_CELLS)
    masks = np.zeros((SAMPLE_CELLS, n), U64)
    masks[np.arange(SAMPLE_CELLS), V] = row_masks(S, n)[np.arange(SAMPLE_CELLS), V]
    loc = real.local(masks)[1]
    assert loc[np.arange(SAMPLE_CELLS), V].tobytes() == table[S, V].tobytes()
    forb = None
    if name == "asia":                                      # the blacklist of the hill-climb corpus' "forbidden" case
        forb = hc.hc_case("forbidden").forbidden
    out = {}
    for fb in ([None, forb] if forb is not None else [None]):
        parents, score, rescored, order = real.search(table, cap, fb)
        ref = ref_dp(table, cap, fb)
        assert parents.tobytes() == ref.parents.tobytes() and score == ref.score and order.tobytes() == ref.order.tobytes()
        assert cp.flags_ref([int(x) for x in parents]) == 0 and max(bin(int(x)).count("1") for x in parents) <= cap
        L = real.local(parents[None])[1][0]
        tau = tau_of(L, n)
        assert abs(score - rescored) <= tau, (name, real.typ, score, rescored, tau)
        greedy, tabu = real.heuristics(cap, fb)
        print(f"\n{name} {real.typ} cap {cap} blacklist {fb is not None}: exact {score!r} rescored {rescored!r} tau {tau:.3e} "
              f"hill_climb {greedy!r} (gap {score - greedy:.6g}) tabu {tabu!r} (gap {score - tabu:.6g})")
        assert score >= greedy - tau and score >= tabu - tau, (name, real.typ, score, greedy, tabu, tau)
        out[fb is not None] = (score, greedy, tabu)
    if name == "asia":
        # the known network has a three-parent variable: it is admissible from cap 3 on, so it bounds that optimum (and the
        # uncapped one) from below by monotonicity; against the cap-2 optimum the comparison is a fact of the data
        known, oracle = known_asia(real.typ, real.arg)
        Lk = real.local(known[None])[1][0]
        table3 = real.table(None)
        for c in (3, None):
            p3, s3, r3, _ = real.search(table3, c, None)
            t3 = max(tau_of(real.local(p3[None])[1][0], n), tau_of(Lk, n))
            cells = sum(float(table3[int(known[v]), v]) for v in range(n))
            assert table3[[int(x) for x in known], np.arange(n)].tobytes() == Lk.tobytes()
            assert s3 >= cells - t3 and s3 >= oracle - t3 and abs(s3 - r3) <= t3, (real.typ, c, s3, cells, oracle, t3)
        print(f"asia {real.typ}: known network {oracle!r}; optimum uncapped {s3!r}, cap 2 {out[False][0]!r}")
        assert out[False][0] >= oracle - tau_of(Lk, n), (real.typ, out[False][0], oracle)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 5. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    """(entry point, arguments, return code, text dvs_last_error must contain) of dvs_exact_search: every check, and the pairs
    where two checks fail and the earlier one decides.  D: a dummy non-null pointer, never dereferenced."""
    tb, wb = 3 * 256 * 8 * 8, layout(3, 8)[4]
    cases = []
    c = entry("dvs_exact_search", cases, batch=3, n_vars=8, table=D, table_bytes=tb, max_parents=0, forbidden=None, workspace=D,
              workspace_bytes=wb, parents=D, order=D, score=D, flags=D, stream=None)
    big = dict(table_bytes=1 << 40, workspace_bytes=1 << 40)
    c(2, "batch must be > 0", batch=0)
    c(2, "batch must be > 0", batch=-2)
    c(3, "n_vars must be in [1, 20]", n_vars=0)
    c(3, "n_vars must be in [1, 20]", n_vars=21)
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=128, n_vars=20, **big)      # 2^27 * 20 > 2^31
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=1 << 30, n_vars=1, **big)   # 2^31 exactly
    for name in ("table", "workspace", "parents", "order", "score", "flags"):
        c(10, "null pointer", **{name: None})
    c(14, f"table_bytes < batch * 2^n_vars * n_vars * 8 = {tb}", table_bytes=tb - 1)
    c(14, f"workspace_bytes < dvs_exact_workspace_bytes = {wb}", workspace_bytes=wb - 1)
    c(14, f"workspace_bytes < dvs_exact_workspace_bytes = {layout(5, 20)[4]}", batch=5, n_vars=20, table_bytes=1 << 40,
      workspace_bytes=0)
    c(2, "batch must be > 0", batch=0, n_vars=21)                                      # batch before n_vars
    c(3, "n_vars must be in [1, 20]", batch=1 << 30, n_vars=21)                        # n_vars before the product
    c(2, "batch * 2^n_vars * n_vars must be < 2^31", batch=128, n_vars=20, table=None)   # the product before null
    c(10, "null pointer", flags=None, table_bytes=0, workspace_bytes=0)                # null before the sizes
    c(14, f"table_bytes < batch * 2^n_vars * n_vars * 8 = {tb}", table_bytes=0, workspace_bytes=0)   # table_bytes before workspace_bytes
    return cases


def check_argument_refusals(lib, D):
    run(lib, validation_cases(D))
    for batch, n in ((1, 1), (3, 8), (5, 20), (1, 14)):
        assert lib.dvs_exact_workspace_bytes(batch, n) == layout(batch, n)[4]
    for (batch, n), text in (((0, 8), "batch must be > 0"), ((1, 0), "n_vars must be in [1, 20]"), ((1, 21), "n_vars must be in [1, 20]"),
                             ((128, 20), "must be < 2^31")):
        assert lib.dvs_exact_workspace_bytes(batch, n) == 0
        assert lib.dvs_last_error().decode().startswith("dvs_exact_workspace_bytes: ") and text in lib.dvs_last_error().decode()
