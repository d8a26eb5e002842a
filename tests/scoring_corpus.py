"""TEST HELPER: seeded cases, high-precision references and the checks themselves for the fp64 scoring kernels of
csrc/k_bic.hip (dvs_bic_scores, dvs_bic_parent_masks, dvs_gp_predict, dvs_gp_kernel, dvs_gp_kernel_backward) and for
dvs_clip_adam's gradient norm (csrc/k_optim.hip), over the whole range include/dvs.h promises rather than the shapes of
the shipped data.  Plain numpy, no GPU.  tests/test_emu_scoring.py (emulator build) and tests/test_gpu_scoring.py
(device) import the same cases AND the same check functions; they differ only in the `Backend` that moves buffers.

References
  BIC   reference_local_score: the formula of oracle/bic.py restated sparsely (occupied cells via np.unique, terms summed
        with math.fsum, q_v a Python integer), so that 16^15 configurations are representable.  It is anchored, not
        free-standing: wherever q * r <= 2^24 it must equal oracle.bic.local_score to 1e-12 (bic_reference asserts it).
  GP    gp_kernel_ref / gp_kernel_backward_ref / gp_predict_ref: the formulas of include/dvs.h in float64, points taken as
        float32 and promoted.
  Adam  adam_ref / clip_adam_ref: torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU in float64.

Tolerances are derived, not measured.
  BIC, dvs_gp_kernel, dvs_gp_kernel_backward: fp64 on both sides.  An output is a sum of at most S (BIC) or nb (GP) terms,
        each a few roundings (division, log / exp, product), added S / 256 (nb / 64) per lane and then in a tree of 8 (6)
        levels: the error is below (S / 256 + 12) * 2^-53 * T <= 2e-14 * T with T the sum of the terms' absolute values.
        Asserted: |got - ref| <= 1e-12 * T per output element — two decades over the bound, many decades under what a
        swapped pair of counts, a wrong parent column or a transposed G changes.
  dvs_gp_predict: the kernel accumulates the squared distance in float32 (dim fmaf's), the reference in float64.  A
        relative error e in d2 changes exp(-d2 / 2l^2) by the factor e * d2 / 2l^2, so per query
            bound = 4 * outputscale * sum_m |alpha_m| exp(-d2_m / 2l^2) * (dim + 2) * 2^-24 * d2_m / 2l^2
        ((dim + 2) roundings of 2^-24 each; the 4 covers the float32 subtraction, whose error enters d^2 twice).
  dvs_clip_adam: see check_clip_adam.
"""
import ctypes
import functools
import math
from collections import namedtuple

import numpy as np

from oracle import bic as obic
from tests.abi_cases import call, call_rc

MAX_BINS = 36864          # dense LDS table of k_bic_local (include/dvs.h: "up to 36 864 cells")
MAX_SORT = 16384          # samples the sorted-samples path holds
BIC_RTOL = 1e-12
GP_RTOL = 1e-12
ORACLE_CELLS = 1 << 24    # oracle.bic.local_score's dense bincount is affordable up to here
U64 = np.uint64


# ---------------------------------------------------------------------------------------------------------------------
# Backends: how a test moves numpy buffers to the library under test
# ---------------------------------------------------------------------------------------------------------------------
class EmuBackend:
    """tests/emu build: the library reads and writes the numpy buffers in place."""
    stream = None

    def __init__(self, lib):
        self.lib = lib

    def put(self, a):
        return np.array(a, copy=True, order="C")

    def get(self, h):
        return h

    def ptr(self, h):
        return ctypes.c_void_p(h.ctypes.data)


class GpuBackend:
    """device build: buffers are torch tensors on cuda:0 (64-bit unsigned words travel as int64)."""

    def __init__(self, lib):
        import torch
        self.lib, self.torch = lib, torch
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def put(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint64:
            return (self.torch.from_numpy(a.view(np.int64).copy()).cuda(), np.uint64)
        return (self.torch.from_numpy(a.copy()).cuda(), None)

    def get(self, h):
        self.torch.cuda.synchronize()
        a = h[0].cpu().numpy()
        return a.view(h[1]) if h[1] is not None else a

    def ptr(self, h):
        return ctypes.c_void_p(h[0].data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# BIC: data, reference
# ---------------------------------------------------------------------------------------------------------------------
def synthetic_dataset(n_vars, n_samples, cards, seed, drop_top=()):
    """Level-coded uint8 [S, n] with DEPENDENT columns: column i is, with probability 0.75, a fixed function of one or two
    earlier columns and otherwise uniform noise (independent uniform columns would make every parent set score alike and
    let a mixed-up parent index pass).  Returns (data, card) with card exactly `cards` — not data.max(0) + 1: a column in
    `drop_top` never takes its top level, a 1-level column is constant."""
    cards = [int(c) for c in cards]
    assert len(cards) == n_vars and all(1 <= c <= 16 for c in cards)
    rng = np.random.default_rng(seed)
    data = np.zeros((n_samples, n_vars), np.uint8)
    for i, c in enumerate(cards):
        levels = c - 1 if (i in drop_top and c > 1) else c
        noise = rng.integers(0, levels, n_samples)
        if i == 0:
            col = noise
        else:
            a = int(rng.integers(0, i))
            b = int(rng.integers(0, i))
            f = (3 * data[:, a].astype(np.int64) + 5 * data[:, b].astype(np.int64) + i) % levels
            col = np.where(rng.random(n_samples) < 0.75, f, noise)
        data[:, i] = col
    return data, np.asarray(cards, np.uint8)


def pack(data):
    """[S, n] level codes -> the ABI's u64 [S][ceil(n/16)] words (4 bits per variable)."""
    S, n = data.shape
    packed = np.zeros((S, (n + 15) // 16), U64)
    for i in range(n):
        packed[:, i // 16] |= data[:, i].astype(U64) << U64(4 * (i % 16))
    return packed


def reference_local_score(data, card, v, parents):
    """(local BIC score of variable v with the given parents, T = sum |N_jk log(N_jk / N_j)| + |penalty|)."""
    S = data.shape[0]
    parents = sorted(int(p) for p in parents)
    assert v not in parents and len(set(parents)) == len(parents)
    r = int(card[v])
    q = 1
    for p in parents:
        q *= int(card[p])
    cells, njk = np.unique(data[:, parents + [v]], axis=0, return_counts=True)
    if parents:
        _, inv = np.unique(cells[:, :-1], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        nj = np.bincount(inv, weights=njk)[inv]
    else:
        nj = np.full(len(njk), S, np.float64)
    terms = [int(c) * math.log(int(c) / int(t)) for c, t in zip(njk, nj)]
    penalty = 0.5 * math.log(S) * (r - 1) * q
    return math.fsum(terms) - penalty, math.fsum(abs(t) for t in terms) + abs(penalty)


def reference_bic(data, card, parent_sets):
    """parent_sets[v]: parents of data-set variable v -> (BIC, local scores [n], T [n])."""
    loc, tol = zip(*(reference_local_score(data, card, v, parent_sets[v]) for v in range(data.shape[1])))
    return math.fsum(loc), np.asarray(loc), np.asarray(tol)


def mask_bits(m):
    return [u for u in range(64) if (int(m) >> u) & 1]


def masks_of(n, *dags):
    """dags: {child: [parents]} each -> u64 [B, n]."""
    out = np.zeros((len(dags), n), U64)
    for b, d in enumerate(dags):
        for v, ps in d.items():
            for p in ps:
                out[b, v] |= U64(1) << U64(p)
    return out


def cells_of(card, v, parents):
    q = 1
    for p in parents:
        q *= int(card[p])
    return q * int(card[v])


def key_bits(card, v, parents):
    bits = lambda c: max(int(c) - 1, 0).bit_length()
    return bits(card[v]) + sum(bits(card[p]) for p in parents)


BicCase = namedtuple("BicCase", "name data card masks status refused bitwise_pairs zero_cells")
BicCase.__doc__ = """data u8 [S, n], card u8 [n], masks u64 [B, n]; status: expected status word; refused: the (DAG, variable)
cells that must come back NaN — every other cell is compared with the reference; bitwise_pairs: ((b, v), (b', v')) local
scores that must be equal bytes; zero_cells: cells that must be exactly 0.0."""


def _case(name, data, card, masks, status=0, refused=(), bitwise_pairs=(), zero_cells=()):
    refused = frozenset(refused)
    assert len({b for b, _ in refused}) * 4 <= len(masks), name              # never more than one DAG in four
    return BicCase(name, data, card, np.ascontiguousarray(masks, U64), status, refused, tuple(bitwise_pairs),
                   tuple(zero_cells))


def expected_path(case, b, v):
    """'dense' | 'sort' | 'refused' for one cell, from the documented limits (include/dvs.h), not from the kernel."""
    n, S = case.data.shape[1], case.data.shape[0]
    ps = [u for u in mask_bits(case.masks[b, v]) if u != v]
    if any(u >= n for u in ps):
        return "refused"
    if cells_of(case.card, v, ps) <= MAX_BINS:
        return "dense"
    return "sort" if (S <= MAX_SORT and key_bits(case.card, v, ps) <= 63) else "refused"


def _random_dag(rng, n, max_parents=3):
    """parents drawn from anywhere in a random topological order: a parent's data word may be above its child's."""
    order = rng.permutation(n)
    d = {}
    for k in range(1, n):
        cnt = int(rng.integers(0, max_parents + 1))
        if cnt:
            d[int(order[k])] = sorted(int(x) for x in rng.choice(order[:k], size=min(cnt, k), replace=False))
    return d


def _cross_word_dag(n):
    """One child in every data word with a parent in every data word (all 3 x 3 (child word, parent word) pairs that exist
    at this n), plus: the last variable (47 at n = 48) as a child of variable 0 and of its neighbour and as the only parent
    of variable 4, and variable 5 with variable 0 as its only parent."""
    d = {}
    for cw in range(3):
        for pw in range(3):
            c, p = 16 * cw + 1 + pw, 16 * pw + 7 + cw
            if c < n - 1 and p < n - 1:
                d.setdefault(c, []).append(p)
    d[n - 1] = [0, n - 2]
    d[4] = [n - 1]
    d[5] = [0]
    return d


def smooth_neighbours(m=MAX_BINS):
    """(largest product of level counts 1..16 below m, smallest above m): the integers next to m with no prime factor
    over 13 — the nearest table sizes a parent set can reach on either side of the dense / sort switch."""
    def smooth(x):
        for p in (2, 3, 5, 7, 11, 13):
            while x % p == 0:
                x //= p
        return x == 1
    lo = next(x for x in range(m - 1, 0, -1) if smooth(x))
    hi = next(x for x in range(m + 1, 2 * m) if smooth(x))
    return lo, hi


def level_factors(m):
    """m as a product of level counts 2..16, largest first."""
    out = []
    while m > 1:
        d = next(d for d in range(16, 1, -1) if m % d == 0)
        out.append(d)
        m //= d
    return out


_SORT_CARDS = [16, 16, 16, 16, 8, 4]


def bic_cases():
    """The named BIC cases (see each block)."""
    cases = []
    # 1. wide rows: 1, 2 and 3 data words, the 16 / 32 edges, the headline n = 37 and the maximum; small tables (dense path)
    for n in (16, 17, 32, 33, 37, 48):
        rng = np.random.default_rng(1000 + n)
        data, card = synthetic_dataset(n, 300, rng.integers(2, 5, n), seed=n)
        masks = masks_of(n, _random_dag(rng, n), _cross_word_dag(n), _random_dag(rng, n, 2))
        cases.append(_case(f"wide{n}", data, card, masks))
    #    the sort path over three data words: 16-level variables in words 0, 1 and 2, a child in the last word with parents in
    #    all three and a child in word 0 likewise (16^5 cells each: the key-building loop reads every word of the row)
    for n, big in ((37, (1, 2, 18, 34, 35, 36)), (48, (0, 15, 16, 31, 32, 47))):
        rng = np.random.default_rng(1100 + n)
        cards = rng.integers(2, 5, n)
        cards[list(big)] = 16
        data, card = synthetic_dataset(n, 500, cards, seed=100 + n)
        lo_child, hi_child = big[0], big[-1]
        d0 = {hi_child: [v for v in big[:-1] if v != big[1]], 7: [big[2], 20]}
        d1 = {lo_child: [v for v in big[1:] if v != big[3]], 21: [lo_child, 8]}
        c = _case(f"widesort{n}", data, card, masks_of(n, d0, d1))
        assert expected_path(c, 0, hi_child) == "sort" and expected_path(c, 1, lo_child) == "sort"
        assert {p // 16 for p in d0[hi_child]} == {0, 1, 2} == {p // 16 for p in d1[lo_child]}
        cases.append(c)
    # 2. level counts 1..16 in one data set; variable 5 never takes its top level; 3 and 7 are constant columns
    cards = [16, 16, 16, 1, 5, 16, 7, 1, 3, 9, 12, 2, 13]
    data, card = synthetic_dataset(13, 2000, cards, seed=21, drop_top=(5,))
    assert data[:, 5].max() == 14 and not data[:, 3].any() and not data[:, 7].any()
    base = {2: [0, 1], 4: [0], 5: [4], 6: [5, 11], 9: [6], 10: [9, 2], 12: [5, 8], 8: [4]}
    with1 = {2: [0, 1, 7], 3: [0], 4: [0, 3], 5: [4], 6: [5, 7, 11], 9: [6, 3, 7], 10: [9, 2], 12: [5, 8], 8: [4]}
    sort0 = {10: [0, 1, 2, 5], 6: [0, 1, 2]}                 # 16^4 * 12 cells: sort; 16^3 * 7 = 28 672 cells: dense
    sort1 = {10: [0, 1, 2, 3, 5, 7], 6: [0, 1, 2, 3]}
    c = _case("levels", data, card, masks_of(13, base, with1, sort0, sort1),
              bitwise_pairs=[((0, v), (1, v)) for v in (2, 4, 6, 9)] + [((2, 10), (3, 10)), ((2, 6), (3, 6))],
              zero_cells=[(0, 3), (1, 3), (0, 7), (2, 3)])
    assert expected_path(c, 2, 10) == "sort" and expected_path(c, 2, 6) == "dense"
    cases.append(c)
    # 3. the dense / sort switch: exactly 36 864 cells two ways, and the nearest reachable table sizes on either side
    lo, hi = smooth_neighbours()
    groups = [[16, 16, 16, 9], [9, 16, 16, 16], level_factors(lo), level_factors(hi)]
    cards, dag, at = [], {}, 0
    for g in groups:
        dag[at] = list(range(at + 1, at + len(g)))
        cards += g
        at += len(g)
    data, card = synthetic_dataset(len(cards), 1500, cards, seed=33)
    children = sorted(dag)
    assert [cells_of(card, v, dag[v]) for v in children] == [MAX_BINS, MAX_BINS, lo, hi] and lo < MAX_BINS < hi
    c = _case("boundary", data, card, masks_of(len(cards), dag, {}))
    assert [expected_path(c, 0, v) for v in children] == ["dense", "dense", "dense", "sort"]
    cases.append(c)
    #    the same tables with one sample more than the sort path holds tell WHICH path a table took, where the scores cannot:
    #    36 864 cells and below must still be counted (dense), the size above must be refused
    big, _ = synthetic_dataset(len(cards), MAX_SORT + 1, cards, seed=34)
    top = children[3]
    c = _case("boundaryS16385", big, card, masks_of(len(cards), {v: dag[v] for v in children[:3]}, {top: dag[top]}, {},
                                                    {children[2]: dag[children[2]]}), status=16, refused={(1, top)})
    assert [expected_path(c, 0, v) for v in children[:3]] == ["dense"] * 3 and expected_path(c, 1, top) == "refused"
    cases.append(c)
    # 4. sample counts: the sort path pads to a power of two (257 -> 512; 16 384 exactly full); the dense path has no limit
    full, card = synthetic_dataset(6, 40000, _SORT_CARDS, seed=404)
    sortd = masks_of(6, {0: [1, 2, 3], 4: [5]}, {3: [0, 1, 2, 4], 5: [4]})
    for S in (1, 2, 63, 64, 255, 256, 257, 1000, 16384):
        c = _case(f"sortS{S}", full[:S], card, sortd)
        assert expected_path(c, 0, 0) == "sort" and expected_path(c, 1, 3) == "sort"
        cases.append(c)
    densed = masks_of(6, {0: [1, 2], 4: [5, 0], 5: [1]}, {3: [0, 4, 5], 1: [0]})
    for S in (16385, 40000):
        c = _case(f"denseS{S}", full[:S], card, densed)
        assert all(expected_path(c, b, v) == "dense" for b in range(2) for v in range(6))
        cases.append(c)
    # 5. refusals.  64 key bits (a 16-level child with 15 parents of 16 levels) next to 63 (one 8-level parent instead),
    #    which must be scored; dense DAGs around them: the batch mixes dense, sort and refused variables
    data, card = synthetic_dataset(17, 512, [16] * 16 + [8], seed=55)
    m = masks_of(17, {3: [1, 2], 16: [0]}, {0: list(range(1, 16)), 5: [16]}, {0: list(range(1, 15)) + [16], 5: [16]},
                 {9: [16, 0], 1: [2, 3, 4, 5]})
    c = _case("keybits64", data, card, m, status=16, refused={(1, 0)})
    assert key_bits(card, 0, range(1, 16)) == 64 and key_bits(card, 0, list(range(1, 15)) + [16]) == 63
    assert expected_path(c, 2, 0) == "sort" and expected_path(c, 3, 1) == "sort" and expected_path(c, 1, 0) == "refused"
    cases.append(c)
    #    one sample too many for the sort path
    card = np.asarray(_SORT_CARDS, np.uint8)
    m = masks_of(6, {4: [5]}, {0: [1, 2, 3], 4: [5]}, {0: [1, 2]}, {5: [0, 4]})
    cases.append(_case("sortS16385", full[:16385], card, m, status=16, refused={(1, 0)}))
    #    a parent bit >= n_vars (17 and 63), two DAGs in eight
    data, card = synthetic_dataset(17, 400, [3] * 17, seed=56)
    rng = np.random.default_rng(57)
    m = masks_of(17, *[_random_dag(rng, 17) for _ in range(8)])
    m[2, 3] |= U64(1) << U64(17)
    m[6, 16] |= U64(1) << U64(63)
    cases.append(_case("parentbit", data, card, m, status=16, refused={(2, 3), (6, 16)}))
    #    a self-loop bit is masked off: scores like the set without it (sort, dense, the last variable, a lone self-loop)
    data, card = synthetic_dataset(17, 600, [16] * 8 + [3] * 9, seed=58)
    d = {0: [1, 2, 3], 16: [0, 9], 9: [10], 4: [5]}
    m = masks_of(17, d, {v: ps + [v] for v, ps in d.items()})
    m[1, 12] |= U64(1) << U64(12)
    c = _case("selfloop", data, card, m, bitwise_pairs=[((0, v), (1, v)) for v in (0, 16, 9, 4, 12)])
    assert expected_path(c, 1, 0) == "sort"
    cases.append(c)
    # 6. batch geometry: k_bic_sum's last partial workgroup
    data, card = synthetic_dataset(4, 64, [2, 3, 4, 5], seed=66)
    pats = masks_of(4, {}, {1: [0]}, {2: [0, 1]}, {3: [0, 1, 2]}, {3: [2], 2: [1], 1: [0]}, {0: [3], 1: [3]}, {2: [3, 0]})
    for B in (1, 255, 256, 257):
        cases.append(_case(f"batch{B}", data, card, pats[np.arange(B) % len(pats)]))
    return cases


def real_data_cases():
    """asia / sachs (the shipped data, card = data.max(0) + 1) with random DAGs and the sachs 10-parent sink: every cell is
    small enough for oracle.bic, so these anchor the sparse reference on real counts."""
    from oracle import features as ofeat
    from tests.helpers import load_npz
    cases = []
    for name, n in (("asia", 8), ("sachs", 11)):
        data = load_npz(f"bn_{name}_data.npz")["data"].astype(np.uint8)
        card = (data.max(0) + 1).astype(np.uint8)
        graphs = list(ofeat.synthetic_dags(n, n, 3, seed=5))
        if name == "sachs":
            graphs[2] = (list(range(11)), [(u, 10) for u in range(10)])
        m = np.zeros((len(graphs), n), U64)
        for b, (lab, edges) in enumerate(graphs):
            for u, v in edges:
                m[b, lab[v]] |= U64(1) << U64(lab[u])
        cases.append(_case(name, data, card, m))
    return cases


# The tests parametrise over names and build the data on first use: collecting the suite does not generate a corpus.
BIC_CASE_NAMES = tuple([f"wide{n}" for n in (16, 17, 32, 33, 37, 48)] + ["widesort37", "widesort48", "levels", "boundary",
                       "boundaryS16385"] + [f"sortS{s}" for s in (1, 2, 63, 64, 255, 256, 257, 1000, 16384)]
                       + ["denseS16385", "denseS40000", "keybits64", "sortS16385", "parentbit", "selfloop"]
                       + [f"batch{b}" for b in (1, 255, 256, 257)] + ["asia", "sachs"])
REFUSAL_CASE_NAMES = ("boundaryS16385", "keybits64", "sortS16385", "parentbit")
RELABEL_CASE_NAMES = ("relabel16", "relabel17", "relabel48")


@functools.lru_cache(maxsize=None)
def _bic_cases_by_name():
    cases = {c.name: c for c in bic_cases() + real_data_cases()}
    assert tuple(cases) == BIC_CASE_NAMES, tuple(cases)
    assert {n for n, c in cases.items() if c.refused} == set(REFUSAL_CASE_NAMES)
    return cases


def bic_case(name):
    return _bic_cases_by_name()[name]


@functools.lru_cache(maxsize=None)
def _relabel_cases_by_name():
    cases = {c[0]: c for c in relabel_cases()}
    assert tuple(cases) == RELABEL_CASE_NAMES
    return cases


def relabel_case(name):
    return _relabel_cases_by_name()[name]


_ref_cache = {}


def bic_reference(case):
    """(local [B, n], T [B, n]) of every cell that is not refused (NaN there), asserting the anchor on the way: wherever
    oracle.bic.local_score can represent the table, the sparse reference equals it to 1e-12."""
    if case.name in _ref_cache:
        return _ref_cache[case.name]
    B, n = case.masks.shape
    loc = np.full((B, n), np.nan)
    tol = np.full((B, n), np.nan)
    memo = {}
    anchored = 0
    for b in range(B):
        for v in range(n):
            if (b, v) in case.refused:
                assert expected_path(case, b, v) == "refused", (case.name, b, v)
                continue
            assert expected_path(case, b, v) != "refused", (case.name, b, v)
            ps = tuple(u for u in mask_bits(case.masks[b, v]) if u != v)
            if (v, ps) not in memo:
                memo[v, ps] = reference_local_score(case.data, case.card, v, ps)
                if cells_of(case.card, v, ps) <= ORACLE_CELLS:
                    want = obic.local_score(case.data.astype(np.int64), case.card, v, ps)
                    assert abs(memo[v, ps][0] - want) <= 1e-12 * max(abs(want), memo[v, ps][1]), (case.name, b, v)
                    anchored += 1
            loc[b, v], tol[b, v] = memo[v, ps]
    assert anchored > 0, case.name
    _ref_cache[case.name] = (loc, tol)
    return loc, tol


def run_bic(be, data, card, masks):
    """one dvs_bic_scores call -> (return code, scratch [B, n], out [B], status)."""
    B, n = masks.shape
    h = dict(data=be.put(pack(data)), card=be.put(card), parents=be.put(masks), scratch=be.put(np.full((B, n), -7.0)),
             out=be.put(np.full(B, -7.0)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bic_scores", batch=B, n_vars=n, n_samples=data.shape[0], **h)
    return rc, be.get(h["scratch"]).copy(), be.get(h["out"]).copy(), int(be.get(h["status"])[0])


def check_bic_case(be, case, twice=True):
    """The per-variable local scores (scratch) and the per-DAG sums of one case against the reference; returns the worst
    |got - ref| / T seen (for reporting only: the assert is the fixed 1e-12)."""
    loc, tol = bic_reference(case)
    rc, scratch, out, status = run_bic(be, case.data, case.card, case.masks)
    assert rc == 0 and status == case.status, (case.name, rc, status)
    B, n = case.masks.shape
    worst = 0.0
    bad_dags = {b for b, _ in case.refused}
    for b in range(B):
        for v in range(n):
            if (b, v) in case.refused:
                assert np.isnan(scratch[b, v]), (case.name, b, v, scratch[b, v])
                continue
            err = abs(scratch[b, v] - loc[b, v])
            assert err <= BIC_RTOL * tol[b, v], (case.name, "dag", b, "variable", v, expected_path(case, b, v),
                                                 scratch[b, v], loc[b, v], err / max(tol[b, v], 1e-300))
            if tol[b, v] > 0:
                worst = max(worst, err / tol[b, v])
        if b in bad_dags:
            assert np.isnan(out[b]), (case.name, b, out[b])
        else:
            assert abs(out[b] - math.fsum(loc[b])) <= BIC_RTOL * math.fsum(tol[b]), (case.name, "dag", b, out[b])
    for (b0, v0), (b1, v1) in case.bitwise_pairs:
        assert expected_path(case, b0, v0) == expected_path(case, b1, v1)
        assert scratch[b0, v0].tobytes() == scratch[b1, v1].tobytes(), (case.name, (b0, v0), (b1, v1))
    for b, v in case.zero_cells:
        assert scratch[b, v] == 0.0, (case.name, b, v, scratch[b, v])
    if twice:         # integer counts and a fixed summation order: the result does not depend on the order of the atomics
        rc, scratch2, out2, status2 = run_bic(be, case.data, case.card, case.masks)
        assert rc == 0 and status2 == status and scratch2.tobytes() == scratch.tobytes() and out2.tobytes() == out.tobytes()
    return worst


# dvs_bic_parent_masks composed with dvs_bic_scores
def relabel_cases():
    """(name, data, card, labels u8 [B, n], preds u64 [B, n]) at n in {16, 17, 48} with u64 predecessor rows: vertex v
    stands for variable labels[v]; row 0 reversed labels, row 1 a random permutation, row 2 the identity."""
    out = []
    for n in (16, 17, 48):
        rng = np.random.default_rng(700 + n)
        data, card = synthetic_dataset(n, 300, rng.integers(2, 5, n), seed=70 + n)
        labels = np.stack([np.arange(n)[::-1], rng.permutation(n), np.arange(n)]).astype(np.uint8)
        preds = np.zeros((3, n), U64)
        for b in range(3):
            for v in range(1, n):
                for u in rng.choice(v, size=min(v, int(rng.integers(0, 4))), replace=False):
                    preds[b, v] |= U64(1) << U64(int(u))
        preds[:, n - 1] |= U64(1)                       # vertex 0 -> last vertex: the reversed row maps it to n-1 -> 0
        out.append((f"relabel{n}", data, card, labels, preds))
    return out


def check_relabel_case(be, name, data, card, labels, preds):
    B, n = labels.shape
    want = np.zeros((B, n), U64)
    for b in range(B):
        for v in range(n):
            for u in mask_bits(preds[b, v]):
                want[b, labels[b, v]] |= U64(1) << U64(int(labels[b, u]))
    lab, pr = be.put(labels), be.put(preds)
    got, status = be.put(np.full((B, n), 0xFFFF, U64)), be.put(np.zeros(1, np.int32))
    rc = call_rc(be, "dvs_bic_parent_masks", batch=B, n_vars=n, preds_are_u64=1, labels=lab, preds=pr, parents=got, status=status)
    assert rc == 0 and int(be.get(status)[0]) == 0, name
    got = be.get(got).copy()
    assert np.array_equal(got, want), name
    return check_bic_case(be, _case(name, data, card, got), twice=False)


# ---------------------------------------------------------------------------------------------------------------------
# GP kernels
# ---------------------------------------------------------------------------------------------------------------------
def _sqdist(xa, xb):
    a, b = xa.astype(np.float64), xb.astype(np.float64)
    d = b[None, :, :] - a[:, None, :]                    # [na, nb, D]: xb_b - xa_a
    return d, (d * d).sum(-1)


def gp_kernel_ref(xa, xb, o, l):
    """(K [na, nb], sum of absolute terms = K: one positive term per element)."""
    _, d2 = _sqdist(xa, xb)
    K = o * np.exp(-d2 / (2.0 * l * l))
    return K, K.copy()


def gp_kernel_backward_ref(xa, xb, o, l, G, symmetric):
    """((dxa [na, D], row_sums [na, 2]), (their sums of absolute terms))."""
    d, d2 = _sqdist(xa, xb)
    K = o * np.exp(-d2 / (2.0 * l * l))
    Gp = G + G.T if symmetric else G
    W = Gp * K
    dxa = (W[:, :, None] * d).sum(1) / (l * l)
    dxa_abs = (np.abs(W)[:, :, None] * np.abs(d)).sum(1) / (l * l)
    GK = G * K
    rows = np.stack([(GK * d2).sum(1) / l ** 3, GK.sum(1) / o], 1)
    rows_abs = np.stack([(np.abs(GK) * d2).sum(1) / l ** 3, np.abs(GK).sum(1) / o], 1)
    return (dxa, rows), (dxa_abs, rows_abs)


def gp_predict_ref(x, z, alpha, o, l, c):
    """(out [B], bound [B]: the float32-distance tolerance of the module docstring)."""
    _, d2 = _sqdist(x, z)
    e = d2 / (2.0 * l * l)
    k = np.exp(-e)
    out = c + o * np.array([math.fsum(row) for row in k * alpha[None, :]])
    D = x.shape[1]
    bound = 4.0 * o * (np.abs(alpha)[None, :] * k * (D + 2) * 2.0 ** -24 * e).sum(1)
    return out, bound


# every value of each axis appears: {1, 3, 4, 5, 63, 64, 65, 257} x {1, 63, 64, 65, 500} x {1, 7, 31, 32}
GP_TRIPLES = [(1, 1, 1), (1, 500, 32), (3, 63, 7), (3, 65, 31), (4, 64, 32), (4, 1, 7), (5, 65, 1), (5, 500, 31),
              (63, 63, 31), (63, 64, 1), (63, 1, 32), (64, 64, 7), (64, 65, 32), (64, 500, 1), (65, 65, 31), (65, 63, 32),
              (65, 1, 1), (257, 500, 7), (257, 64, 31), (257, 63, 1), (257, 1, 31), (1, 64, 31), (3, 500, 1), (4, 65, 7),
              (5, 63, 32), (63, 500, 7), (64, 1, 31), (65, 64, 7), (1, 1, 32), (5, 5, 31)]
GP_PREDICT_TRIPLES = [(1, 1, 1), (1, 500, 32), (3, 63, 7), (3, 64, 32), (4, 65, 1), (4, 500, 7), (5, 64, 7), (5, 1, 32),
                      (4097, 63, 32), (4097, 65, 7), (4097, 500, 1), (1, 64, 1), (3, 65, 32), (5, 63, 1), (4, 1, 7)]
assert len(GP_TRIPLES) >= 24
for _ax, _vals in enumerate(((1, 3, 4, 5, 63, 64, 65, 257), (1, 63, 64, 65, 500), (1, 7, 31, 32))):
    assert {t[_ax] for t in GP_TRIPLES} >= set(_vals)
for _ax, _vals in enumerate(((1, 3, 4, 5, 4097), (1, 63, 64, 65, 500), (1, 7, 32))):
    assert {t[_ax] for t in GP_PREDICT_TRIPLES} == set(_vals)


def gp_points(na, nb, D, seed):
    """float32 points ~ N(0, 1) and a lengthscale of about sqrt(D): |xa - xb|^2 / 2 l^2 is O(1), so that the exponent's own
    conditioning (its relative error is multiplied by its size) stays inside the 1e-12 budget."""
    rng = np.random.default_rng(seed)
    xa = rng.standard_normal((na, D)).astype(np.float32)
    xb = rng.standard_normal((nb, D)).astype(np.float32)
    return rng, xa, xb, 1.7, math.sqrt(D) * 1.1


def run_gp_kernel(be, xa, xb, o, l):
    na, nb, D = len(xa), len(xb), xa.shape[1]
    h = dict(xa=be.put(xa), xb=be.put(xb), K=be.put(np.full((na, nb), np.nan)))
    rc = call_rc(be, "dvs_gp_kernel", na=na, nb=nb, dim=D, outputscale=o, lengthscale=l, **h)
    return rc, be.get(h["K"]).copy()


def check_gp_kernel(be, na, nb, D):
    _, xa, xb, o, l = gp_points(na, nb, D, seed=na * 1000003 + nb * 1009 + D)
    rc, K = run_gp_kernel(be, xa, xb, o, l)
    ref, T = gp_kernel_ref(xa, xb, o, l)
    assert rc == 0
    err = np.abs(K - ref)                                           # NaN (an element never written) fails the comparison
    assert (err <= GP_RTOL * T).all(), ((na, nb, D), np.argwhere(~(err <= GP_RTOL * T))[:4])
    return float((err / T).max())


def check_gp_kernel_edges(be):
    """identical points give exactly outputscale; far points underflow to 0 without a NaN; dim = 33 is refused (code 2)."""
    for D in (1, 7, 32):
        rng = np.random.default_rng(D)
        x = rng.standard_normal((5, D)).astype(np.float32)
        rc, K = run_gp_kernel(be, x, x, 1.7, 0.3)
        assert rc == 0 and (np.diag(K) == 1.7).all() and np.array_equal(K, K.T)
        rc, K = run_gp_kernel(be, x, (x + np.float32(1e4)).astype(np.float32), 1.7, 0.3)
        assert rc == 0 and (K == 0.0).all()
        rc, K = run_gp_kernel(be, x, (x * np.float32(3e19)).astype(np.float32), 1.7, 0.3)       # d^2 ~ 1e39: finite in fp64
        assert rc == 0 and (K == 0.0).all()
    x = np.zeros((2, 33), np.float32)
    assert run_gp_kernel(be, x, x, 1.0, 1.0)[0] == 2


GUARD = 37          # doubles after the last output element that the kernel must not touch


def run_gp_backward(be, xa, xb, o, l, G, symmetric):
    na, nb, D = len(xa), len(xb), xa.shape[1]
    dxa = np.full(na * D + GUARD, np.nan)
    rows = np.full(na * 2 + GUARD, np.nan)
    dxa[na * D:] = -123.25
    rows[na * 2:] = -123.25
    h = dict(xa=be.put(xa), xb=be.put(xb), G=be.put(G), dxa=be.put(dxa), row_sums=be.put(rows))
    rc = call_rc(be, "dvs_gp_kernel_backward", na=na, nb=nb, dim=D, symmetric=symmetric, outputscale=o, lengthscale=l, **h)
    return rc, be.get(h["dxa"]).copy(), be.get(h["row_sums"]).copy()


def gp_cotangent(rng, na, nb):
    """mixed signs, magnitudes over six decades, not symmetric"""
    return rng.choice([-1.0, 1.0], (na, nb)) * 10.0 ** rng.uniform(-3, 3, (na, nb))


def check_gp_kernel_backward(be, na, nb, D, symmetric):
    rng, xa, xb, o, l = gp_points(na, nb, D, seed=na * 1000003 + nb * 1009 + D + 17 * symmetric)
    if symmetric:
        assert na == nb
        xb = xa
    G = gp_cotangent(rng, na, nb)
    assert not symmetric or na == 1 or not np.array_equal(G, G.T)
    rc, dxa, rows = run_gp_backward(be, xa, xb, o, l, G, symmetric)
    assert rc == 0
    (rdxa, rrows), (tdxa, trows) = gp_kernel_backward_ref(xa, xb, o, l, G, symmetric)
    assert (dxa[na * D:] == -123.25).all() and (rows[2 * na:] == -123.25).all(), ("guard region written", na, nb, D)
    worst = 0.0
    for name, got, ref, T in (("dxa", dxa[:na * D].reshape(na, D), rdxa, tdxa),
                              ("rows", rows[:2 * na].reshape(na, 2), rrows, trows)):
        err = np.abs(got - ref)                                     # a NaN left from the pre-fill fails here: "overwritten"
        assert (err <= GP_RTOL * T).all(), (name, (na, nb, D, symmetric), np.argwhere(~(err <= GP_RTOL * T))[:4])
        worst = max(worst, float((err / np.maximum(T, 1e-300)).max()))
    rc, dxa2, rows2 = run_gp_backward(be, xa, xb, o, l, G, symmetric)
    assert rc == 0 and dxa2.tobytes() == dxa.tobytes() and rows2.tobytes() == rows.tobytes()     # fixed summation order
    return worst


def check_gp_backward_refusals(be):
    rng, xa, xb, o, l = gp_points(4, 5, 8, seed=1)
    assert run_gp_backward(be, xa, xb, o, l, gp_cotangent(rng, 4, 5), 1)[0] == 12        # symmetric needs na == nb
    x = np.zeros((2, 33), np.float32)
    assert run_gp_backward(be, x, x, o, l, np.ones((2, 2)), 0)[0] == 2                  # dim <= 32


def predict_inputs(B, M, D, seed):
    """SGPR-like weights: inducing points in near-pairs whose weights are +a 1e6 and -a 1e6 + O(1), so the weighted sum is
    O(1) although every term is O(1e6) — the case k_gp_predict's comment gives as the reason for fp64 accumulation."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((M, D)).astype(np.float32)
    alpha = rng.standard_normal(M)
    for i in range(0, M - 1, 2):
        z[i + 1] = z[i] + (rng.standard_normal(D) * 1e-5).astype(np.float32)
        a = 1e6 * (1.0 + rng.random())
        alpha[i], alpha[i + 1] = a, -a + rng.standard_normal()
    x = rng.standard_normal((B, D)).astype(np.float32)
    return x, z, alpha, 1.3, math.sqrt(D) * 1.1, -2.5


def predict_inputs_resolved(B, M, D, seed):
    """Independent inducing points with O(1) weights of mixed sign: nothing cancels, so the same derived bound is 1e-6 ..
    1e-4 of the output and every single inducing point is resolved — a dropped, doubled or mis-indexed m (the last point of
    an odd M, the lone point of the second 64-lane pass at M = 65) is far outside it.  The +-1e6 weights above cannot show
    that: there the bound, honestly derived, is as large as the output."""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((M, D)).astype(np.float32)
    alpha = rng.choice([-1.0, 1.0], M) * rng.uniform(0.5, 2.0, M)
    x = rng.standard_normal((B, D)).astype(np.float32)
    return x, z, alpha, 1.3, math.sqrt(D) * 1.1, -2.5


PREDICT_WEIGHTS = {"sgpr": predict_inputs, "resolved": predict_inputs_resolved}


def check_gp_predict(be, B, M, D, weights="sgpr"):
    """returns the worst |got - ref| / bound"""
    x, z, alpha, o, l, c = PREDICT_WEIGHTS[weights](B, M, D, seed=B * 7919 + M * 31 + D)
    h = dict(x=be.put(x), inducing=be.put(z), alpha=be.put(alpha), out=be.put(np.full(B + GUARD, np.nan)))
    call(be, "dvs_gp_predict", batch=B, n_inducing=M, dim=D, outputscale=o, lengthscale=l, constant=c, **h)
    got = be.get(h["out"]).copy()
    assert np.isnan(got[B:]).all()
    ref, bound = gp_predict_ref(x, z, alpha, o, l, c)
    err = np.abs(got[:B] - ref)
    assert (bound > 0).all() and (err <= bound).all(), ((B, M, D), float(np.nanmax(err / bound)))
    return float((err / bound).max())


# ---------------------------------------------------------------------------------------------------------------------
# clip_grad_norm_ + Adam: the norm's tail and an update in which the norm matters
# ---------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 2, 3, 255, 256, 257, 1021, 1022, 65539)      # every residue of n % 4, both sides of one 256-lane pass
ADAM_STEP = 7
F32_EPS = 2.0 ** -24


def sq_parts(n):
    return ((n + 3) // 4 + 63) // 64            # dvs_sq_parts: one partial per 256 gradient entries


def adam_inputs(n):
    """a plain random vector whose last n % 4 entries (k_sqnorm_part's scalar tail) each carry a tenth of the rest's norm,
    about 1 % of the sum of squares apiece, so that a lost tail is 1e4 tolerances away at every size; moments as after a
    few steps (non-zero, exp_avg of the gradient's sign so that no term cancels); max_norm a tenth of the gradient's norm."""
    rng = np.random.default_rng(9000 + n)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    g[g == 0] = 1.0
    if n > 4 and n % 4:
        head = math.sqrt(float((g[:n - n % 4].astype(np.float64) ** 2).sum()))
        g[n - n % 4:] = np.sign(g[n - n % 4:]) * np.float32(0.1 * head)
    p = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    m = (0.05 * g * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    v = ((0.1 * g.astype(np.float64)) ** 2 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    return p, g, m, v, np.float32(0.1 * norm)


HYPER = tuple(float(np.float32(x)) for x in (0.05, 0.9, 0.999, 1e-8))       # lr, betas, eps as the float32 the ABI carries


def adam_ref(p, g, m, v, step, hyper=HYPER, max_norm=None):
    """torch.optim.Adam in float64 on the CPU: step number `step` (1-based) from the given moments, behind
    torch.nn.utils.clip_grad_norm_ when `max_norm` is given.  `hyper` = (lr, beta1, beta2, eps).  Returns (norm before
    clipping or None, the gradient Adam saw, exp_avg, exp_avg_sq, parameters)."""
    import torch
    lr, b1, b2, eps = hyper
    w = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    w.grad = torch.from_numpy(g.astype(np.float64))
    opt = torch.optim.Adam([w], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[w] = {"step": torch.tensor(float(step - 1)), "exp_avg": torch.from_numpy(m.astype(np.float64)),
                    "exp_avg_sq": torch.from_numpy(v.astype(np.float64))}
    norm = None if max_norm is None else float(torch.nn.utils.clip_grad_norm_([w], float(max_norm)))
    clipped = w.grad.detach().numpy().copy()
    opt.step()
    st = opt.state[w]
    assert int(st["step"]) == step
    return norm, clipped, st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), w.detach().numpy().copy()


def clip_adam_ref(p, g, m, v, max_norm):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64 on the CPU, from the given moments at ADAM_STEP."""
    return adam_ref(p, g, m, v, ADAM_STEP, HYPER, max_norm)


def bias_correction_rounding(b1, b2, step):
    """Relative error of the parameter update that the float32 bias corrections 1 - powf(b, step) can add.  powf is within
    one ulp (2 * 2^-24 relative) of b^step; the subtraction from 1 is exact for b^step >= 0.5 and one rounding otherwise,
    but it turns that ulp into b^step / (1 - b^step) ulps of the difference.  The update is proportional to
    sqrt(1 - b2^step) / (1 - b1^step), so beta2's share enters by half."""
    a1, a2 = b1 ** step / (1.0 - b1 ** step), b2 ** step / (1.0 - b2 ** step)
    return 2 * F32_EPS * (a1 + 0.5 * a2)


def adam_tolerances(p, gc, m, v, upd, b1, b2, rcoef=0.0, rbias=0.0, floor=0.0, upd_terms=None):
    """Per-element tolerances (exp_avg, exp_avg_sq, parameters) of one float32 Adam step, derived in check_clip_adam's
    docstring: 8 * 2^-24 of the absolute terms each quantity is made of, `rcoef` (relative error of a clip coefficient that
    the reference gradient `gc` does not carry yet) once on exp_avg's gradient term and twice on exp_avg_sq's and on the
    update `upd` = |new p - p|, `rbias` (bias_correction_rounding) on the update, `floor` absolute (float32 underflow).
    `upd_terms`: the update's absolute terms where they are not |upd| itself: the update is a ratio exp_avg / denominator, so
    when b1 m and (1 - b1) g cancel in exp_avg its terms are (b1 |m| + (1 - b1) |g|) / |exp_avg| times larger than it."""
    p, gc, m, v = (np.abs(np.asarray(a, np.float64)) for a in (p, gc, m, v))
    t1, t2 = b1 * m, (1 - b1) * gc
    tol_m = 8 * F32_EPS * (t1 + t2) + rcoef * t2 + floor
    t1, t2 = b2 * v, (1 - b2) * gc * gc
    tol_v = 8 * F32_EPS * (t1 + t2) + 2 * rcoef * t2 + floor
    tol_p = 8 * F32_EPS * (p + (upd if upd_terms is None else upd_terms)) + (2 * rcoef + rbias) * upd + floor
    return tol_m, tol_v, tol_p


def run_clip_adam(be, n, p, g, m, v, max_norm, guard=(0.0, 0.0), partials=None):
    lr, b1, b2, eps = HYPER
    P, G, M, V = be.put(p), be.put(g), be.put(m), be.put(v)
    scratch = np.zeros(4096, np.float32)
    if partials is not None:
        scratch[2:2 + len(partials)] = partials
    scratch, gd = be.put(scratch), be.put(np.asarray(guard, np.float32))
    rc = call_rc(be, "dvs_clip_adam" if partials is None else "dvs_clip_adam_from_partials", n=n, params=P, grads=G, exp_avg=M,
                 exp_avg_sq=V, lr=lr, beta1=b1, beta2=b2, adam_eps=eps, step=ADAM_STEP, max_norm=float(max_norm), scratch=scratch,
                 guard=gd)
    return rc, be.get(P).copy(), be.get(G).copy(), be.get(M).copy(), be.get(V).copy(), be.get(scratch).copy()


def check_clip_adam(be, n):
    """dvs_clip_adam and dvs_clip_adam_from_partials at step 7 from non-zero moments against the float64 torch reference.

    Tolerances.  scratch[0] (sum of squares, a 256-way float32 tree): 1e-6 relative, as tests/test_emu_backward.py.  The
    coefficient max_norm / (sqrt(ss) + 1e-6) inherits half of that plus its own roundings: rc = 0.5e-6 + 4 * 2^-24.
    Every element of a float32 result is allowed 8 * 2^-24 of the absolute terms it is made of (the kernel does at most 8
    roundings per quantity; no term cancels in the gradient or the moments, so there that is 8 * 2^-24 |value|) plus the
    propagated coefficient error on the terms that are scaled by it: the clipped gradient g c once, exp_avg's
    (1 - b1) g c once, exp_avg_sq's (1 - b2) (g c)^2 twice, the parameter update (a ratio m / sqrt(v)) at most twice; a
    parameter's absolute terms are |p| and |update|.  The library's float32 bias corrections 1 - powf(b, 7) (the subtraction
    amplifies powf's rounding by b^7 / (1 - b^7), 142 for b = 0.999: about 4e-6 of the update) get no term of their own:
    they fit inside 8 * 2^-24 |p| here (measured worst |P - ref| / tolerance: 0.14 on the emulator build); at small steps
    they do not, and tests/train_steps_common.py adds bias_correction_rounding.  adam_tolerances holds the arithmetic."""
    lr, b1, b2, eps = HYPER
    p, g, m, v, max_norm = adam_inputs(n)
    norm, cg, cm, cv, cp = clip_adam_ref(p, g, m, v, max_norm)
    coef = float(max_norm) / (norm + 1e-6)
    assert 0.09 < coef < 0.11
    ss = float((g.astype(np.float64) ** 2).sum())
    rcoef = 0.5e-6 + 4 * F32_EPS
    parts = np.array([(g[256 * i:256 * i + 256].astype(np.float64) ** 2).sum() for i in range(sq_parts(n))], np.float32)
    worst = 0.0
    for partials in (None, parts):
        tag = (n, "from_partials" if partials is not None else "clip_adam")
        rc, P, G, M, V, scratch = run_clip_adam(be, n, p, g, m, v, max_norm, partials=partials)
        assert rc == 0, tag
        assert abs(float(scratch[0]) - ss) <= 1e-6 * ss, (tag, "sum of squares", float(scratch[0]), ss)
        assert abs(float(scratch[1]) - coef) <= rcoef * coef, (tag, "coefficient", float(scratch[1]), coef)
        gc = np.abs(cg)
        assert (np.abs(G - cg) <= (8 * F32_EPS + rcoef) * gc).all(), (tag, "clipped gradient")
        upd = np.abs(cp - p.astype(np.float64))
        tol_m, tol_v, tol = adam_tolerances(p, gc, m, v, upd, b1, b2, rcoef=rcoef)
        assert (np.abs(M - cm) <= tol_m).all(), (tag, "exp_avg")
        assert (np.abs(V - cv) <= tol_v).all(), (tag, "exp_avg_sq")
        assert (np.abs(P - cp) <= tol).all(), (tag, "parameters", float((np.abs(P - cp) / tol).max()))
        assert (upd > 1e-3).all()                   # the update is visible in float32 next to |p| <= 2
        worst = max(worst, float((np.abs(P - cp) / tol).max()))
        # a raised guard leaves all four buffers as they were
        for guard in ((1.0, 0.0), (0.0, 1.0)):
            rc, P, G, M, V, _ = run_clip_adam(be, n, p, g, m, v, max_norm, guard=guard, partials=partials)
            assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in ((P, p), (G, g), (M, m), (V, v))), (tag, guard)
    # max_norm <= 0: no clipping, the gradient stays bitwise as it was
    for off in (0.0, -1.0):
        rc, P, G, M, V, scratch = run_clip_adam(be, n, p, g, m, v, off)
        assert rc == 0 and G.tobytes() == g.tobytes() and float(scratch[1]) == 1.0, (n, off)
        assert abs(float(scratch[0]) - ss) <= 1e-6 * ss
    return worst          # worst |P - ref| / tolerance
