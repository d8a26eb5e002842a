"""Conditional Gaussian networks on mixed data (include/dvs_mixed.h; csrc/dvs_mixed.h): the cases, the references and the checks
that tests/test_emu_mixed.py runs on the host emulator and tests/test_gpu_mixed.py on the device, through the raw ABI by
argument name on one back end (scoring_corpus.EmuBackend / GpuBackend).

Partition.  count, start and order against numpy's stable argsort of the integer keys, exactly.
Moments.    every block, as bytes, against dvs_gbn_moments with rows= the segment, and within gaussian_corpus' moment bound of
            the exact rationals.
Scores.     mpmath at 60 digits per configuration (gaussian_corpus.Reference on each configuration's exact moments, the terms
            summed) and, on the CPU, numpy.linalg.lstsq on the raw rows per configuration.  No tolerance is fitted to an output:
            the bound of a family is the sum over its non-empty configurations of Reference.local's bound for loglik-g, plus
            gamma(q' + 1) sum |LL_z| for the q' - 1 additions of the sum (and the one onto +0, which is exact), plus the
            penalty's roundings: k q and (k q)(p + 2) are two, the subtraction a third, bic's default k = log(S) / 2 one more
            (the library's log is taken as correctly rounded within one ulp): 4 U |penalty| + 2 U |local|.  Each
            configuration's conditioning (KAPPA_CAP) and eta (ETA_CAP) are asserted inside Reference.local, from the
            reference, before any device value is read.
Fit.        coefficients, intercept and sd per configuration within Reference.fit's bounds of mpmath's lu_solve.
"""
import ctypes
import functools
import math

import mpmath as mp
import numpy as np

from dags_vae_search_amd import _lib as dl
from tests import gaussian_corpus as gc
from tests import scoring_corpus as sc

U64, U, NAN, SENTINEL = np.uint64, gc.U, gc.NAN, gc.SENTINEL
CHUNK, CAP = gc.CHUNK, gc.CAP
ISENT = -7777
MAXQ = dl.CG_MAX_CONFIGS
TYPES = ("loglik-cg", "aic-cg", "bic-cg")
GAUSS_OF = {"loglik-cg": "loglik-g", "aic-cg": "aic-g", "bic-cg": "bic-g"}
DISC_OF = {"loglik-cg": "loglik", "aic-cg": "aic", "bic-cg": "bic"}
VARIANTS = (("loglik-cg", None), ("aic-cg", None), ("aic-cg", 0.3), ("bic-cg", None), ("bic-cg", 2.5))


class Mixed:
    """a mixed data set: ``card`` [n] (0: continuous), ``levels`` uint8 [S, n] (0 in real columns), ``x`` f64 [S, n_cont]"""

    def __init__(self, card, levels, x):
        self.card = np.asarray(card, np.uint8)
        self.n, self.S = len(card), len(levels)
        self.levels, self.x = np.asarray(levels, np.uint8), np.ascontiguousarray(x, np.float64).reshape(self.S, -1)
        self.cvars = [v for v in range(self.n) if card[v] == 0]
        self.dvars = [v for v in range(self.n) if card[v] != 0]
        self.nc = len(self.cvars)
        assert self.x.shape == (self.S, self.nc)
        self.packed = sc.pack(self.levels)
        self.col = {v: j for j, v in enumerate(self.cvars)}

    def q(self, D):
        return int(np.prod([int(self.card[v]) for v in gc.bits_of(D)], dtype=object)) if D else 1

    def keys(self, D):
        key, stride = np.zeros(self.S, np.int64), 1
        for v in gc.bits_of(D):
            key += self.levels[:, v].astype(np.int64) * stride
            stride *= int(self.card[v])
        return key

    def segments(self, D):
        """the row indices of every configuration of D, each ascending"""
        key = self.keys(D)
        return [np.nonzero(key == z)[0].astype(np.int32) for z in range(self.q(D))]


@functools.lru_cache(maxsize=None)
def mixed_data(cards, nc, S, seed=0, interleave=True):
    """factors with the level counts ``cards`` (dependent columns: scoring_corpus.synthetic_dataset) and ``nc`` real columns
    (gaussian_corpus.gauss_data) shifted by the levels of the first two factors, so that a mixed-up configuration shows; with
    ``interleave`` the kinds alternate as far as they go"""
    nd = len(cards)
    lev, _ = sc.synthetic_dataset(nd, S, list(cards), 3200 + seed) if nd else (np.zeros((S, 0), np.uint8), None)
    x = np.array(gc.gauss_data(nc, S, seed)) if nc else np.zeros((S, 0))
    for j in range(nc):
        for d in range(min(nd, 2)):
            x[:, j] = x[:, j] + 0.25 * (j % 3 + 1) * (d + 1) * lev[:, d]
    kinds, di, ci = [], 0, 0
    while di < nd or ci < nc:
        if di < nd and (not interleave or ci >= nc or di <= ci):
            kinds.append(("d", di))
            di += 1
        else:
            kinds.append(("c", ci))
            ci += 1
    n = nd + nc
    card = [cards[i] if k == "d" else 0 for k, i in kinds]
    levels = np.zeros((S, n), np.uint8)
    for v, (k, i) in enumerate(kinds):
        if k == "d":
            levels[:, v] = lev[:, i]
    xs = np.stack([x[:, i] for k, i in kinds if k == "c"], 1) if nc else np.zeros((S, 0))
    return Mixed(card, levels, xs)


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI by argument name
# ---------------------------------------------------------------------------------------------------------------------
def run_partition(be, md, masks, q_pitch, guard=1):
    """dvs_cg_partition between sentinel rows -> (count [R, q_pitch], start, order [R, S], status)"""
    R, S = len(masks), md.S
    count, start = be.put(np.full((R + 2 * guard, q_pitch), ISENT, np.int32)), be.put(np.full((R + 2 * guard, q_pitch), ISENT, np.int32))
    order, status = be.put(np.full((R + 2 * guard, S), ISENT, np.int32)), be.put(np.zeros(1, np.int32))
    off = lambda h, w: ctypes.c_void_p(be.ptr(h).value + guard * w * 4)
    gc.call(be, "dvs_cg_partition", n_vars=md.n, n_samples=S, data=be.put(md.packed), card=be.put(md.card), n_requests=R,
            masks=be.put(np.asarray(masks, U64)), q_pitch=q_pitch, count=off(count, q_pitch), count_bytes=R * q_pitch * 4,
            start=off(start, q_pitch), order=off(order, S), order_bytes=R * S * 4, status=status)
    c, s, o = (np.array(be.get(h), copy=True) for h in (count, start, order))
    for a in (c, s, o):
        assert (a[:guard] == ISENT).all() and (a[R + guard:] == ISENT).all(), "the partition wrote outside its rows"
    return c[guard:R + guard], s[guard:R + guard], o[guard:R + guard], int(be.get(status)[0])


def run_cg_moments(be, md, count, start, order, q_pitch, guard=1):
    """dvs_cg_moments between sentinel blocks -> f64 [R, q_pitch, stride]"""
    R, st = len(count), gc.stride(md.nc)
    need = be.lib.dvs_cg_moments_workspace_bytes(md.nc, md.S, R, q_pitch)
    slots = -(-md.S // CHUNK) + q_pitch
    assert need == 8 * ((q_pitch + 2) // 2) * R + 8 * R * slots * (md.nc + md.nc * (md.nc + 1) // 2), need
    ws, mom = be.put(np.zeros(need, np.uint8)), be.put(np.full((R + 2 * guard, q_pitch, st), SENTINEL))
    gc.call(be, "dvs_cg_moments", n_cont=md.nc, n_samples=md.S, x=be.put(md.x), n_requests=R, q_pitch=q_pitch, count=be.put(count),
            start=be.put(start), order=be.put(order), workspace=ws, workspace_bytes=need,
            moments=ctypes.c_void_p(be.ptr(mom).value + guard * q_pitch * st * 8), moments_bytes=R * q_pitch * st * 8)
    m = np.array(be.get(mom), copy=True)
    assert (m[:guard] == SENTINEL).all() and (m[R + guard:] == SENTINEL).all(), "the moments wrote outside their blocks"
    return m[guard:R + guard]


class Tables:
    """the tables of a list of sets D on a back end: what the host side of mixed.py keeps in its cache"""

    def __init__(self, be, md, masks):
        self.be, self.md, self.masks = be, md, [int(m) for m in masks]
        self.index = {m: i for i, m in enumerate(self.masks)}
        self.host, self.handles = [], []
        if md.nc == 0:
            return
        self.host = [None] * len(self.masks)
        for q in sorted({md.q(m) for m in self.masks}):                  # one launch per q: the requests of a call share a pitch
            mine = [i for i, m in enumerate(self.masks) if md.q(m) == q]
            c, s, o, st = run_partition(be, md, [self.masks[i] for i in mine], q)
            assert st == 0
            mom = run_cg_moments(be, md, c, s, o, q)
            for j, i in enumerate(mine):
                self.host[i] = mom[j]
        self.handles = [be.put(t) for t in self.host]                     # the handles stay alive with this object
        self.addresses = be.put(np.asarray([be.ptr(h).value for h in self.handles] or [0], U64))

    def of(self, masks):
        """int32 like ``masks``: the table of each D, -1 for a negative entry or one that has no table"""
        return np.vectorize(lambda m: self.index.get(int(m), -1) if m >= 0 else -1, otypes=[np.int32])(np.asarray(masks, np.int64))


def family_masks(md, P):
    """D of every family [B, n] of the structures P; -1 on the rows of discrete variables"""
    P = np.asarray(P, U64)
    disc = U64(gc.mask_of(md.dvars))
    D = (P & disc).astype(np.int64)
    D[:, md.dvars] = -1
    return D


def tables_for(be, md, masks):
    wanted = sorted({int(m) for m in np.asarray(masks).ravel() if m >= 0 and md.q(int(m)) <= MAXQ})
    return Tables(be, md, wanted)


def _score_args(typ, k):
    return dict(score_type=dl.CGSCORE_TYPES[typ], score_arg=NAN if k is None else float(k))


def _common(be, md, tb, table_of):
    nothing = md.nc == 0
    return dict(n_vars=md.n, n_cont=md.nc, n_samples=md.S, data=be.put(md.packed), card=be.put(md.card),
                tables=None if nothing else tb.addresses, table_of=None if nothing else be.put(np.ascontiguousarray(table_of, np.int32)))


def run_scores(be, md, P, typ, k=None, tb=None, guard=1):
    """dvs_cg_scores -> (local [B, n], out [B], status), local between sentinel rows"""
    P = np.ascontiguousarray(P, U64)
    B, n = P.shape
    D = family_masks(md, P)
    tb = tables_for(be, md, D) if tb is None else tb
    need = be.lib.dvs_cg_scores_workspace_bytes(B, n)
    assert need == 8 * B * n + 64
    local, out, status = be.put(np.full((B + 2 * guard, n), SENTINEL)), be.put(np.full(B, SENTINEL)), be.put(np.zeros(1, np.int32))
    gc.call(be, "dvs_cg_scores", batch=B, parents=be.put(P), workspace=be.put(np.zeros(need, np.uint8)), workspace_bytes=need,
            local=ctypes.c_void_p(be.ptr(local).value + guard * n * 8), out=out, status=status, **_common(be, md, tb, tb.of(D)),
            **_score_args(typ, k))
    loc = np.array(be.get(local), copy=True)
    assert (loc[:guard] == SENTINEL).all() and (loc[B + guard:] == SENTINEL).all()
    return loc[guard:B + guard], np.array(be.get(out), copy=True), int(be.get(status)[0])


def toggle_masks(md, P, worklist=None):
    """D of every cell of a pass: [B * n, n], or [2 B, n] by worklist slot; -1 where no table is read"""
    P = np.asarray(P, U64)
    B, n = P.shape
    D = family_masks(md, P)
    if worklist is None:
        rows = D.reshape(B * n)
    else:
        rows = np.asarray([D[s // 2, v] if 0 <= v < n else -1 for s, v in enumerate(worklist)], np.int64)
    flip = np.asarray([(1 << u) if md.card[u] else 0 for u in range(n)], np.int64)
    return np.where(rows[:, None] >= 0, rows[:, None] ^ flip[None, :], -1)


def run_toggle(be, md, P, typ, k=None, worklist=None, tables=None, tb=None):
    P = np.ascontiguousarray(P, U64)
    B, n = P.shape
    cells = toggle_masks(md, P, worklist)
    tb = tables_for(be, md, cells) if tb is None else tb
    L0, T0 = (np.full((B, n), SENTINEL), np.full((B, n, n), SENTINEL)) if tables is None else tables
    L, T, status = be.put(L0), be.put(T0), be.put(np.zeros(1, np.int32))
    need = be.lib.dvs_cg_toggle_workspace_bytes(B, n)
    assert need == 8 * B * n + 64 + 8 * B
    gc.call(be, "dvs_cg_toggle_scores", batch=B, parents=be.put(P), worklist=None if worklist is None else be.put(np.asarray(worklist, np.int32)),
            workspace=be.put(np.zeros(need, np.uint8)), workspace_bytes=need, local=L, local_bytes=B * n * 8, toggles=T,
            toggles_bytes=B * n * n * 8, status=status, **_common(be, md, tb, tb.of(cells)), **_score_args(typ, k))
    return np.array(be.get(L), copy=True), np.array(be.get(T), copy=True), int(be.get(status)[0])


def run_bn_scores(be, md, P, typ, k=None):
    """dvs_bn_scores on the packed rows with the factors' level counts (a real column counts as one level)"""
    P = np.ascontiguousarray(P, U64)
    B, n = P.shape
    card = np.where(md.card == 0, 1, md.card).astype(np.uint8)
    local, out, status = be.put(np.full((B, n), SENTINEL)), be.put(np.full(B, SENTINEL)), be.put(np.zeros(1, np.int32))
    gc.call(be, "dvs_bn_scores", batch=B, n_vars=n, n_samples=md.S, data=be.put(md.packed), card=be.put(card), parents=be.put(P),
            score_type=dl.SCORE_TYPES[DISC_OF[typ]], score_arg=NAN if k is None else float(k), scratch=local, out=out, status=status)
    return np.array(be.get(local), copy=True), np.array(be.get(out), copy=True), int(be.get(status)[0])


def run_fit(be, md, fams, tb=None):
    """dvs_cg_fit for the continuous families [(v, parent mask)] -> (coef [cells, n], intercept, sd, count, offset, status)"""
    F = len(fams)
    Ds = [pm & gc.mask_of(md.dvars) & ~(1 << v) for v, pm in fams]
    tb = tables_for(be, md, Ds) if tb is None else tb
    offset = np.concatenate([[0], np.cumsum([md.q(D) for D in Ds])]).astype(np.int64)
    cells = int(offset[-1])
    addr = np.asarray([be.ptr(tb.handles[tb.index[D]]).value for D in Ds], U64)
    coef, status = be.put(np.full((cells + 2, md.n), SENTINEL)), be.put(np.zeros(1, np.int32))
    icpt, sd, cnt = (be.put(np.full(cells + 1, SENTINEL)) for _ in range(3))
    gc.call(be, "dvs_cg_fit", n_families=F, n_cells=cells, n_vars=md.n, n_cont=md.nc, card=be.put(md.card),
            var=be.put(np.asarray([v for v, _ in fams], np.int32)), parents=be.put(np.asarray([pm for _, pm in fams], U64)),
            table=be.put(addr), offset=be.put(offset), coef=ctypes.c_void_p(be.ptr(coef).value + md.n * 8), coef_bytes=cells * md.n * 8,
            intercept=icpt, sd=sd, count=cnt, status=status)
    c, i, s, m = (np.array(be.get(h), copy=True) for h in (coef, icpt, sd, cnt))
    assert (c[0] == SENTINEL).all() and (c[-1] == SENTINEL).all() and i[-1] == s[-1] == m[-1] == SENTINEL
    return c[1:-1], i[:-1], s[:-1], m[:-1], offset, int(be.get(status)[0])


# ---------------------------------------------------------------------------------------------------------------------
# Partition
# ---------------------------------------------------------------------------------------------------------------------
PARTITION_CARDS = (3, 4, 16, 2, 1, 16)
PARTITION_S = (1, 37, 256, 257, 1000)


def partition_case(S):
    return mixed_data(PARTITION_CARDS, 3, S)


def partition_requests(md):
    d = md.dvars
    return [0, 1 << d[0], 1 << d[2], 1 << d[4], (1 << d[1]) | (1 << d[3]), (1 << d[0]) | (1 << d[5]), (1 << d[0]) | (1 << d[1]) | (1 << d[3]),
            (1 << d[2]) | (1 << d[3]) | (1 << d[5])]


def expect_partition(md, D, q_pitch):
    key = md.keys(D)
    count = np.bincount(key, minlength=q_pitch).astype(np.int32)
    return count, (np.cumsum(count) - count).astype(np.int32), np.argsort(key, kind="stable").astype(np.int32)


def check_partition_requests(be, md, masks):
    q_pitch = max(md.q(D) for D in masks if not D >> md.n)
    count, start, order, status = run_partition(be, md, masks, q_pitch)
    again = run_partition(be, md, masks, q_pitch)
    refused = [D for D in masks if D >> md.n]
    assert status == (16 if refused else 0)
    for r, D in enumerate(masks):
        if D in refused:
            assert count[r, 0] == -1 and (count[r, 1:] == ISENT).all() and (start[r] == ISENT).all() and (order[r] == ISENT).all()
            continue
        wc, ws, wo = expect_partition(md, D, q_pitch)
        assert np.array_equal(count[r], wc) and np.array_equal(start[r], ws), (md.S, hex(D))
        assert np.array_equal(order[r], wo), (md.S, hex(D))
    assert all(a.tobytes() == b.tobytes() for a, b in zip((count, start, order), again[:3]))


def check_partition(be, S):
    md = partition_case(S)
    check_partition_requests(be, md, partition_requests(md))


@functools.lru_cache(maxsize=None)
def wide_case():
    """n = 48 with the factors 15, 16 and 33, one in each packed word"""
    S = 300
    rng = np.random.default_rng(3248)
    card = np.zeros(48, np.uint8)
    card[[15, 16, 33]] = (5, 16, 3)
    levels = np.zeros((S, 48), np.uint8)
    for v in (15, 16, 33):
        levels[:, v] = rng.integers(0, card[v], S)
    return Mixed(card, levels, gc.gauss_data(45, S))


def check_partition_wide(be):
    md = wide_case()
    b = [1 << 15, 1 << 16, 1 << 33]
    check_partition_requests(be, md, [0, b[0], b[1], b[2], b[0] | b[1], b[1] | b[2], b[0] | b[1] | b[2]])


def check_partition_spans(be):
    """8193 rows: a request is cut into three spans of 4096 rows (csrc/dvs_mixed.h: CG_SPAN), the last one a single row"""
    md = mixed_data(PARTITION_CARDS, 1, 2 * 4096 + 1)
    d = md.dvars
    check_partition_requests(be, md, [0, 1 << d[0], (1 << d[1]) | (1 << d[3]), (1 << d[2]) | (1 << d[5]), 1 << 63])


def check_partition_refusals(be):
    """q = 4096 accepted, 16^4 refused; a continuous variable; a bit at or above n; q > q_pitch: each refuses its own request"""
    S = 64
    rng = np.random.default_rng(3277)
    card = np.asarray([16, 16, 16, 16, 0, 2], np.uint8)
    levels = np.zeros((S, 6), np.uint8)
    for v in (0, 1, 2, 3, 5):
        levels[:, v] = rng.integers(0, card[v], S)
    md = Mixed(card, levels, rng.normal(size=(S, 1)))
    masks = [0b000111, 0b001111, 0b010001, 0b100000, 1 << 6, 1 << 63, 0b100001]
    count, start, order, status = run_partition(be, md, masks, MAXQ)
    assert status == 16
    for r, D in enumerate(masks):
        if r in (0, 3, 6):
            wc, ws, wo = expect_partition(md, D, MAXQ)
            assert np.array_equal(count[r], wc) and np.array_equal(start[r], ws) and np.array_equal(order[r], wo), r
        else:
            assert count[r, 0] == -1 and (count[r, 1:] == ISENT).all() and (start[r] == ISENT).all() and (order[r] == ISENT).all(), r
    count, _, _, status = run_partition(be, md, [0b100001, 0b000011], 32)
    assert status == 16 and count[0, 0] >= 0 and count[1, 0] == -1          # 256 configurations at q_pitch = 32


# ---------------------------------------------------------------------------------------------------------------------
# Moments
# ---------------------------------------------------------------------------------------------------------------------
LEVEL_COUNTS = (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)


@functools.lru_cache(maxsize=None)
def moments_case(nc):
    """one six-level factor whose levels occur exactly LEVEL_COUNTS times, in interleaved positions, and nc real columns"""
    col = np.concatenate([np.full(c, z, np.uint8) for z, c in enumerate(LEVEL_COUNTS)])
    S = len(col)
    col = col[np.random.default_rng(3300 + nc).permutation(S)]
    levels = np.zeros((S, 1 + nc), np.uint8)
    levels[:, 0] = col
    return Mixed([6] + [0] * nc, levels, gc.gauss_data(nc, S, seed=1))


def check_moments(be, nc):
    md = moments_case(nc)
    q_pitch = 8                                              # two blocks past q: empty as well
    count, start, order, status = run_partition(be, md, [1, 0], q_pitch)
    assert status == 0 and list(count[0, :6]) == list(LEVEL_COUNTS)
    mom = run_cg_moments(be, md, count, start, order, q_pitch)
    assert mom.tobytes() == run_cg_moments(be, md, count, start, order, q_pitch).tobytes()
    worst = 0.0
    empty = np.zeros(gc.stride(nc))
    for z, seg in enumerate(md.segments(1)):
        if len(seg) == 0:
            assert mom[0, z].tobytes() == empty.tobytes(), "an empty configuration is m = 0 and +0"
            continue
        assert np.array_equal(order[0, start[0, z]:start[0, z] + count[0, z]], seg)
        assert mom[0, z].tobytes() == gc.run_moments(be, md.x, seg[None, :])[0].tobytes(), (nc, z)
        worst = max(worst, gc.moments_against_exact(mom[0, z], gc.ExactMoments(md.x[seg])))
    assert mom[0, 6:].tobytes() == np.zeros((2, gc.stride(nc))).tobytes()
    assert mom[1, 0].tobytes() == gc.run_moments(be, md.x)[0].tobytes(), "D = {} is dvs_gbn_moments on all rows"
    assert mom[1, 1:].tobytes() == np.zeros((q_pitch - 1, gc.stride(nc))).tobytes()
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# Scores against mpmath
# ---------------------------------------------------------------------------------------------------------------------
SCORE_CARDS = (2, 3, 4)
SCORE_NC = CAP + 2


@functools.lru_cache(maxsize=None)
def score_case():
    """factors 0, 1, 2 (2, 3, 4 levels) in a full cross, 30 rows a cell, next to CAP + 2 real columns: D = {0} has q = 2 and 360
    rows a configuration, D = {1, 2} q = 12 and 60 rows >= 4 (CAP + 2)"""
    S = 720
    s = np.random.default_rng(3400).permutation(S)
    levels = np.zeros((S, 3 + SCORE_NC), np.uint8)
    levels[:, 0], levels[:, 1], levels[:, 2] = s % 2, (s // 2) % 3, (s // 6) % 4
    x = np.array(gc.gauss_data(SCORE_NC, S, seed=2))
    for j in range(SCORE_NC):
        x[:, j] = x[:, j] + 0.25 * (j % 3 + 1) * levels[:, 0] + 0.125 * (j % 5) * levels[:, 2]
    return Mixed(list(SCORE_CARDS) + [0] * SCORE_NC, levels, x)


def score_families():
    """(v, D, continuous parents as variables): q in {1, 2, 12} x p in {0, 2, CAP}"""
    c = list(range(3, 3 + SCORE_NC))
    fams = []
    for D in (0, 0b001, 0b110):
        fams += [(c[0], D, []), (c[4], D, [c[1], c[7]]), (c[CAP], D, c[:CAP])]
    return fams


@functools.lru_cache(maxsize=None)
def config_reference(case, D, z):
    """gaussian_corpus.Reference on the exact moments of configuration z of D, with the mean the header's summation gives"""
    md = case()
    seg = md.segments(D)[z]
    rows = np.ascontiguousarray(md.x[seg])
    return gc.Reference(gc.ExactMoments(rows), gc.restated_moments(rows)[0, 1:1 + md.nc]), rows


@gc.at60
def reference_local(case, v, D, G, typ, k=None):
    """(local score as mpf, bound) of the continuous family; None where the definition refuses it.  Asserts every
    configuration's conditioning and eta (Reference.logdet_bound) on the way."""
    md = case()
    q, p = md.q(D), len(G)
    terms, bound = [], 0.0
    for z in range(q):
        if len(md.segments(D)[z]) == 0:
            continue
        ref, _ = config_reference(case, D, z)
        want, b = ref.local(md.col[v], [md.col[u] for u in G], "loglik-g")
        if want is None:
            return None, None
        terms.append(want)
        bound += b
    ll = sum(terms, mp.mpf(0))
    bound += gc.gamma(len(terms) + 1) * float(sum(abs(t) for t in terms))
    if typ == "loglik-cg":
        return ll, bound + 2 * U * float(abs(ll))
    kk = (mp.log(md.S) / 2 if typ == "bic-cg" else mp.mpf(1)) if k is None else mp.mpf(k)
    pen = kk * q * (p + 2)
    local = ll - pen
    return local, bound + 4 * U * float(abs(pen)) + 2 * U * float(abs(local))


def lstsq_local(case, v, D, G, typ, k=None):
    """the independent float64 route: numpy.linalg.lstsq on the raw rows of every configuration"""
    md = case()
    q, p = md.q(D), len(G)
    ll = 0.0
    for z in range(q):
        seg = md.segments(D)[z]
        if len(seg):
            ll += gc.lstsq_family(md.x[seg], md.col[v], [md.col[u] for u in G], "loglik-g")
    if typ == "loglik-cg":
        return ll
    kk = (math.log(md.S) / 2.0 if typ == "bic-cg" else 1.0) if k is None else k
    return ll - kk * q * (p + 2.0)


@gc.at60
def check_scores(be):
    """every family of score_families under every variant against mpmath; -> the largest error / bound"""
    md, fams = score_case(), score_families()
    wants = {(i, var): reference_local(score_case, v, D, G, var[0], var[1]) for i, (v, D, G) in enumerate(fams) for var in VARIANTS}
    P = np.zeros((len(fams), md.n), U64)
    for b, (v, D, G) in enumerate(fams):
        P[b, v] = U64(D | gc.mask_of(G) | (1 << v) * (b & 1))            # the self bit is ignored
    tb = tables_for(be, md, family_masks(md, P))
    worst = 0.0
    for var in VARIANTS:
        local, out, status = run_scores(be, md, P, var[0], var[1], tb=tb)
        assert status == 0 and local.tobytes() == run_scores(be, md, P, var[0], var[1], tb=tb)[0].tobytes()
        for b, (v, D, G) in enumerate(fams):
            want, bound = wants[(b, var)]
            err = float(abs(mp.mpf(float(local[b, v])) - want))
            assert err <= bound, (var, v, D, G, float(local[b, v]), float(want), err, bound)
            worst = max(worst, err / bound)
            total = 0.0
            for w in range(md.n):
                total = total + float(local[b, w])
            assert np.float64(total).tobytes() == out[b].tobytes()
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# Byte identities
# ---------------------------------------------------------------------------------------------------------------------
def check_identities(be):
    # all variables continuous: dvs_gbn_scores on the moments of all rows
    n, S = 5, CHUNK + 1
    x = gc.gauss_data(n, S)
    md = Mixed([0] * n, np.zeros((S, n), np.uint8), x)
    P = gc.random_dags(n, 6, 3, seed=4)
    mom = gc.run_moments(be, x)
    for typ, k in VARIANTS:
        local, out, status = run_scores(be, md, P, typ, k)
        gl, go, gs = gc.run_scores(be, mom, n, P, GAUSS_OF[typ], k)
        assert status == gs == 0 and local.tobytes() == gl.tobytes() and out.tobytes() == go.tobytes(), typ
    # all variables discrete: dvs_bn_scores
    data, card = sc.synthetic_dataset(6, 500, [3, 4, 16, 2, 1, 16], 3500)
    md = Mixed(card, data, np.zeros((500, 0)))
    P = gc.random_dags(6, 6, 3, seed=5)
    for typ, k in VARIANTS:
        local, out, status = run_scores(be, md, P, typ, k)
        bl, bo, bs = run_bn_scores(be, md, P, typ, k)
        assert status == bs == 0 and local.tobytes() == bl.tobytes() and out.tobytes() == bo.tobytes(), typ
    # mixed data: a continuous v with D = {} is the Gaussian scorer's cell on the real columns, a discrete v the discrete scorer's
    md = partition_case(257)
    c, d = md.cvars, md.dvars
    P = np.zeros((3, md.n), U64)
    P[0, c[2]] = U64(gc.mask_of([c[0], c[1]]))
    P[1, c[0]] = U64(gc.mask_of([c[1]]))
    P[1, d[2]] = U64(gc.mask_of([d[0], d[1]]))
    P[2, d[3]] = U64(gc.mask_of([d[2], d[5]]))
    P[2, c[1]] = U64(gc.mask_of([d[0], c[0]]))
    mom = gc.run_moments(be, md.x)
    PG = np.zeros((3, md.nc), U64)
    PG[0, 2], PG[1, 0] = U64(0b011), U64(0b010)
    PD = P.copy()
    PD[:, c] = U64(0)
    for typ, k in VARIANTS:
        local, out, status = run_scores(be, md, P, typ, k)
        gl, _, _ = gc.run_scores(be, mom, md.nc, PG, GAUSS_OF[typ], k)
        bl, _, _ = run_bn_scores(be, md, PD, typ, k)
        assert status == 0
        assert local[:, d].tobytes() == bl[:, d].tobytes(), typ
        assert local[:2, c].tobytes() == gl[:2].tobytes() and local[2, [c[0], c[2]]].tobytes() == gl[2, [0, 2]].tobytes(), typ
        assert local[2, c[1]] != gl[2, 1]


# ---------------------------------------------------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refusal_case():
    """variables: factors 0 (3 levels), 1 .. 4 (16 levels each); real columns 5 .. 17 (CAP + 2).  Level 2 of factor 0 has 3 rows
    (1 <= m <= p + 1 with two parents); inside level 1 of factor 0 alone column 7 duplicates column 6"""
    S = 400
    rng = np.random.default_rng(3600)
    levels = np.zeros((S, 5 + SCORE_NC), np.uint8)
    f0 = np.asarray([0] * 200 + [1] * 197 + [2] * 3, np.uint8)
    levels[:, 0] = f0[rng.permutation(S)]
    levels[:, 1] = rng.integers(0, 16, S)                    # factors 2 .. 4 follow factor 1: 16 of the 4096 configurations hold rows
    levels[:, 2], levels[:, 3], levels[:, 4] = (3 * levels[:, 1] + 1) % 16, (5 * levels[:, 1] + 2) % 16, 15 - levels[:, 1]
    x = np.array(gc.gauss_data(SCORE_NC, S, seed=3))
    dup = levels[:, 0] == 1
    x[dup, 2] = x[dup, 1]
    return Mixed([3, 16, 16, 16, 16] + [0] * SCORE_NC, levels, x)


def refusal_cases():
    """[(name, v, parent mask, refused)]"""
    c = list(range(5, 5 + SCORE_NC))
    m = gc.mask_of
    return [("a configuration with 1 .. p + 1 rows", c[5], m([0, c[3], c[4]]), True),
            ("the same parents without the factor", c[5], m([c[3], c[4]]), False),
            ("three rows hold one regressor less", c[5], m([0, c[3]]), False),
            ("a column duplicated inside one configuration", c[2], m([0, c[1]]), True),
            ("the duplicate is not one over all rows", c[2], m([c[1]]), False),
            ("q = 4096", c[0], m([1, 2, 3]), False),
            ("16^4 configurations", c[0], m([1, 2, 3, 4]), True),
            ("a continuous parent of a discrete node", 1, m([0, c[0]]), True),
            ("a discrete parent of a discrete node", 1, m([0]), False),
            ("a bit at or above n", c[0], m([c[1]]) | (1 << 18), True),
            ("bit 63", c[0], 1 << 63, True),
            ("a bit at or above n on a discrete node", 0, 1 << 20, True),
            ("p = CAP", c[CAP], m(c[:CAP]), False),
            ("p = CAP + 1", c[CAP], m(c[:CAP] + [c[CAP + 1]]), True)]


def check_refusals(be):
    """every case as the middle structure of three, sentinels around the buffers: NaN and bit 4 for its own family alone"""
    md = refusal_case()
    assert md.n == 18
    for name, v, pm, refused in refusal_cases():
        P = np.zeros((3, md.n), U64)
        P[1, v] = U64(pm)
        P[0, 6], P[2, 7] = U64(1), U64(1 << 5)
        for typ in ("loglik-cg", "bic-cg"):
            local, out, status = run_scores(be, md, P, typ)
            want = np.zeros((3, md.n), bool)
            want[1, v] = refused
            assert np.array_equal(np.isnan(local), want), (name, typ, np.argwhere(np.isnan(local)))
            assert status == (16 if refused else 0), (name, typ, status)
            assert np.array_equal(np.isnan(out), want.any(1)), name
        L, T, st = run_toggle(be, md, P, "bic-cg")
        assert L.tobytes() == local.tobytes(), name


# ---------------------------------------------------------------------------------------------------------------------
# Toggles
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def toggle_case(n):
    """about half the variables factors of 2 .. 3 levels; structures from random orders with legal arcs only"""
    S = 3 * CHUNK + 5
    nd = n // 2
    md = mixed_data(tuple([2, 3, 2][i % 3] for i in range(nd)), n - nd, S, seed=n)
    B = {5: 6, 17: 3, 48: 2}[n]
    P = gc.random_dags(n, B, 3, seed=n + 1)
    cont = U64(gc.mask_of(md.cvars))
    for v in md.dvars:
        P[:, v] &= ~cont
    return md, P


def check_toggles(be, n, variants=(("bic-cg", None), ("aic-cg", 0.3))):
    """every cell against the scorer on the flipped structure, as bytes; the NaN pattern; a worklist pass; one shared set of
    tables and a fresh one give equal bytes"""
    md, P = toggle_case(n)
    B = len(P)
    eye = np.eye(n, dtype=bool)
    is_d = md.card != 0
    illegal = np.broadcast_to(is_d[:, None] & ~is_d[None, :], (B, n, n))            # [v, u]: a discrete v, a continuous u
    for typ, k in variants:
        L, T, status = run_toggle(be, md, P, typ, k)
        local, _, st0 = run_scores(be, md, P, typ, k)
        assert L.tobytes() == local.tobytes() and st0 == 0
        # structure (b, u) flips bit u in every row but u's own: its local[v] is the wanted cell (b, v, u)
        flipped = np.repeat(P, n, 0).reshape(B, n, n)
        for u in range(n):
            flipped[:, u, :] ^= U64(1 << u)
            flipped[:, u, u] ^= U64(1 << u)
        fl_local, _, st1 = run_scores(be, md, flipped.reshape(-1, n), typ, k)
        want = fl_local.reshape(B, n, n).transpose(0, 2, 1).copy()          # [B, v, u]
        assert np.isnan(want[illegal]).all(), "the scorer refuses every illegal arc"
        refused = np.isnan(want) & ~illegal & ~eye
        assert np.array_equal(np.isnan(T), eye[None] | illegal | refused), (n, typ)
        assert T[:, ~eye].tobytes() == want[:, ~eye].tobytes(), (n, typ)
        assert (status == 16) == bool(refused.any())
        wl = np.full(2 * B, -1, np.int32)
        for b in range(B):
            wl[2 * b] = (b + 1) % n
            if b % 2 and n > 2:
                wl[2 * b + 1] = (b + 2) % n
        L2, T2, _ = run_toggle(be, md, P, typ, k, worklist=wl)
        named = np.zeros((B, n), bool)
        for s, v in enumerate(wl):
            if v >= 0:
                named[s // 2, v] = True
        assert (L2 == SENTINEL).all() and (T2[~named] == SENTINEL).all()
        off = np.broadcast_to(~eye, (B, n, n)) & named[:, :, None]
        assert T2[off].tobytes() == T[off].tobytes()
        assert (T2[np.broadcast_to(eye, (B, n, n)) & named[:, :, None]] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# Fit
# ---------------------------------------------------------------------------------------------------------------------
@gc.at60
def check_fit(be):
    """coefficients, intercept and sd per configuration against mpmath's lu_solve; the D = {} rows equal dvs_gbn_fit as bytes"""
    md = score_case()
    fams = [(v, D | gc.mask_of(G) | (1 << v)) for v, D, G in score_families()]
    coef, icpt, sd, cnt, offset, status = run_fit(be, md, fams)
    assert status == 0
    worst = [0.0, 0.0, 0.0]
    for f, (v, D, G) in enumerate(score_families()):
        for z in range(md.q(D)):
            cell = int(offset[f]) + z
            ref, rows = config_reference(score_case, D, z)
            assert cnt[cell] == len(rows)
            (beta, c0, s), (cb, ib, sb) = ref.fit(md.col[v], [md.col[u] for u in G])
            for u in range(md.n):
                if u in G:
                    err = float(abs(mp.mpf(float(coef[cell, u])) - beta[md.col[u]]))
                    assert err <= cb, ("coef", v, D, z, u, err, cb)
                    worst[0] = max(worst[0], err / cb)
                else:
                    assert coef[cell, u] == 0.0
            e1, e2 = float(abs(mp.mpf(float(icpt[cell])) - c0)), float(abs(mp.mpf(float(sd[cell])) - s))
            assert e1 <= ib and e2 <= sb, ("intercept / sd", v, D, z, e1, ib, e2, sb)
            worst[1], worst[2] = max(worst[1], e1 / ib), max(worst[2], e2 / sb)
    # D = {}: dvs_gbn_fit on the moments of all rows
    mom = gc.run_moments(be, md.x)
    for f, (v, D, G) in enumerate(score_families()):
        if D == 0:
            P = np.zeros((1, md.nc), U64)
            P[0, md.col[v]] = U64(gc.mask_of([md.col[u] for u in G]))
            gcoef, gi, gs, st = gc.run_fit(be, mom, md.nc, P)
            cell = int(offset[f])
            assert st == 0 and coef[cell, md.cvars].tobytes() == gcoef[0, md.col[v]].tobytes()
            assert icpt[cell].tobytes() == gi[0, md.col[v]].tobytes() and sd[cell].tobytes() == gs[0, md.col[v]].tobytes()
    # an empty configuration is NaN without a status bit; a refused one sets bit 4
    mc = moments_case(5)
    coef, icpt, sd, cnt, offset, status = run_fit(be, mc, [(1, 0b000101)])
    assert status == 16 and list(cnt) == list(LEVEL_COUNTS)
    assert np.isnan(sd[[0, 1]]).all() and not np.isnan(sd[2:]).any() and np.isnan(coef[0]).all() and not np.isnan(coef[2:]).any()
    coef, icpt, sd, cnt, offset, status = run_fit(be, mc, [(1, 0b000001), (3, 0)])
    assert status == 16 and np.isnan(sd[:2]).all() and not np.isnan(sd[2:]).any() and len(sd) == 7       # m = 1 leaves no degree of freedom
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# Argument refusals by name
# ---------------------------------------------------------------------------------------------------------------------
def check_argument_refusals(lib, ptr):
    """the codes the header states, each before anything is enqueued (dummy non-null pointers do)"""
    nan = NAN

    def partition(**kw):
        a = dict(n=6, S=100, data=ptr, card=ptr, R=3, masks=ptr, pitch=64, count=ptr, cb=3 * 64 * 4, start=ptr, order=ptr, ob=3 * 100 * 4, status=ptr)
        a.update(kw)
        return lib.dvs_cg_partition(a["n"], a["S"], a["data"], a["card"], a["R"], a["masks"], a["pitch"], a["count"], a["cb"], a["start"],
                                    a["order"], a["ob"], a["status"], None)
    assert partition(R=0) == 2 and partition(S=0) == 2 and partition(n=0) == 3 and partition(n=49) == 3
    assert partition(pitch=0) == 13 and partition(pitch=MAXQ + 1) == 13 and partition(R=1 << 20, pitch=MAXQ) == 2
    for k in ("data", "card", "masks", "count", "start", "order", "status"):
        assert partition(**{k: None}) == 10, k
    assert partition(cb=767) == 14 and b"768" in lib.dvs_last_error()
    assert partition(ob=1199) == 14 and b"1200" in lib.dvs_last_error()

    ws = lambda **kw: lib.dvs_cg_moments_workspace_bytes(*[kw.get(k, d) for k, d in (("n", 5), ("S", 300), ("R", 2), ("pitch", 6))])
    assert ws() == 8 * 4 * 2 + 8 * 2 * 9 * 20 and ws(n=0) == 0 and ws(n=49) == 0 and ws(S=0) == 0 and ws(R=0) == 0 and ws(pitch=0) == 0
    assert ws(n=48, R=1 << 12, pitch=MAXQ) == 0 and b"2^31" in lib.dvs_last_error()

    def moments(**kw):
        a = dict(n=5, S=300, x=ptr, R=2, pitch=6, count=ptr, start=ptr, order=ptr, ws=ptr, wsb=1 << 20, mom=ptr, momb=2 * 6 * 31 * 8)
        a.update(kw)
        return lib.dvs_cg_moments(a["n"], a["S"], a["x"], a["R"], a["pitch"], a["count"], a["start"], a["order"], a["ws"], a["wsb"], a["mom"],
                                  a["momb"], None)
    assert moments(S=0) == 2 and moments(R=0) == 2 and moments(n=0) == 3 and moments(n=49) == 3 and moments(pitch=MAXQ + 1) == 13
    for k in ("x", "count", "start", "order", "ws", "mom"):
        assert moments(**{k: None}) == 10, k
    assert moments(wsb=2943) == 14 and b"2944" in lib.dvs_last_error()
    assert moments(momb=2975) == 14 and b"2976" in lib.dvs_last_error()

    def scores(**kw):
        a = dict(B=4, n=5, nc=2, S=100, data=ptr, card=ptr, tables=ptr, table_of=ptr, parents=ptr, typ=2, arg=nan, ws=ptr, wsb=4 * 5 * 8 + 64,
                 local=ptr, out=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_cg_scores(a["B"], a["n"], a["nc"], a["S"], a["data"], a["card"], a["tables"], a["table_of"], a["parents"], a["typ"],
                                 a["arg"], a["ws"], a["wsb"], a["local"], a["out"], a["status"], None)

    def toggle(**kw):
        a = dict(B=4, n=5, nc=2, S=100, data=ptr, card=ptr, tables=ptr, table_of=ptr, parents=ptr, typ=2, arg=nan, wl=None, ws=ptr,
                 wsb=4 * 5 * 8 + 64 + 32, L=ptr, Lb=4 * 5 * 8, T=ptr, Tb=4 * 25 * 8, status=ptr)
        a.update(kw)
        return lib.dvs_cg_toggle_scores(a["B"], a["n"], a["nc"], a["S"], a["data"], a["card"], a["tables"], a["table_of"], a["parents"],
                                        a["typ"], a["arg"], a["wl"], a["ws"], a["wsb"], a["L"], a["Lb"], a["T"], a["Tb"], a["status"], None)
    for fn in (scores, toggle):
        assert fn(B=0) == 2 and fn(S=0) == 2 and fn(n=0) == 3 and fn(n=49) == 3 and fn(nc=-1) == 3 and fn(nc=6) == 3
        assert fn(typ=-1) == 12 and fn(typ=3) == 12
        assert fn(typ=0, arg=1.0) == 13
        for typ in (1, 2):
            assert fn(typ=typ, arg=-1.0) == 13 and fn(typ=typ, arg=float("inf")) == 13
        for k in ("data", "card", "tables", "table_of", "parents", "ws", "status"):
            assert fn(**{k: None}) == 10, k
    assert scores(local=None) == 10 and scores(out=None) == 10
    assert scores(wsb=223) == 14 and b"224" in lib.dvs_last_error()
    assert toggle(B=1 << 20, n=48) == 2 and toggle(L=None) == 10 and toggle(T=None) == 10
    assert toggle(wsb=255) == 14 and b"256" in lib.dvs_last_error()
    assert toggle(Lb=159) == 14 and b"160" in lib.dvs_last_error()
    assert toggle(Tb=799) == 14 and b"800" in lib.dvs_last_error()
    assert lib.dvs_cg_scores_workspace_bytes(0, 5) == 0 and lib.dvs_cg_scores_workspace_bytes(4, 49) == 0
    assert lib.dvs_cg_toggle_workspace_bytes(1 << 20, 48) == 0

    def fit(**kw):
        a = dict(F=2, cells=7, n=6, nc=5, card=ptr, var=ptr, parents=ptr, table=ptr, offset=ptr, coef=ptr, cb=7 * 6 * 8, icpt=ptr, sd=ptr,
                 count=ptr, status=ptr)
        a.update(kw)
        return lib.dvs_cg_fit(a["F"], a["cells"], a["n"], a["nc"], a["card"], a["var"], a["parents"], a["table"], a["offset"], a["coef"],
                              a["cb"], a["icpt"], a["sd"], a["count"], a["status"], None)
    assert fit(F=0) == 2 and fit(cells=0) == 2 and fit(n=49) == 3 and fit(nc=0) == 3 and fit(nc=7) == 3 and fit(cells=1 << 27, n=48) == 2
    for k in ("card", "var", "parents", "table", "offset", "coef", "icpt", "sd", "count", "status"):
        assert fit(**{k: None}) == 10, k
    assert fit(cb=335) == 14 and b"336" in lib.dvs_last_error()
