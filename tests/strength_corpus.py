"""TEST HELPER: cases, references and the checks themselves for model averaging (csrc/dvs_strength.h: dvs_bn_scores_rows,
dvs_bn_toggle_scores_rows, dvs_bootstrap_rows, dvs_arc_strength, dvs_averaged_network; dags_vae_search_amd/strength.py),
written once and run by tests/test_emu_strength.py (emulator build) and tests/test_gpu_strength.py (device) through a back
end of tests/scoring_corpus.py.

References
  row sets        the library's own plain entry points on the host-gathered data set data[rows[set]]: the definition of
                  include/dvs.h.  Bytes are compared, NaN cells and status words included.
  bootstrap_ref   numpy on oracle/rng.py (site_key, draw): the formula of include/dvs.h.
  arc_ref         numpy bit tests, pair by pair.
  averaged_ref    Python ints: threshold, order, orientation and insertion as include/dvs.h states them, the ancestors by a
                  graph walk (the kernel keeps closure rows).  is_acyclic checks every output separately.
  l1_brute        the L1 estimator of Scutari and Nagarajan (2013) by exact minimisation in fractions.Fraction.
Everything is integers or equality of fp64 bytes: there are no tolerances.  The one statistical check (chi-square of the
restated draw, CPU only) has a fixed seed and a stated bound.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np

from oracle import rng as orng
from tests import bn_score_corpus as bn
from tests import scoring_corpus as sc
from tests.abi_cases import call, call_rc, entry, run

U64 = np.uint64
NAN = float("nan")
SITE_BOOTSTRAP = 600


class Driver:
    """the raw C ABI on a back end of scoring_corpus (numpy in place on the emulator, torch tensors on the device)"""

    def __init__(self, be):
        self.be, self.lib = be, be.lib

    def _scorer_args(self, packed, card, masks, typ, arg, rows, set_of):
        """(entry-point suffix, the named arguments every scorer call shares); the *_rows variants extend them by the row sets"""
        be = self.be
        B, n = masks.shape
        args = dict(batch=B, n_vars=n, n_samples=packed.shape[0], data=be.put(packed), card=be.put(card),
                    parents=be.put(np.ascontiguousarray(masks, U64)), score_type=bn.TYPE_CODE[typ],
                    score_arg=NAN if arg is None else float(arg), status=be.put(np.zeros(1, np.int32)))
        if rows is None:
            return "", args
        rows = np.ascontiguousarray(rows, np.int32)
        return "_rows", dict(args, rows=be.put(rows), set_size=rows.shape[1], n_sets=rows.shape[0],
                             set_of=None if set_of is None else be.put(np.ascontiguousarray(set_of, np.int32)))

    def scores(self, packed, card, masks, typ, arg=None, rows=None, set_of=None):
        """one dvs_bn_scores (rows None) or dvs_bn_scores_rows -> (scratch [B, n], out [B], status)"""
        be = self.be
        B, n = masks.shape
        suffix, args = self._scorer_args(packed, card, masks, typ, arg, rows, set_of)
        scratch, out = be.put(np.full((B, n), -7.0)), be.put(np.full(B, -7.0))
        call(be, "dvs_bn_scores" + suffix, **args, scratch=scratch, out=out)
        return be.get(scratch).copy(), be.get(out).copy(), int(be.get(args["status"])[0])

    def toggle(self, packed, card, masks, typ, arg=None, worklist=None, rows=None, set_of=None):
        """one dvs_bn_toggle_scores(_rows) into tables that start as -7 -> (L [B, n], T [B, n, n], status)"""
        be = self.be
        B, n = masks.shape
        suffix, args = self._scorer_args(packed, card, masks, typ, arg, rows, set_of)
        L, T = be.put(np.full((B, n), -7.0)), be.put(np.full((B, n, n), -7.0))
        wl = None if worklist is None else be.put(np.ascontiguousarray(worklist, np.int32))
        call(be, "dvs_bn_toggle_scores" + suffix, **args, worklist=wl, local=L, local_bytes=B * n * 8, toggles=T,
             toggles_bytes=B * n * n * 8)
        return be.get(L).copy(), be.get(T).copy(), int(be.get(args["status"])[0])

    def bootstrap(self, n_sets, set_size, n_samples, seed, set_offset=0):
        be = self.be
        rows = be.put(np.full((n_sets, set_size), -7, np.int32))
        call(be, "dvs_bootstrap_rows", n_sets=n_sets, set_size=set_size, n_samples=n_samples, seed=seed, set_offset=set_offset,
             rows=rows)
        return be.get(rows).copy()

    def arc_strength(self, P, counts=None):
        """one dvs_arc_strength accumulated into `counts` (zeros when None) -> i32 [n, n, 2]"""
        be = self.be
        P = np.ascontiguousarray(P, U64)
        B, n = P.shape
        hP = be.put(P)
        hc = be.put(np.zeros((n, n, 2), np.int32) if counts is None else np.ascontiguousarray(counts, np.int32))
        call(be, "dvs_arc_strength", batch=B, n_vars=n, pdag=hP, counts=hc, counts_bytes=n * n * 8)
        assert be.get(hP).tobytes() == P.tobytes()
        return be.get(hc).copy()

    def averaged(self, counts, n_networks, min_any):
        """one dvs_averaged_network over G groups -> (parents u64 [G, n], info i32 [G, 4]); the outputs start as garbage"""
        be = self.be
        counts = np.ascontiguousarray(counts, np.int32)
        G, n = counts.shape[:2]
        hc, hn, hm = be.put(counts), be.put(np.asarray(n_networks, np.int32)), be.put(np.asarray(min_any, np.int32))
        par, info = be.put(np.full((G, n), 0xA5A5A5A5A5A5A5A5, U64)), be.put(np.full((G, 4), -7, np.int32))
        call(be, "dvs_averaged_network", groups=G, n_vars=n, counts=hc, n_networks=hn, min_any=hm, parents=par,
             parents_bytes=G * n * 8, info=info)
        return be.get(par).copy(), be.get(info).copy()


def same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 1. Row sets in the scorer
# ---------------------------------------------------------------------------------------------------------------------
ROW_DATASETS = ("n12", "n20", "n48")
SET_SIZES = (1, 64, 97, 150)
SCORE_VARIANTS = (("loglik", None), ("aic", None), ("bic", None), ("bde", 10.0), ("bds", None), ("k2", None), ("bdj", None))


@functools.lru_cache(maxsize=None)
def row_dataset(name):
    """(data u8 [S, n], card, packed, structures u64 [B, n], expected status)"""
    if name == "n12":
        cards = [3] * 12
        cards[5] = 2
        data, card = sc.synthetic_dataset(12, 97, cards, seed=1201)
        chain = {v: [v - 1] for v in range(1, 12)}
        dense = {3: [0, 1, 2], 7: [4, 5, 6, 3], 11: [8, 9, 10], 2: [5]}
        sort = {4: [u for u in range(12) if u != 4]}                 # 11 parents, 3^10 * 2 * 3 cells: the sort path
        assert sc.cells_of(card, 4, sort[4]) > sc.MAX_BINS and sc.key_bits(card, 4, sort[4]) <= 63
        mixed = {4: [u for u in range(12) if u != 4], 0: [1], 9: [0, 5]}
        masks, status = sc.masks_of(12, {}, chain, dense, sort, mixed), 0
    elif name == "n20":
        rng = np.random.default_rng(2001)
        data, card = sc.synthetic_dataset(20, 97, rng.integers(2, 5, 20), seed=2002)
        assert set(int(c) for c in card) == {2, 3, 4}
        chain = {v: [v - 1] for v in range(1, 20)}
        dense = {17: [0, 16, 19], 3: [18, 1], 16: [15, 2, 3, 4], 19: [0]}       # parents and children in both data words
        many = {18: list(range(0, 13)) + [19], 1: [17]}
        assert sc.cells_of(card, 18, many[18]) > sc.MAX_BINS                 # the sort path across both words
        masks, status = sc.masks_of(20, {}, chain, dense, many, sc._random_dag(rng, 20)), 0
    else:
        data, card = sc.synthetic_dataset(48, 64, [4] * 48, seed=4801)
        chain = {v: [v - 1] for v in range(1, 48)}
        dense = {47: [0, 16, 32], 5: [46, 47], 20: [1, 2, 33, 40]}
        refused = {40: list(range(0, 32)), 3: [47]}                          # 32 four-level parents: 66 key bits
        assert sc.key_bits(card, 40, refused[40]) > 63
        masks, status = sc.masks_of(48, {}, chain, dense, refused, {9: list(range(10, 21))}), 16
    return data, card, sc.pack(data), masks, status


def row_sets(n_samples, set_size, seed):
    """i32 [5, set_size]: identity, reversed, one index repeated, two seeded sets with duplicates"""
    i = np.arange(set_size)
    rng = np.random.default_rng(seed)
    sets = [i % n_samples, (n_samples - 1 - i) % n_samples, np.full(set_size, (7 * set_size + 3) % n_samples),
            rng.integers(0, n_samples, set_size), rng.integers(0, max(1, n_samples // 3), set_size)]
    rows = np.stack(sets).astype(np.int32)
    assert set_size < 8 or all(len(np.unique(r)) < set_size for r in rows[2:])
    return rows


def set_of_variants(B, n_sets):
    """null (structure b on set b), permuted, with repeats; B <= n_sets"""
    assert B <= n_sets
    perm = np.array([(3 * b + 1) % n_sets for b in range(B)], np.int32)
    rep = np.array([(b // 2) * 2 % n_sets for b in range(B)], np.int32)
    assert len(set(perm.tolist())) == B and len(set(rep.tolist())) < B
    return (("null", None), ("permuted", perm), ("repeats", rep))


def _gathered(packed, rows, s):
    return np.ascontiguousarray(packed[rows[s]])


def check_scores_rows(drv, name, set_size, variants=SCORE_VARIANTS):
    """dvs_bn_scores_rows against dvs_bn_scores on the gathered rows, set by set: scratch, out and status, as bytes"""
    data, card, packed, masks, status = row_dataset(name)
    B, n = masks.shape
    rows = row_sets(len(data), set_size, seed=len(data) * 1000 + set_size)
    refused = 0
    for typ, arg in variants:
        ref = [drv.scores(_gathered(packed, rows, s), card, masks, typ, arg) for s in range(len(rows))]
        assert all(r[2] == status for r in ref), (name, typ, [r[2] for r in ref])
        for label, set_of in set_of_variants(B, len(rows)):
            scratch, out, st = drv.scores(packed, card, masks, typ, arg, rows=rows, set_of=set_of)
            which = np.arange(B) if set_of is None else set_of
            want_scratch = np.stack([ref[which[b]][0][b] for b in range(B)])
            want_out = np.array([ref[which[b]][1][b] for b in range(B)])
            assert st == status, (name, set_size, typ, label, st)
            assert same_bytes(scratch, want_scratch), (name, set_size, typ, label)
            assert same_bytes(out, want_out), (name, set_size, typ, label)
            refused += int(np.isnan(scratch).sum())
    if status:
        assert refused > 0
    return refused


def worklist_for(B, n):
    """i32 [2 B]: one row, two rows, an empty pair, (-1, row) and an out-of-range slot, cycled over the structures"""
    pats = [(1 % n, -1), (0, n - 1), (-1, -1), (-1, 2 % n), (n - 1, n)]
    return np.array([x for b in range(B) for x in pats[b % len(pats)]], np.int32)


def check_toggle_rows(drv, name, set_size, typ, arg, set_of_label, structures=None):
    """dvs_bn_toggle_scores_rows, full pass and worklist pass, against dvs_bn_toggle_scores on the gathered rows"""
    data, card, packed, masks, status = row_dataset(name)
    if structures is not None:
        masks = masks[list(structures)]
    B, n = masks.shape
    rows = row_sets(len(data), set_size, seed=len(data) * 1000 + set_size)
    set_of = dict(set_of_variants(B, len(rows)))[set_of_label]
    which = np.arange(B) if set_of is None else set_of
    for wl in (None, worklist_for(B, n)):
        ref = {s: drv.toggle(_gathered(packed, rows, s), card, masks, typ, arg, worklist=wl) for s in sorted(set(which.tolist()))}
        L, T, st = drv.toggle(packed, card, masks, typ, arg, worklist=wl, rows=rows, set_of=set_of)
        assert len({r[2] for r in ref.values()}) == 1 and st == next(iter(ref.values()))[2], (name, set_size, typ)
        assert same_bytes(L, np.stack([ref[which[b]][0][b] for b in range(B)])), (name, set_size, typ, wl is None)
        assert same_bytes(T, np.stack([ref[which[b]][1][b] for b in range(B)])), (name, set_size, typ, wl is None)
        if wl is None:
            assert not (T == -7.0).any() and not (L == -7.0).any()
        else:
            assert (L == -7.0).all() and (T == -7.0).any() and (T != -7.0).any()     # only the named rows are written


def check_identity_set(drv, name):
    """the identity set with set_size == n_samples is the plain call on the same data"""
    data, card, packed, masks, status = row_dataset(name)
    B, S = len(masks), len(data)
    rows = np.arange(S, dtype=np.int32)[None, :]
    zeros = np.zeros(B, np.int32)
    for typ, arg in (("bic", None), ("bde", 10.0)):
        a = drv.scores(packed, card, masks, typ, arg)
        b = drv.scores(packed, card, masks, typ, arg, rows=rows, set_of=zeros)
        assert a[2] == b[2] == status and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1]), (name, typ)
    a = drv.toggle(packed, card, masks[:2], "bic")
    b = drv.toggle(packed, card, masks[:2], "bic", rows=rows, set_of=zeros[:2])
    assert a[2] == b[2] and same_bytes(a[0], b[0]) and same_bytes(a[1], b[1]), name


def check_rows_refusals(drv):
    """code 13 for the row-set arguments, 14 for the sizes; nothing is written"""
    be, lib = drv.be, drv.lib
    data, card, packed, masks, _ = row_dataset("n12")
    B, n = masks.shape
    rows = row_sets(len(data), 64, seed=5)
    d, c, m, r = be.put(packed), be.put(card), be.put(masks), be.put(rows)
    scratch, out, status = be.put(np.full((B, n), -7.0)), be.put(np.full(B, -7.0)), be.put(np.zeros(1, np.int32))
    L, T = be.put(np.full((B, n), -7.0)), be.put(np.full((B, n, n), -7.0))
    BIC = bn.TYPE_CODE["bic"]

    head = dict(batch=B, n_vars=n, n_samples=len(data), data=d, card=c, parents=m, score_type=BIC, score_arg=NAN, status=status)

    def score(set_size=64, n_sets=5, set_of=None, rows=r):
        return call_rc(be, "dvs_bn_scores_rows", **head, scratch=scratch, out=out, rows=rows, set_size=set_size, n_sets=n_sets,
                       set_of=set_of)

    def toggle(set_size=64, n_sets=5, set_of=None, local_bytes=B * n * 8, toggles_bytes=B * n * n * 8):
        return call_rc(be, "dvs_bn_toggle_scores_rows", **head, worklist=None, local=L, local_bytes=local_bytes, toggles=T,
                       toggles_bytes=toggles_bytes, rows=r, set_size=set_size, n_sets=n_sets, set_of=set_of)
    for fn, name in ((score, "dvs_bn_scores_rows"), (toggle, "dvs_bn_toggle_scores_rows")):
        for kw, text in ((dict(set_size=0), "set_size and n_sets must be >= 1"), (dict(n_sets=0), "set_size and n_sets must be >= 1"),
                         (dict(n_sets=B - 1), "n_sets must be >= batch")):
            assert fn(**kw) == 13, (name, kw)
            msg = lib.dvs_last_error().decode()
            assert msg.startswith(name + ":") and text in msg, msg
    assert score(rows=None) == 10
    assert toggle(local_bytes=B * n * 8 - 1) == 14 and str(B * n * 8) in lib.dvs_last_error().decode()
    assert toggle(toggles_bytes=B * n * n * 8 - 1) == 14 and str(B * n * n * 8) in lib.dvs_last_error().decode()
    assert toggle(set_size=0, local_bytes=0) == 13                                   # the row-set check before the sizes
    for h in (scratch, out, L, T):
        assert (be.get(h) == -7.0).all()
    assert int(be.get(status)[0]) == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. dvs_bootstrap_rows
# ---------------------------------------------------------------------------------------------------------------------
BOOT_SET_SIZES = (1, 255, 256, 257, 1000)
BOOT_N_SAMPLES = (1, 2, 97, 100000)
BOOT_SEED = 0x9E3779B97F4A7C15                       # both halves of the seed are in play


def bootstrap_ref(n_sets, set_size, n_samples, seed, set_offset=0):
    g = (np.uint64(set_offset) + np.arange(n_sets, dtype=np.uint64)) & orng.M32
    key = orng.site_key(int(seed), SITE_BOOTSTRAP, g)[:, None]
    h = orng.draw(key, np.arange(set_size, dtype=np.uint64)[None, :])
    return ((h * np.uint64(n_samples)) >> np.uint64(32)).astype(np.int32)


def check_bootstrap_bytes(drv, set_size):
    for n_samples in BOOT_N_SAMPLES:
        got = drv.bootstrap(7, set_size, n_samples, BOOT_SEED)
        assert same_bytes(got, bootstrap_ref(7, set_size, n_samples, BOOT_SEED)), (set_size, n_samples)
        assert got.min() >= 0 and got.max() < n_samples


def check_bootstrap_offsets(drv):
    """7 sets in one call = 3 + 4 with set_offset; the global set index wraps at 2^32; the seed matters"""
    whole = drv.bootstrap(7, 257, 97, BOOT_SEED, 11)
    parts = np.concatenate([drv.bootstrap(3, 257, 97, BOOT_SEED, 11), drv.bootstrap(4, 257, 97, BOOT_SEED, 14)])
    assert same_bytes(whole, parts) and same_bytes(whole, bootstrap_ref(7, 257, 97, BOOT_SEED, 11))
    wrap = drv.bootstrap(4, 300, 97, BOOT_SEED, 2 ** 32 - 2)
    assert same_bytes(wrap, bootstrap_ref(4, 300, 97, BOOT_SEED, 2 ** 32 - 2))
    assert same_bytes(wrap[2:], drv.bootstrap(2, 300, 97, BOOT_SEED, 0))
    assert not same_bytes(drv.bootstrap(2, 300, 97, BOOT_SEED ^ (1 << 40), 0), wrap[2:])
    assert len({r.tobytes() for r in whole}) == 7


CHI2_SETS, CHI2_SIZE, CHI2_BINS = 40, 5000, 97
CHI2_BOUND = 177.1        # the 1 - 1e-6 quantile of chi-square with 96 degrees of freedom (scipy.stats.chi2.isf(1e-6, 96) = 177.06)


def check_restatement_is_uniform():
    """the restated draw alone: 200 000 indices into 97 bins.  The seed is fixed; a uniform generator exceeds the bound with
    probability 1e-6, a generator that misses one bin or favours one by 3 % lands far above it (expected statistic 96)."""
    rows = bootstrap_ref(CHI2_SETS, CHI2_SIZE, CHI2_BINS, seed=20131, set_offset=5)
    obs = np.bincount(rows.reshape(-1), minlength=CHI2_BINS).astype(np.float64)
    exp = rows.size / CHI2_BINS
    stat = float(((obs - exp) ** 2 / exp).sum())
    assert stat <= CHI2_BOUND, stat
    per_set = [np.bincount(r, minlength=CHI2_BINS) for r in rows]                  # and no two sets alike
    assert len({p.tobytes() for p in per_set}) == CHI2_SETS
    return stat


# ---------------------------------------------------------------------------------------------------------------------
# 3. dvs_arc_strength
# ---------------------------------------------------------------------------------------------------------------------
ARC_BATCHES = (1, 63, 64, 65, 257)
ARC_SIZES = (2, 17, 48)


def random_pdags(n, count, seed):
    """u64 [count, n]: every pair absent (half), u -> v, v -> u or undirected"""
    rng = np.random.default_rng(seed)
    state = np.array([0, 0, 0, 1, 2, 3])[rng.integers(0, 6, (count, n, n))]
    out = np.zeros((count, n), U64)
    for u, v in itertools.combinations(range(n), 2):
        s = state[:, u, v]
        out[:, v] |= (s & 1).astype(U64) << U64(u)
        out[:, u] |= ((s >> 1) & 1).astype(U64) << U64(v)
    return out


def arc_ref(P, n):
    P = np.asarray(P, U64)
    bit = ((P[:, :, None] >> np.arange(n, dtype=U64)[None, None, :]) & U64(1)).astype(bool)     # [b, v, u]: u in row v
    into, back = bit.transpose(0, 2, 1), bit                                                 # [b, u, v]: u -> v / - ; v -> u / -
    off = ~np.eye(n, dtype=bool)[None]
    counts = np.zeros((n, n, 2), np.int32)
    counts[..., 0] = ((into | back) & off).sum(0)
    counts[..., 1] = (2 * (into & ~back & off) + (into & back & off)).sum(0)
    return counts


def check_arc_identities(counts):
    """adjacency is symmetric, the two direction counts of a pair sum to twice its adjacency count, the diagonal is zero"""
    any_, dir2 = counts[..., 0].astype(np.int64), counts[..., 1].astype(np.int64)
    assert np.array_equal(any_, any_.T) and np.array_equal(dir2 + dir2.T, 2 * any_)
    assert not np.diagonal(any_).any() and not np.diagonal(dir2).any()


def check_arc_random(drv, n):
    for B in ARC_BATCHES:
        P = random_pdags(n, B, seed=7000 + 100 * n + B)
        want = arc_ref(P, n)
        got = drv.arc_strength(P)
        assert same_bytes(got, want), (n, B)
        check_arc_identities(got)
        if B >= 63:
            assert got[n - 1, 0, 0] > 0 and got[0, n - 1, 1] + got[n - 1, 0, 1] > 0       # the top bit of a row is counted
    # stray diagonal and high bits change nothing
    P = random_pdags(n, 65, seed=7100 + n)
    Q = P.copy()
    for v in range(n):
        Q[::2, v] |= U64(1) << U64(v)
    Q[:, 0] |= U64(0xFFFF) << U64(48)
    Q[:, n - 1] |= ~U64(0) << U64(n)
    assert same_bytes(drv.arc_strength(Q), arc_ref(P, n))
    # accumulation: two calls into one table are one call over both batches; a second run gives equal bytes
    A, B2 = random_pdags(n, 65, seed=7200 + n), random_pdags(n, 130, seed=7300 + n)
    both = drv.arc_strength(np.concatenate([A, B2]))
    assert same_bytes(drv.arc_strength(B2, counts=drv.arc_strength(A)), both)
    assert same_bytes(drv.arc_strength(np.concatenate([A, B2])), both)


def check_arc_extremes(drv):
    for n in (2, 48):
        for B in (1, 65):
            assert not drv.arc_strength(np.zeros((B, n), U64)).any()
            full = (1 << n) - 1
            und = np.array([[full & ~(1 << v) for v in range(n)]] * B, U64)          # every pair undirected
            got = drv.arc_strength(und)
            off = ~np.eye(n, dtype=bool)
            assert (got[..., 0][off] == B).all() and (got[..., 1][off] == B).all() and same_bytes(got, arc_ref(und, n))
            order = np.array([[(1 << v) - 1 for v in range(n)]] * B, U64)            # the complete order: u -> v for u < v
            got = drv.arc_strength(order)
            assert same_bytes(got, arc_ref(order, n))
            assert (got[..., 1][np.triu(off)] == 2 * B).all() and not got[..., 1][np.tril(off)].any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dvs_averaged_network
# ---------------------------------------------------------------------------------------------------------------------
def pairs_of(n):
    return list(itertools.combinations(range(n), 2))


def threshold_ref(A_values, R):
    """T of include/dvs.h: the largest A with 2 A <= R, else the smallest A (0 without pairs)"""
    A_values = [int(a) for a in A_values]
    if not A_values:
        return 0
    below = [a for a in A_values if 2 * a <= R]
    return max(below) if below else min(A_values)


def _ancestors(parents, v):
    seen, stack = 0, [v]
    while stack:
        for u in sc.mask_bits(parents[stack.pop()]):
            if not (seen >> u) & 1:
                seen |= 1 << u
                stack.append(u)
    return seen


def is_acyclic(parents):
    return all(not (_ancestors(parents, v) >> v) & 1 for v in range(len(parents)))


def averaged_ref(counts, R, min_any):
    """(parents as ints, (min_any used, placed, dropped, ties)) for one group"""
    counts = np.asarray(counts)
    n = counts.shape[0]
    rec = [(int(counts[u, v, 0]), int(counts[u, v, 1]), int(counts[v, u, 1]), u, v) for u, v in pairs_of(n)]
    if min_any < 0:
        min_any = threshold_ref([r[0] for r in rec], R) + 1
    sig = sorted((r for r in rec if r[0] >= min_any), key=lambda r: (-r[0], -abs(r[1] - r[2]), r[3] * n + r[4]))
    parents = [0] * n
    placed = dropped = ties = 0
    for A, D, Dr, u, v in sig:
        tries = [(u, v)] if D > Dr else [(v, u)] if D < Dr else [(u, v), (v, u)]
        ties += D == Dr
        for t, h in tries:
            if not (_ancestors(parents, t) >> h) & 1 and t != h:
                parents[h] |= 1 << t
                placed += 1
                break
        else:
            dropped += 1
    return parents, (min_any, placed, dropped, ties)


def random_counts(n, R, seed, tie_share=0.3):
    """i32 [n, n, 2] as dvs_arc_strength leaves it for R networks: A symmetric in 0 .. R, D + D' = 2 A, many exact ties and
    equal A's (so every key of the order decides somewhere)"""
    rng = np.random.default_rng(seed)
    c = np.zeros((n, n, 2), np.int32)
    for u, v in pairs_of(n):
        A = int(rng.choice([0, int(rng.integers(0, R + 1)), int(rng.integers(R // 2, R + 1)), R // 2, R // 2 + 1]))
        D = A if rng.random() < tie_share else int(rng.integers(0, 2 * A + 1))
        c[u, v] = (A, D)
        c[v, u] = (A, 2 * A - D)
    return c


def check_averaged_groups(drv, counts_list, R_list, min_any_list):
    """one launch over the groups against averaged_ref, group by group; every output acyclic"""
    par, info = drv.averaged(np.stack(counts_list), R_list, min_any_list)
    out = []
    for g, (c, R, m) in enumerate(zip(counts_list, R_list, min_any_list)):
        want_p, want_i = averaged_ref(c, R, m)
        got_p = [int(x) for x in par[g]]
        assert is_acyclic(got_p), (g, got_p)
        assert got_p == want_p and tuple(int(x) for x in info[g]) == want_i, (g, R, m, got_p, want_p, info[g].tolist(), want_i)
        assert want_i[1] == sum(bin(x).count("1") for x in want_p)
        out.append(want_i)
    return out


def check_averaged_random(drv, n):
    R = 50
    mats = [random_counts(n, R, seed=8000 + 10 * n + k) for k in range(4)]
    mins = [-1, 0, 1, R // 2, R // 2 + 1, R, R + 1, -3]
    counts_list = [m for m in mats for _ in mins]
    infos = check_averaged_groups(drv, counts_list, [R] * len(counts_list), mins * len(mats))
    if n >= 8:
        assert any(i[2] > 0 for i in infos) and any(i[3] > 0 for i in infos)           # cycles dropped, ties met
    assert all(i[1] == 0 for i, m in zip(infos, mins * len(mats)) if m == R + 1)       # above every count: empty
    return infos


def _counts_from(n, R, arcs):
    """arcs: {(u, v): (A, D)} with D the doubled direction count of u -> v"""
    c = np.zeros((n, n, 2), np.int32)
    for (u, v), (A, D) in arcs.items():
        c[u, v] = (A, D)
        c[v, u] = (A, 2 * A - D)
    return c


def check_averaged_hand(drv):
    R = 10
    one = lambda c, m, R=R: (drv.averaged(c[None], [R], [m]), averaged_ref(c, R, m))

    def expect(c, m, parents, info, R=R):
        (par, inf), (rp, ri) = one(c, m, R)
        assert [int(x) for x in par[0]] == rp == parents, (par[0].tolist(), rp, parents)
        assert tuple(int(x) for x in inf[0]) == ri == info, (inf[0].tolist(), ri, info)
    # a majority 3-cycle 0 -> 1 -> 2 -> 0: the weakest arc (2 -> 0, A = 7) is dropped
    cyc = _counts_from(3, R, {(0, 1): (9, 18), (1, 2): (8, 16), (0, 2): (7, 0)})
    expect(cyc, 1, [0, 1 << 0, 1 << 1], (1, 2, 1, 0))
    # exact ties: u -> v first
    tie = _counts_from(3, R, {(0, 1): (9, 9), (1, 2): (8, 8)})
    expect(tie, 1, [0, 1 << 0, 1 << 1], (1, 2, 0, 2))
    # a tie whose first orientation closes a cycle: 1 -> 2, 2 -> 0 placed, then 0 - 1 tied: 0 -> 1 would close, so 1 -> 0
    tie2 = _counts_from(3, R, {(1, 2): (9, 18), (0, 2): (8, 0), (0, 1): (7, 7)})
    expect(tie2, 1, [(1 << 2) | (1 << 1), 0, 1 << 1], (1, 3, 0, 1))
    # min_any above every count: the empty graph
    expect(cyc, 10, [0, 0, 0], (10, 0, 0, 0))
    # min_any <= 0: every pair with A >= min_any is taken, the absent ones as ties
    sparse = _counts_from(3, R, {(1, 2): (4, 0)})
    expect(sparse, 0, [0, (1 << 0) | (1 << 2), 1 << 0], (0, 3, 0, 2))
    # min_any < 0 with a pair at 2 A <= R: T = 5 (2 * 5 <= 10), the pairs above it stay
    est = _counts_from(4, R, {(0, 1): (9, 18), (1, 2): (5, 10), (2, 3): (6, 12), (0, 3): (2, 4)})
    expect(est, -1, [0, 1 << 0, 0, 1 << 2], (6, 2, 0, 0))
    # ... and without one: every pair is above R / 2, T is the smallest A, which is then left out itself
    full = _counts_from(3, R, {(0, 1): (9, 18), (1, 2): (8, 16), (0, 2): (7, 14)})
    expect(full, -1, [0, 1 << 0, 1 << 1], (8, 2, 0, 0))
    expect(full, -7, [0, 1 << 0, 1 << 1], (8, 2, 0, 0))                             # any negative value asks for the estimate
    # one variable: no pairs
    (par, inf), _ = one(np.zeros((1, 1, 2), np.int32), -1)
    assert int(par[0, 0]) == 0 and inf[0].tolist() == [1, 0, 0, 0]


def check_averaged_sweep(drv, n=8):
    """a 16-group sweep over one matrix equals 16 single calls"""
    R = 40
    c = random_counts(n, R, seed=8800 + n)
    mins = [-1] + list(range(0, R + 5, 3))[:15]
    assert len(mins) == 16
    par, info = drv.averaged(np.stack([c] * 16), [R] * 16, mins)
    for g, m in enumerate(mins):
        p1, i1 = drv.averaged(c[None], [R], [m])
        assert same_bytes(p1[0], par[g]) and same_bytes(i1[0], info[g]), (g, m)
    placed = info[1:, 1]
    assert (np.diff(info[1:, 0]) > 0).all() and placed[0] > placed[-1] == 0                 # fewer arcs as the threshold rises
    par2, info2 = drv.averaged(np.stack([c] * 16), [R] * 16, mins)
    assert same_bytes(par, par2) and same_bytes(info, info2)


# ---- the closed-form threshold against exact minimisation of the L1 norm -------------------------------------------------
def l1_brute(A_values, R):
    """The estimator of Scutari and Nagarajan (2013) by brute force in exact rationals -> T (a count).  F is the empirical CDF
    of the strengths x = A / R on [0, 1]; for a level t, L1(t) = integral over [0, 1] of |F(x) - t|.  Every level k / P is
    tried (L1 is piecewise linear and convex in t with its kinks there, so a minimiser is among them); of the minimisers the
    largest is kept (they differ only when 1/2 is itself an observed strength: the closed form then takes 1/2).  The
    threshold is the type-1 quantile of that level, inf {x observed : F(x) >= t}."""
    xs = sorted(Fraction(int(a), R) for a in A_values)
    P = len(xs)
    F = lambda x: Fraction(sum(1 for y in xs if y <= x), P)
    knots = sorted({Fraction(0), Fraction(1)} | {x for x in xs if 0 <= x <= 1})
    pieces = [(b - a, F(a)) for a, b in zip(knots, knots[1:])]                     # F is constant on [a, b)
    l1 = lambda t: sum(w * abs(f - t) for w, f in pieces)
    levels = [Fraction(k, P) for k in range(P + 1)]
    best = min(l1(t) for t in levels)
    t_star = max(t for t in levels if l1(t) == best)
    return int(min(x for x in xs if F(x) >= t_star) * R)


def check_closed_form_threshold(count=1000):
    """threshold_ref == l1_brute on seeded count sets: few and many pairs, strengths on, around and away from 1/2, even and
    odd R, sets with no strength at or below 1/2"""
    rng = np.random.default_rng(4242)
    kinds = {"mixed": 0, "all_high": 0, "half_present": 0}
    for k in range(count):
        R = int(rng.integers(1, 41))
        P = int(rng.choice([1, 3, 6, 10, 28]))
        mode = k % 4
        if mode == 0:
            A = rng.integers(R // 2 + 1, R + 1, P)                                   # nothing at or below 1/2
        elif mode == 1:
            A = rng.choice([0, R // 2, (R + 1) // 2, R], P)
        else:
            A = rng.integers(0, R + 1, P)
        A = [int(a) for a in A]
        kinds["all_high"] += all(2 * a > R for a in A)
        kinds["half_present"] += any(2 * a == R for a in A)
        kinds["mixed"] += any(2 * a > R for a in A) and any(2 * a <= R for a in A)
        assert threshold_ref(A, R) == l1_brute(A, R), (A, R, threshold_ref(A, R), l1_brute(A, R))
    assert min(kinds.values()) >= count // 20, kinds
    return kinds


# ---------------------------------------------------------------------------------------------------------------------
# 5. Argument refusals of the three new calls (checked before anything is enqueued: dummy pointers do)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []

    c = entry("dvs_bootstrap_rows", cases, n_sets=8, set_size=100, n_samples=97, seed=7, set_offset=0, rows=D, stream=None)
    c(2, "n_sets must be > 0", n_sets=0)
    c(13, "set_size and n_samples must be >= 1", set_size=0)
    c(13, "set_size and n_samples must be >= 1", n_samples=0)
    c(2, "n_sets * set_size must be < 2^31", n_sets=1 << 16, set_size=1 << 15)
    c(12, "set_offset must be >= 0", set_offset=-1)
    c(10, "null pointer", rows=None)
    c(2, "n_sets must be > 0", n_sets=0, set_size=0)                                   # n_sets before set_size
    c(13, "set_size and n_samples", n_samples=0, rows=None)                            # sizes before null

    c = entry("dvs_arc_strength", cases, batch=8, n_vars=12, pdag=D, counts=D, counts_bytes=1152, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(10, "null pointer", pdag=None)
    c(10, "null pointer", counts=None)
    c(14, "counts_bytes < n_vars^2 * 8 = 1152", counts_bytes=1151)
    c(10, "null pointer", counts=None, counts_bytes=0)                                 # null before counts_bytes

    c = entry("dvs_averaged_network", cases, groups=4, n_vars=12, counts=D, n_networks=D, min_any=D, parents=D,
              parents_bytes=384, info=D, stream=None)
    c(2, "groups must be > 0", groups=0)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(2, "groups * n_vars^2 * 2 must be < 2^31", groups=1 << 20, n_vars=48, parents_bytes=1 << 40)
    for name in ("counts", "n_networks", "min_any", "parents", "info"):
        c(10, "null pointer", **{name: None})
    c(14, "parents_bytes < groups * n_vars * 8 = 384", parents_bytes=383)
    c(3, "n_vars must be in [1, 48]", n_vars=49, counts=None)                          # range before null
    c(10, "null pointer", info=None, parents_bytes=0)                                  # null before parents_bytes
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_bootstrap_rows", "dvs_arc_strength", "dvs_averaged_network"}
    run(lib, cases)


def toggle_plan():
    """(data set, set size, score variant, set_of variant, structures or None): every data set at every set size, the seven
    score types and the three set_of forms in rotation; n = 48 takes two structures (a full pass is B n^2 workgroups)"""
    plan = []
    labels = ("null", "permuted", "repeats")
    for k, (name, size) in enumerate(itertools.product(ROW_DATASETS, SET_SIZES)):
        typ, arg = SCORE_VARIANTS[k % len(SCORE_VARIANTS)]
        plan.append((name, size, typ, arg, labels[k % 3], (1, 3) if name == "n48" else None))
    assert {p[2] for p in plan} == {t for t, _ in SCORE_VARIANTS}
    return plan
