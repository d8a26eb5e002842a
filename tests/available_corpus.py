"""TEST HELPER: cases, references and the checks themselves for available-case scoring on incomplete data
(csrc/dvs_available.h: dvs_bn_scores_avail, dvs_bn_toggle_scores_avail; include/dvs_available.h), written once and run by
tests/test_emu_available.py (emulator build) and tests/test_gpu_available.py (device) through a back end of
tests/scoring_corpus.py; tests/test_available_ref.py pins the restatement against truth on the CPU.

References
  bytes           the library's own dvs_bn_scores (loglik) on the host-gathered rows that count for a family gives LL; the local
                  score is then LL / m - (k (r - 1)) q in numpy float64, compared as bytes.  Families are grouped by identical
                  row sets, so a data set needs tens of reference calls.
  toggles         dvs_bn_scores_avail on the structure with the bit flipped, as bytes.
  restatement     numpy: a masked bincount and the formula.  Against 60-digit mpmath (bn_score_corpus.MP) on the gathered rows,
                  LL divided by m in mpmath minus the penalty, within bn_score_corpus.RTOL = 1e-12 (the project's convention)
                  of |LL| / m + penalty; the kernels are held to the restatement within the same bound.

Data: strength_corpus.row_dataset n12 (a 12-variable sort-path family), n20 (parents in both data words, a sort-path family
across them), n48 (three words, a refused 66-key-bit family).  Masks per data set: `all`, `light` (about 5 % missing), `heavy`
(about 30 % missing).  What `heavy` forces, by construction:
  row 1 observes nothing; row 3 observes variable 0 alone; row 2 also has every bit at and above n set;
  PAIR (a, b) is never observed together: a is cleared in rows 0, 1 mod 4 and b in rows 2, 3 mod 4 — in rows 0 and 2 as well, so
  "wholly observed" there means every variable but the one of the pair that the row clears (the two conditions cannot both hold
  to the letter: a row that observes everything observes the pair);
  LONE is observed in rows 0 and 2 only, so {LONE, a} counts row 2 alone and {LONE, b} row 0 alone: m = 1.
The corpus asserts its own conditions (check_conditions); they are conditions of the cases, not measurements."""
import functools
from collections import Counter

import numpy as np

from tests import bn_score_corpus as bn
from tests import scoring_corpus as sc
from tests.abi_cases import at, run
from tests.eliminate_corpus import call, call_rc, entry
from tests.strength_corpus import Driver, row_dataset, same_bytes, worklist_for

U64 = np.uint64
DATASETS = ("n12", "n20", "n48")
MASK_SETS = ("all", "light", "heavy")
KS = (0.0, 0.3, 97 ** -0.25)
TOGGLE_STRUCTURES = (0, 1, 2)                     # empty, chain, dense of every row_dataset
TOGGLE_K = 0.3
GUARD = sc.GUARD
# (LONE, a, b) per data set, chosen against its structures: the chain has {LONE, a} (m = 1), a scored family holds a and b (m = 0)
SPECIAL = {"n12": (11, 10, 9), "n20": (19, 0, 18), "n48": (47, 46, 5)}
SEEDS = {("n12", "light"): 1205, ("n12", "heavy"): 1230, ("n20", "light"): 2005, ("n20", "heavy"): 2030,
         ("n48", "light"): 4805, ("n48", "heavy"): 4830}


def observed_bits(seen):
    """bool [S, n] -> u64 [S]"""
    out = np.zeros(seen.shape[0], U64)
    for v in range(seen.shape[1]):
        out |= seen[:, v].astype(U64) << U64(v)
    return out


@functools.lru_cache(maxsize=None)
def mask_set(name, kind):
    """u64 [S]: the observed words of one mask set of one data set"""
    data = row_dataset(name)[0]
    S, n = data.shape
    if kind == "all":
        return np.full(S, (1 << n) - 1, U64)
    rng = np.random.default_rng(SEEDS[name, kind])
    seen = rng.random((S, n)) >= (0.05 if kind == "light" else 0.30)
    if kind == "light":
        return observed_bits(seen)
    lone, a, b = SPECIAL[name]
    seen[0] = seen[2] = True
    seen[1] = False
    seen[3] = False
    seen[3, 0] = True
    seen[:, lone] = False
    seen[[0, 2], lone] = True
    rows = np.arange(S)
    seen[rows % 4 < 2, a] = False
    seen[rows % 4 >= 2, b] = False
    obs = observed_bits(seen)
    obs[2] |= ~U64(0) << U64(n)                    # bits at and above n: ignored
    return obs


def family_mask(masks, b, v):
    return (int(masks[b, v]) & ~(1 << v)) | (1 << v)


def counted(obs, fam):
    """bool [S]: the rows that count for the family mask"""
    return (obs & U64(fam)) == U64(fam)


def is_refused(name, card, masks, b, v):
    ps = [u for u in sc.mask_bits(masks[b, v]) if u != v]
    S = len(row_dataset(name)[0])
    return any(u >= len(card) for u in ps) or (sc.cells_of(card, v, ps) > sc.MAX_BINS and (sc.key_bits(card, v, ps) > 63 or S > sc.MAX_SORT))


def is_sort_path(card, masks, b, v):
    ps = [u for u in sc.mask_bits(masks[b, v]) if u != v]
    return sc.cells_of(card, v, ps) > sc.MAX_BINS


def flipped(masks, b, u):
    """the structure b with bit u flipped in every row but u's own: local[v] of it is T[b, v, u]"""
    out = masks[b].copy()
    for v in range(len(out)):
        if v != u:
            out[v] ^= U64(1) << U64(u)
    return out


def check_conditions():
    """what the cases must be for the checks to mean something; returns the m = 0 / m = 1 counts per data set"""
    found = {}
    for name in DATASETS:
        data, card, packed, masks, status = row_dataset(name)
        S, n = data.shape
        B = len(masks)
        for kind in MASK_SETS:
            obs = mask_set(name, kind)
            seen_any = int(np.bitwise_or.reduce(obs))
            assert all((seen_any >> v) & 1 for v in range(n)), (name, kind)             # every variable is observed somewhere
        light, heavy = mask_set(name, "light"), mask_set(name, "heavy")
        missing = lambda obs: 1.0 - sum(bin(int(x) & ((1 << n) - 1)).count("1") for x in obs) / (S * n)
        assert 0.02 < missing(light) < 0.08 and 0.25 < missing(heavy) < 0.45, (name, missing(light), missing(heavy))
        sort_m = [int(counted(light, family_mask(masks, b, v)).sum()) for b in range(B) for v in range(n)
                  if is_sort_path(card, masks, b, v) and not is_refused(name, card, masks, b, v)]
        assert (name == "n48" or sort_m) and all(m >= 16 for m in sort_m), (name, sort_m)
        lone, a, b_ = SPECIAL[name]
        assert int(heavy[0]) == ((1 << n) - 1) & ~(1 << a) and int(heavy[1]) == 0 and int(heavy[3]) == 1
        assert int(heavy[2]) & ((1 << n) - 1) == ((1 << n) - 1) & ~(1 << b_) and int(heavy[2]) >> n == (1 << (64 - n)) - 1
        assert not counted(heavy, (1 << a) | (1 << b_)).any()                           # never observed together
        scored = Counter(int(counted(heavy, family_mask(masks, b, v)).sum()) for b in range(B) for v in range(n)
                         if not is_refused(name, card, masks, b, v))
        toggled = Counter()
        for b in TOGGLE_STRUCTURES:
            for u in range(n):
                fl = flipped(masks, b, u)[None, :]
                toggled.update(int(counted(heavy, family_mask(fl, 0, v)).sum()) for v in range(n) if v != u)
        assert scored[0] >= 1 and toggled[0] >= 1 and scored[1] >= 1 and toggled[1] >= 1, (name, scored, toggled)
        found[name] = (scored[0], scored[1], toggled[0], toggled[1])
    return found


class AvailDriver(Driver):
    """the two *_avail entry points on a back end; every output sits between two guards of GUARD sentinel elements"""

    def _guarded(self, shape, fill, dtype):
        size = int(np.prod(shape))
        return self.be.put(np.full(size + 2 * GUARD, fill, dtype))

    def _inner(self, h, shape, fill):
        whole = self.be.get(h)
        size = int(np.prod(shape))
        assert (whole[:GUARD] == fill).all() and (whole[GUARD + size:] == fill).all(), "a write outside the output"
        return whole[GUARD:GUARD + size].reshape(shape).copy()

    def _head(self, packed, observed, card, masks, k):
        be = self.be
        B, n = masks.shape
        return dict(batch=B, n_vars=n, n_samples=packed.shape[0], data=be.put(packed), observed=be.put(np.ascontiguousarray(observed, U64)),
                    card=be.put(card), parents=be.put(np.ascontiguousarray(masks, U64)), k=float(k), status=be.put(np.zeros(1, np.int32)))

    def scores_avail(self, packed, observed, card, masks, k, with_used=True):
        """one dvs_bn_scores_avail -> (local [B, n], out [B], used [B, n] or None, status)"""
        be = self.be
        B, n = masks.shape
        args = self._head(packed, observed, card, masks, k)
        local, out = self._guarded((B, n), -7.0, np.float64), self._guarded((B,), -7.0, np.float64)
        used = self._guarded((B, n), -7, np.int32) if with_used else None
        call(be, "dvs_bn_scores_avail", **args, local=at(be, local, GUARD * 8), out=at(be, out, GUARD * 8),
             used=None if used is None else at(be, used, GUARD * 4))
        return (self._inner(local, (B, n), -7.0), self._inner(out, (B,), -7.0),
                None if used is None else self._inner(used, (B, n), -7), int(be.get(args["status"])[0]))

    def toggle_avail(self, packed, observed, card, masks, k, worklist=None):
        """one dvs_bn_toggle_scores_avail into tables that start as -7 -> (L [B, n], T [B, n, n], status)"""
        be = self.be
        B, n = masks.shape
        args = self._head(packed, observed, card, masks, k)
        L, T = self._guarded((B, n), -7.0, np.float64), self._guarded((B, n, n), -7.0, np.float64)
        wl = None if worklist is None else be.put(np.ascontiguousarray(worklist, np.int32))
        call(be, "dvs_bn_toggle_scores_avail", **args, worklist=wl, local=at(be, L, GUARD * 8), local_bytes=B * n * 8,
             toggles=at(be, T, GUARD * 8), toggles_bytes=B * n * n * 8)
        return self._inner(L, (B, n), -7.0), self._inner(T, (B, n, n), -7.0), int(be.get(args["status"])[0])


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2. Scores as bytes
# ---------------------------------------------------------------------------------------------------------------------
def formula(LL, m, k, r, q):
    """the local score in numpy float64: one division, the two products in that order, one subtraction"""
    return np.float64(LL) / np.float64(m) - (np.float64(k) * np.float64(r - 1)) * np.float64(q)


_ll_cache = {}


def gathered_loglik(drv, name, kind):
    """{(b, v): (LL, m)} for every family of the data set's structures that is not refused and has m >= 1: LL is local[v] of the
    plain dvs_bn_scores (loglik) on the rows that count; families with identical row sets share one call"""
    key = (id(drv), name, kind)
    if key in _ll_cache:
        return _ll_cache[key]
    data, card, packed, masks, status = row_dataset(name)
    B, n = masks.shape
    obs = mask_set(name, kind)
    groups = {}
    for b in range(B):
        for v in range(n):
            if is_refused(name, card, masks, b, v):
                continue
            rows = counted(obs, family_mask(masks, b, v))
            if rows.any():
                groups.setdefault(rows.tobytes(), (rows, []))[1].append((b, v))
    out = {}
    for rows, fams in groups.values():
        single = np.zeros((len(fams), n), U64)                # one structure per family: that family and nothing else
        for i, (b, v) in enumerate(fams):
            single[i, v] = masks[b, v]
        scratch, _, st = drv.scores(np.ascontiguousarray(packed[rows]), card, single, "loglik")
        assert st == 0, (name, kind, st)
        for i, (b, v) in enumerate(fams):
            out[b, v] = (scratch[i, v], int(rows.sum()))
    _ll_cache[key] = out
    return out


def expected_scores(drv, name, kind, k):
    """(local [B, n], out [B], used [B, n], status) as the definition gives them"""
    data, card, packed, masks, status = row_dataset(name)
    B, n = masks.shape
    obs = mask_set(name, kind)
    ref = gathered_loglik(drv, name, kind)
    local, used, st = np.zeros((B, n)), np.zeros((B, n), np.int32), 0
    for b in range(B):
        for v in range(n):
            if is_refused(name, card, masks, b, v):
                local[b, v], st = np.nan, st | 16
            elif (b, v) not in ref:
                local[b, v], st = -np.inf, st | 128
            else:
                LL, m = ref[b, v]
                q = np.prod([float(card[u]) for u in sc.mask_bits(masks[b, v]) if u != v])
                local[b, v], used[b, v] = formula(LL, m, k, int(card[v]), q), m
    out = np.zeros(B)
    for v in range(n):                                        # left to right from +0, as k_bic_sum adds
        out = out + local[:, v]
    return local, out, used, st


def check_scores(drv, name, kind):
    """dvs_bn_scores_avail against the definition over the plain scorer on gathered rows: local, out, used, status as bytes,
    for every k; sentinel guards around the outputs (AvailDriver); two runs give equal bytes; used may be null"""
    data, card, packed, masks, status = row_dataset(name)
    obs = mask_set(name, kind)
    seen = Counter()
    for k in KS:
        want = expected_scores(drv, name, kind, k)
        got = drv.scores_avail(packed, obs, card, masks, k)
        assert got[3] == want[3] and (got[3] & 16) == status, (name, kind, k, got[3], want[3])
        assert same_bytes(got[2], want[2]), (name, kind, k, np.argwhere(got[2] != want[2])[:5])
        assert same_bytes(got[0], want[0]), (name, kind, k, np.argwhere(got[0].view(U64) != want[0].view(U64))[:5])
        nan = np.isnan(want[1])                                # a refused family: the total is a NaN, whichever
        assert np.array_equal(nan, np.isnan(got[1])) and same_bytes(got[1][~nan], want[1][~nan]), (name, kind, k)
        seen.update(["nan"] * int(np.isnan(got[0]).sum()) + ["-inf"] * int(np.isneginf(got[0]).sum()))
    again = drv.scores_avail(packed, obs, card, masks, KS[1])
    assert same_bytes(again[0], expected_scores(drv, name, kind, KS[1])[0])
    no_used = drv.scores_avail(packed, obs, card, masks, KS[1], with_used=False)
    assert no_used[2] is None and same_bytes(no_used[0], again[0]) and same_bytes(no_used[1], again[1])
    if kind == "heavy":
        assert seen["-inf"] > 0, (name, seen)
    if status:
        assert seen["nan"] > 0
    return seen


def check_everything_observed(drv, name):
    """with every bit set and k = 0 the score is LL / S of the plain scorer (not local * S back: a different rounding), and every
    family that is not refused uses all S rows"""
    data, card, packed, masks, status = row_dataset(name)
    S = len(data)
    B, n = masks.shape
    plain, _, st = drv.scores(packed, card, masks, "loglik")
    local, out, used, st2 = drv.scores_avail(packed, mask_set(name, "all"), card, masks, 0.0)
    assert st == st2 == status
    ok = ~np.isnan(plain)
    assert np.array_equal(ok, ~np.isnan(local)) and (used[ok] == S).all() and (used[~ok] == 0).all()
    assert same_bytes(local[ok], plain[ok] / np.float64(S) - 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. Toggles
# ---------------------------------------------------------------------------------------------------------------------
def check_toggles(drv, name, kind):
    """a full pass and the worklist_for pass on {empty, chain, dense}: L is local of dvs_bn_scores_avail, T[b, v, u] is local[v]
    of dvs_bn_scores_avail on the structure with that bit flipped, as bytes; NaN on the diagonal; the worklist pass writes the
    named rows only"""
    data, card, packed, masks, status = row_dataset(name)
    masks = np.ascontiguousarray(masks[list(TOGGLE_STRUCTURES)])
    B, n = masks.shape
    obs = mask_set(name, kind)
    want_L = drv.scores_avail(packed, obs, card, masks, TOGGLE_K)[0]
    flips = np.stack([flipped(masks, b, u) for b in range(B) for u in range(n)])
    ref = drv.scores_avail(packed, obs, card, flips, TOGGLE_K, with_used=False)[0].reshape(B, n, n)      # [b, u, v]
    want_T = ref.transpose(0, 2, 1).copy()
    want_T[:, np.arange(n), np.arange(n)] = np.nan
    L, T, st = drv.toggle_avail(packed, obs, card, masks, TOGGLE_K)
    assert same_bytes(L, want_L), (name, kind)
    diag = T[:, np.arange(n), np.arange(n)]
    assert np.isnan(diag).all()
    assert same_bytes(T, want_T), (name, kind, np.argwhere(T.view(U64) != want_T.view(U64))[:5])
    if kind == "heavy":
        assert np.isneginf(T).any() and st & 128
    assert not st & 16
    wl = worklist_for(B, n)
    L2, T2, _ = drv.toggle_avail(packed, obs, card, masks, TOGGLE_K, worklist=wl)
    want = np.full((B, n, n), -7.0)
    for slot, v in enumerate(wl.tolist()):
        if 0 <= v < n:
            b = slot // 2
            keep = np.arange(n) != v
            want[b, v, keep] = want_T[b, v, keep]
    assert (L2 == -7.0).all() and same_bytes(T2, want), (name, kind)
    assert (T2 == -7.0).any() and (T2 != -7.0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Truth
# ---------------------------------------------------------------------------------------------------------------------
def restate_local(data, observed, card, v, parents, k):
    """(local score, m, T) by the definition in numpy: a masked bincount and the formula; T = |LL| / m + penalty"""
    parents = sorted(int(p) for p in parents if p != v)
    fam = (1 << v) | sum(1 << p for p in parents)
    rows = counted(np.asarray(observed, U64), fam)
    m = int(rows.sum())
    r = int(card[v])
    q = 1
    for p in parents:
        q *= int(card[p])
    if m == 0:
        return -np.inf, 0, 0.0
    sub = data[rows]
    key = np.zeros(m, np.int64)
    stride = 1
    for p in parents:
        key += sub[:, p].astype(np.int64) * stride
        stride *= int(card[p])
    _, inv = np.unique(key, return_inverse=True)               # the occupied configurations only: q may be huge
    inv = inv.reshape(-1)
    njk = np.bincount(inv * r + sub[:, v].astype(np.int64), minlength=(int(inv.max()) + 1) * r).reshape(-1, r)
    nj = njk.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = np.where(njk > 0, njk * np.log(njk / nj), 0.0)
    LL = float(terms.sum())
    pen = float(k) * (r - 1) * q
    return LL / m - pen, m, abs(LL) / m + pen


def mp_local(data, observed, card, v, parents, k):
    """the same at 60 digits over bn_score_corpus's counts of the gathered rows: LL / m in mpmath, minus the penalty"""
    parents = sorted(int(p) for p in parents if p != v)
    fam = (1 << v) | sum(1 << p for p in parents)
    rows = counted(np.asarray(observed, U64), fam)
    c = bn.cell_counts(data[rows], card, v, parents)
    mpf = bn.MP.mpf
    total = mpf(0)
    for (n, nj), mult in Counter(zip(c.njk.tolist(), c.nj_cell.tolist())).items():
        total += mult * n * bn.MP.log(mpf(n) / nj)
    pen = mpf(float(k)) * (c.r - 1) * c.q
    return total / c.S - pen, bn.MP.fabs(total) / c.S + pen


def truth_families():
    """n12 `heavy`: every family of its structures with m >= 1"""
    data, card, packed, masks, status = row_dataset("n12")
    obs = mask_set("n12", "heavy")
    return [(b, v) for b in range(len(masks)) for v in range(12) if counted(obs, family_mask(masks, b, v)).any()]


def check_restatement_against_mpmath():
    data, card, packed, masks, status = row_dataset("n12")
    obs = mask_set("n12", "heavy")
    worst = 0.0
    for k in KS:
        for b, v in truth_families():
            ps = sc.mask_bits(masks[b, v])
            assert sc.cells_of(card, v, [p for p in ps if p != v]) <= sc.ORACLE_CELLS
            got, m, T = restate_local(data, obs, card, v, ps, k)
            want, Tmp = mp_local(data, obs, card, v, ps, k)
            err = float(bn.MP.fabs(bn.MP.mpf(got) - want))
            assert err <= bn.RTOL * float(Tmp), (k, b, v, got, float(want), err)
            if float(Tmp) > 0:
                worst = max(worst, err / (bn.RTOL * float(Tmp)))
    return worst


def check_kernels_against_restatement(drv):
    data, card, packed, masks, status = row_dataset("n12")
    obs = mask_set("n12", "heavy")
    for k in KS:
        local, out, used, st = drv.scores_avail(packed, obs, card, masks, k)
        for b in range(len(masks)):
            for v in range(12):
                want, m, T = restate_local(data, obs, card, v, sc.mask_bits(masks[b, v]), k)
                assert used[b, v] == m
                if m == 0:
                    assert np.isneginf(local[b, v])
                else:
                    assert abs(local[b, v] - want) <= bn.RTOL * T, (k, b, v, local[b, v], want)


def hand_cases():
    """[(label, data u8 [S, n], observed u64 [S], card, masks u64 [1, n], k, {v: (closed-form local, m)})]"""
    ln = np.log
    # A -> B, two binary variables, 8 rows, B missing in rows 3, 6, 7.  A: four 0 and four 1 in all 8 rows.  B given A over
    # the 5 rows with B: A = 0 -> (2, 1), A = 1 -> (0, 2)
    A = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.uint8)
    Bv = np.array([0, 0, 1, 1, 1, 1, 0, 0], np.uint8)          # the nibbles of rows 3, 6, 7 are ignored
    seen = np.ones((8, 2), bool)
    seen[[3, 6, 7], 1] = False
    k = 0.25
    ll_b = 2 * ln(2 / 3) + ln(1 / 3)                           # + 2 ln(2 / 2) = 0
    ab = ("A -> B", np.stack([A, Bv], 1), observed_bits(seen), np.array([2, 2], np.uint8), sc.masks_of(2, {1: [0]}), k,
          {0: (8 * ln(0.5) / 8 - k * 1 * 1, 8), 1: (ll_b / 5 - k * 1 * 2, 5)})
    # one variable of three levels observed in a single row: LL = 1 ln(1 / 1) = 0, m = 1, nal = 0 exactly
    one = ("single row", np.array([[2], [1], [0], [1]], np.uint8), np.array([0, 0, 1, 0], U64), np.array([3], np.uint8),
           np.zeros((1, 1), U64), 0.0, {0: (0.0, 1)})
    return [ab, one]


def check_hand_cases(drv=None):
    """the restatement (drv None) or the kernels against the closed forms, within RTOL of |LL| / m + penalty"""
    for label, data, obs, card, masks, k, want in hand_cases():
        if drv is not None:
            local, out, used, st = drv.scores_avail(sc.pack(data), obs, card, masks, k)
            assert st == 0, label
        for v, (value, m) in want.items():
            got, gm, T = restate_local(data, obs, card, v, sc.mask_bits(masks[0, v]), k)
            if drv is not None:
                got, gm = local[0, v], used[0, v]
            assert gm == m and abs(got - value) <= bn.RTOL * T, (label, v, got, value)
            if label == "single row":
                assert got == 0.0 and not np.signbit(got)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Argument refusals (checked before anything is enqueued: dummy pointers do)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []
    c = entry("dvs_bn_scores_avail", cases, batch=4, n_vars=12, n_samples=97, data=D, observed=D, card=D, parents=D, k=0.3, local=D,
              out=D, used=D, status=D, stream=None)
    c(10, "null pointer", observed=None)
    for name in ("data", "card", "parents", "local", "out", "status"):
        c(10, "null pointer", **{name: None})
    c(13, "k must be finite and >= 0", k=-0.5)
    c(13, "k must be finite and >= 0", k=float("nan"))
    c(13, "k must be finite and >= 0", k=float("inf"))
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch and n_samples must be > 0", batch=0)
    c(2, "batch and n_samples must be > 0", n_samples=0)
    c(2, "batch and n_samples must be > 0", batch=0, n_vars=49)                        # sizes before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, observed=None)                        # range before null
    c(10, "null pointer", observed=None, k=-1.0)                                       # null before k

    c = entry("dvs_bn_toggle_scores_avail", cases, batch=4, n_vars=12, n_samples=97, data=D, observed=D, card=D, parents=D, k=0.3,
              worklist=None, local=D, local_bytes=384, toggles=D, toggles_bytes=4608, status=D, stream=None)
    c(10, "null pointer", observed=None)
    for name in ("data", "card", "parents", "local", "toggles", "status"):
        c(10, "null pointer", **{name: None})
    c(13, "k must be finite and >= 0", k=-0.5)
    c(13, "k must be finite and >= 0", k=float("nan"))
    c(13, "k must be finite and >= 0", k=float("-inf"))
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch and n_samples must be > 0", batch=0)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48)
    c(14, "local_bytes < batch * n_vars * 8 = 384", local_bytes=383)
    c(14, "toggles_bytes < batch * n_vars^2 * 8 = 4608", toggles_bytes=4607)
    c(13, "k must be finite and >= 0", k=-1.0, local_bytes=0)                          # k before the sizes
    c(14, "local_bytes", local_bytes=0, toggles_bytes=0)                               # local before toggles
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_bn_scores_avail", "dvs_bn_toggle_scores_avail"}
    run(lib, cases)


def check_refusals_leave_outputs_untouched(drv):
    """the same codes on real buffers: nothing is written"""
    be = drv.be
    data, card, packed, masks, _ = row_dataset("n12")
    B, n = masks.shape
    obs = mask_set("n12", "light")
    d, o, c, m = be.put(packed), be.put(obs), be.put(card), be.put(masks)
    local, out, used = be.put(np.full((B, n), -7.0)), be.put(np.full(B, -7.0)), be.put(np.full((B, n), -7, np.int32))
    L, T, status = be.put(np.full((B, n), -7.0)), be.put(np.full((B, n, n), -7.0)), be.put(np.zeros(1, np.int32))
    head = dict(batch=B, n_vars=n, n_samples=len(data), data=d, observed=o, card=c, parents=m, k=0.3, status=status)

    def score(**kw):
        return call_rc(be, "dvs_bn_scores_avail", **{**head, "local": local, "out": out, "used": used, **kw})

    def toggle(**kw):
        return call_rc(be, "dvs_bn_toggle_scores_avail", **{**head, "worklist": None, "local": L, "local_bytes": B * n * 8,
                                                            "toggles": T, "toggles_bytes": B * n * n * 8, **kw})
    for fn in (score, toggle):
        assert fn(observed=None) == 10
        for bad in (-1.0, float("nan"), float("inf")):
            assert fn(k=bad) == 13
        assert fn(n_vars=49) == 3 and fn(batch=0) == 2
    assert toggle(local_bytes=B * n * 8 - 1) == 14 and str(B * n * 8) in be.lib.dvs_last_error().decode()
    assert toggle(toggles_bytes=B * n * n * 8 - 1) == 14 and str(B * n * n * 8) in be.lib.dvs_last_error().decode()
    for h in (local, out, L, T):
        assert (be.get(h) == -7.0).all()
    assert (be.get(used) == -7).all() and int(be.get(status)[0]) == 0
