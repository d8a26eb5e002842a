"""TEST HELPER: cases, references and the checks themselves for local constraint-based structure learning (csrc/dvs_local.h:
dvs_ci_tests_group, dvs_mmpc_update; dags_vae_search_amd/local.py), written once and run by tests/test_emu_local.py (emulator
build) and tests/test_gpu_local.py (device) on the back ends of tests/scoring_corpus.py.  The CI cases, their mpmath reference
and the tolerances CI_RTOL / P_RTOL / GUARD_FACTOR are those of tests/pc_corpus.py.

References (numpy and plain Python, nothing shared with the kernels)
  dvs_ci_tests    the grouped kernel promises its bytes, test by test; pc.ci_reference holds both to mpmath.
  update_ref      the decisions of dvs_mmpc_update, target by target and group by group.
  mmpc_ref        the whole search on update_ref, its tests answered by a callback: pc.data_test on a data set (numpy counts, p
                  by mpmath) or an exact d-separation oracle.  ref_forward_groups / ref_backward_groups restate the host's
                  enumeration with itertools.
Guards (mmpc_ref on data records them, check_mmpc_guard asserts them before anything is compared)
  decision    every p-value that decides something has |p - alpha| / alpha > GUARD_FACTOR * P_RTOL.
  selection   the member chosen is separated from every other open candidate by a relative gap above the same guard in pmax,
              or, at equal flushed pmax, in smin.  The gap in pmax is taken after 2 * P_FLOOR, the absolute error pc_corpus
              allows a p-value on top of P_RTOL, so that it holds for the tiny p-values too.
  flushing    p-values below 2^-1022 compare as 0.  No pmax of a selection may lie in (0, 2^-1000): asserted on every case but
              the two that TINY_ALLOWED names, sachs at 5000 rows with mi and with x2, which the end-to-end cases must
              include and which have such values.  For those the exact values are pinned, in order, so that one more, one
              fewer or another value fails: mi has 2.129e-303 three times, a normal number 2^16 above the threshold with
              all its digits, once as the winner; x2 has one denormal, 1.84e-315, which flushes to 0 like an underflowed
              value by definition.  On every case no pmax may lie within a factor 2 of the threshold itself, where a
              p-value a few ulp off could fall either way.
"""
import functools
import itertools
import math
from types import SimpleNamespace

import numpy as np

from tests import cpdag_corpus as cp
from tests import pc_corpus as pc
from tests import scoring_corpus as sc
from tests.abi_cases import at, run
from tests.eliminate_corpus import call, call_rc, entry

U64 = np.uint64
MAX_CELLS = pc.MAX_CELLS
NAN_BITS = np.array([np.nan]).tobytes()
FLUSH = 2.0 ** -1022
TINY = 2.0 ** -1000
GUARD = pc.GUARD_FACTOR * pc.P_RTOL


def bits(m):
    return list(cp.bits(int(m)))


def popcount(m):
    return bin(int(m)).count("1")


# ---------------------------------------------------------------------------------------------------------------------
# 1. The grouped kernel
# ---------------------------------------------------------------------------------------------------------------------
def run_group(be, data_h, card_h, n, S, groups, typ, lds_cells):
    """one dvs_ci_tests_group over groups [(y, zs, candidate mask)] -> (rc, out [G, n, 3], status); the output sits between two
    sentinel rows of -7, which must come back untouched"""
    G = len(groups)
    buf = be.put(np.full((G + 2, n, 3), -7.0))
    h = dict(target=be.put(np.array([y for y, _, _ in groups], np.int32)), cond=be.put(np.array([pc.mask_of(zs) for _, zs, _ in groups], U64)),
             candidates=be.put(np.array([c for _, _, c in groups], U64)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_ci_tests_group", n_groups=G, n_vars=n, n_samples=S, data=data_h, card=card_h, test_type=pc.TYPE_ID[typ],
                 lds_cells=lds_cells, out=at(be, buf, n * 24), out_bytes=G * n * 24, **h)
    got = be.get(buf).copy()
    assert (got[0] == -7.0).all() and (got[-1] == -7.0).all(), "written outside out"
    return rc, got[1:-1], int(be.get(h["status"])[0])


def per_test(be, data_h, card_h, n, S, groups, typ, max_cells=MAX_CELLS):
    """the same tests through dvs_ci_tests -> out [G, n, 3] with NaN where nothing was asked, and the status"""
    tests = [(x, y, zs) for y, zs, c in groups for x in bits(c) if x < n]
    want = np.full((len(groups), n, 3), np.nan)
    if not tests:
        return want, 0
    rc, out, status = pc.run_ci(be, data_h, card_h, n, S, tests, typ, max_cells)
    assert rc == 0
    k = 0
    for g, (y, zs, c) in enumerate(groups):
        for x in bits(c):
            if x < n:
                want[g, x] = out[k]
                k += 1
    return want, status


SIX_CONDS = ((), (1,), (0, 3), (1, 3, 4), (0, 1))


def six_groups():
    """every target of the six-variable cases with a few conditioning sets, the candidates all the others"""
    n = 6
    return [(y, zs, ((1 << n) - 1) & ~(1 << y) & ~pc.mask_of(zs)) for y in range(n) for zs in SIX_CONDS if y not in zs]


def check_group_equal_bytes(be, S, typ):
    """sixS<S>: every asked cell is the bytes of dvs_ci_tests and within CI_RTOL / P_RTOL of mpmath; one candidate per pass, all
    of LDS and a ragged last pass give equal bytes; cells not asked are NaN and the status stays 0"""
    name = f"sixS{S}"
    case = pc.ci_case(name)
    n = 6
    card = [int(c) for c in case.card]
    dh, ch = be.put(sc.pack(case.data)), be.put(case.card)
    groups = six_groups()
    assert any(pc.cells_of(card, x, y, zs) == 16 * 16 * 12 for y, zs, c in groups for x in bits(c))
    rc, out, status = run_group(be, dh, ch, n, S, groups, typ, MAX_CELLS)
    assert rc == 0 and status == 0, (rc, status)
    want, wstatus = per_test(be, dh, ch, n, S, groups, typ)
    assert wstatus == 0 and out.tobytes() == want.tobytes(), (name, typ, np.argwhere(out.view(U64) != want.view(U64))[:5])
    worst, asked = 0.0, 0
    for g, (y, zs, c) in enumerate(groups):
        for x in range(n):
            if not (c >> x) & 1:
                assert out[g, x].tobytes() == NAN_BITS * 3, (g, x)
                continue
            stat, df, T = pc.ci_reference(name, x, y, zs, typ)
            assert out[g, x, 1] == df
            err = abs(pc.mpmath.mpf(float(out[g, x, 0])) - stat)
            assert out[g, x, 0] >= 0.0 and err <= pc.CI_RTOL * T, (name, typ, g, x, float(err), T)
            pe = pc.p_error(out[g, x, 2], df, out[g, x, 0])
            assert 0.0 <= out[g, x, 2] <= 1.0 and pe <= pc.P_RTOL, (name, typ, g, x, pe)
            worst = max(worst, pe)
            asked += 1
    passes = {n_passes([pc.cells_of(card, x, y, zs) for x in bits(c)], MAX_CELLS) for y, zs, c in groups}
    for g, (y, zs, c) in enumerate(groups):
        sizes = [pc.cells_of(card, x, y, zs) for x in bits(c)]
        ragged = sum(sizes) - min(sizes)                     # everything but the last table fits the first pass, or less
        for lds in (max(sizes), max(max(sizes), ragged)):
            rc, one, status = run_group(be, dh, ch, n, S, [groups[g]], typ, lds)
            assert rc == 0 and status == 0 and one[0].tobytes() == out[g].tobytes(), (name, typ, g, lds)
            passes.add(n_passes(sizes, lds))
    assert {1, 2} <= passes and max(passes) >= 4, passes
    rc, again, _ = run_group(be, dh, ch, n, S, groups, typ, MAX_CELLS)
    assert again.tobytes() == out.tobytes()                  # two runs give equal bytes
    print(f"{name} {typ}: {asked} cells in {len(groups)} groups, passes seen {sorted(passes)}, worst relative p error {worst:.3e}")
    return asked


def n_passes(sizes, lds):
    """the passes a workgroup takes over tables of these sizes, in order, with lds cells"""
    count, room = 0, 0
    for s in sizes:
        if s > room:
            count, room = count + 1, lds
        room -= s
    return count


def check_group_refusals(be):
    """a table above lds_cells is refused alone; x = y, x in Z, y in Z, bits and indices at or above n_vars set bit 4; cells not
    asked stay NaN without a status bit"""
    case = pc.ci_case("sixS257")
    S, n = case.data.shape
    dh, ch = be.put(sc.pack(case.data)), be.put(case.card)
    full = (1 << n) - 1
    nan3 = NAN_BITS * 3
    big = [(5, (0, 1), full & ~0b100011)]                    # x = 2 has 16 * 16 * 12 cells, x = 3 has 384, x = 4 has 192
    want, _ = per_test(be, dh, ch, n, S, big, "mi")
    rc, out, status = run_group(be, dh, ch, n, S, big, "mi", 16 * 16 * 12)
    assert rc == 0 and status == 0 and out.tobytes() == want.tobytes()
    rc, out, status = run_group(be, dh, ch, n, S, big, "mi", 16 * 16 * 12 - 1)
    assert status == 16 and out[0, 2].tobytes() == nan3 and out[0, [3, 4]].tobytes() == want[0, [3, 4]].tobytes()
    rc, out, status = run_group(be, dh, ch, n, S, big, "x2-adf", 192)
    assert status == 16 and np.isnan(out[0, [2, 3]]).all() and not np.isnan(out[0, 4]).any()
    rc, out, status = run_group(be, dh, ch, n, S, big, "mi", 191)                     # nothing fits: every candidate refused
    assert status == 16 and np.isnan(out).all()
    good = (0, (), 0b000110)
    ref, _ = per_test(be, dh, ch, n, S, [good], "mi")
    for bad in ((2, (), 0b000101),                           # x = y
                (0, (1, 3), 0b001110),                       # x in Z
                (0, (0,), 0b000110),                         # y in Z
                (0, (6,), 0b000110),                         # a bit of Z at n_vars
                (0, (63,), 0b000110),
                (6, (), 0b000110),                           # y outside the data set
                (-1, (), 0b000110),
                (0, (), 0b000110 | 1 << 6),                  # a candidate bit at n_vars: no cell, bit 4
                (0, (), 0b000110 | 1 << 63),
                (0, (), 0b010110)):                          # a candidate of one level is evaluated (df 0), not refused
        rc, out, status = run_group(be, dh, ch, n, S, [good, bad, good], "mi", MAX_CELLS)
        y, zs, c = bad
        legal = 0 <= y < n and y not in zs and all(z < n for z in zs)
        refused = {x for x in bits(c) if x >= n or not legal or x == y or x in zs}
        assert rc == 0 and status == (16 if refused else 0), (bad, status)
        assert out[0].tobytes() == ref[0].tobytes() == out[2].tobytes(), bad           # the neighbours are evaluated
        for x in range(n):
            asked_ok = (c >> x) & 1 and x not in refused
            assert np.isnan(out[1, x]).all() != bool(asked_ok), (bad, x, out[1, x])
        if not refused:
            assert out[1, 4, 1] == 0.0 and out[1, 4, 2] == 1.0
    rc, out, status = run_group(be, dh, ch, n, S, [(3, (1,), 0)], "mi", MAX_CELLS)   # nothing asked
    assert rc == 0 and status == 0 and out.tobytes() == nan3 * n
    zero = case.card.copy()
    zero[1] = 0                                              # a variable of no levels has no table: as x, as y, in Z
    zh = be.put(zero)
    for grp, refused in (((0, (), 0b001110), {1}), ((1, (), 0b001101), {0, 2, 3}), ((0, (1,), 0b001100), {2, 3})):
        rc, out, status = run_group(be, dh, zh, n, S, [grp], "mi", MAX_CELLS)
        assert rc == 0 and status == 16 and {x for x in bits(grp[2]) if np.isnan(out[0, x]).all()} == refused, grp


@functools.lru_cache(maxsize=None)
def wide_case():
    """48 variables, 300 rows, seeded levels with some dependence, mixed level counts; the three conditioning variables that
    straddle the 16-variable words are small so that every table fits"""
    rng = np.random.default_rng(2701)
    cards = [int(c) for c in rng.choice([2, 3, 4, 5, 16], 48, p=[0.3, 0.3, 0.2, 0.1, 0.1])]
    for z, c in ((15, 2), (16, 3), (33, 2), (40, 16), (47, 16)):
        cards[z] = c
    data, card = sc.synthetic_dataset(48, 300, cards, seed=2702)
    return data, card


def check_group_wide(be):
    """n = 48: all 47 others as candidates, Z across the word boundaries, targets in every word; bytes of dvs_ci_tests"""
    data, card = wide_case()
    S, n = data.shape
    dh, ch = be.put(sc.pack(data)), be.put(card)
    full = (1 << n) - 1
    Z = (15, 16, 33)
    groups = [(y, Z, full & ~(1 << y)) for y in (0, 17, 40, 47)] + [(31, (), full & ~(1 << 31)), (32, (47,), full & ~(1 << 32))]
    want, wstatus = per_test(be, dh, ch, n, S, groups, "mi")
    assert wstatus == 16                                     # the members of Z are candidates too, and refused as dvs_ci_tests does
    for typ, lds in (("mi", MAX_CELLS), ("x2-adf", MAX_CELLS), ("mi", 16 * 16 * 12 + 5)):
        want, _ = per_test(be, dh, ch, n, S, groups, typ)
        rc, out, status = run_group(be, dh, ch, n, S, groups, typ, lds)
        assert rc == 0 and status == 16
        assert out.tobytes() == want.tobytes(), (typ, lds, np.argwhere(out.view(U64) != want.view(U64))[:5])
        assert int(np.isnan(out[0, :, 2]).sum()) == 4 and np.isnan(out[0, [0, 15, 16, 33]]).all()
    sizes = [pc.cells_of(card, x, 40, Z) for x in range(n) if x not in Z + (40,)]
    assert n_passes(sizes, MAX_CELLS) >= 2 and n_passes(sizes, 16 * 16 * 12 + 5) > n_passes(sizes, MAX_CELLS)
    return len(groups) * 47


# ---------------------------------------------------------------------------------------------------------------------
# 2. dvs_mmpc_update
# ---------------------------------------------------------------------------------------------------------------------
def new_state(n, cand=None):
    full = (1 << n) - 1
    return SimpleNamespace(cpc=[0] * n, cand=[full & ~(1 << t) for t in range(n)] if cand is None else list(cand), last=[-7] * n,
                           pmax=np.zeros((n, n)), smin=np.full((n, n), np.inf), sepset=np.zeros((n, n), U64))


def flushed(p):
    return 0.0 if p < FLUSH else float(p)


def update_ref(n, phase, groups, out, alpha, st, watch=None):
    """the definition of dvs_mmpc_update in include/dvs_local.h -> (state, refused, result [n, 2]); `watch(kind, ...)` sees every
    decision and every selection"""
    target, cond, candidates, offsets = groups
    G = len(target)
    new = SimpleNamespace(cpc=list(st.cpc), cand=list(st.cand), last=list(st.last), pmax=st.pmax.copy(), smin=st.smin.copy(),
                          sepset=st.sepset.copy())
    result, refused = np.zeros((n, 2), np.int64), 0
    for t in range(n):
        open_ = (st.cand[t] if phase == 0 else st.cpc[t]) & ((1 << n) - 1) & ~(1 << t)
        left = 0
        for g in range(max(int(offsets[t]), 0), min(int(offsets[t + 1]), G)):
            if target[g] != t:
                continue
            for x in bits(open_ & ~left & int(candidates[g])):
                stat, p = float(out[g, x, 0]), float(out[g, x, 2])
                if math.isnan(p):
                    refused += 1
                    continue
                if watch:
                    watch("decision", p)
                if p > alpha:
                    left |= 1 << x
                    new.sepset[t, x] = cond[g]
                elif phase == 0:
                    if p > new.pmax[t, x]:
                        new.pmax[t, x] = p
                    if stat < new.smin[t, x]:
                        new.smin[t, x] = stat
        if phase == 1:
            new.cpc[t] = st.cpc[t] & ~left
            result[t] = (-1, popcount(left))
            continue
        still = bits(open_ & ~left)
        F = min(still, key=lambda x: (flushed(new.pmax[t, x]), -new.smin[t, x], x)) if still else -1
        if watch and still:
            watch("selection", F, [(x, float(new.pmax[t, x]), float(new.smin[t, x])) for x in still])
        f = 1 << F if F >= 0 else 0
        new.cpc[t] = st.cpc[t] | f
        new.cand[t] = st.cand[t] & ~left & ~f
        new.last[t] = F
        result[t] = (F, popcount(left))
    return new, refused, result


def run_update(be, n, phase, groups, out, alpha, st):
    """dvs_mmpc_update on the back end -> (state, refused, result), cpc_next and cand_next pre-filled with a pattern"""
    target, cond, candidates, offsets = groups
    G = len(target)
    h = dict(target=be.put(np.array(target, np.int32)), cond=be.put(np.array(cond, U64)), candidates=be.put(np.array(candidates, U64)),
             group_offsets=be.put(np.array(offsets, np.int64)), out=be.put(np.ascontiguousarray(out, np.float64)),
             cpc=be.put(np.array(st.cpc, U64)), cand=be.put(np.array(st.cand, U64)),
             cpc_next=be.put(np.full(n, 0xA5A5A5A5A5A5A5A5, U64)), cand_next=be.put(np.full(n, 0xA5A5A5A5A5A5A5A5, U64)),
             last=be.put(np.array(st.last, np.int32)), pmax=be.put(st.pmax.copy()), smin=be.put(st.smin.copy()),
             sepset=be.put(st.sepset.copy()), refused=be.put(np.full(1, -7, np.int32)), result=be.put(np.full((n, 2), -7, np.int64)))
    call(be, "dvs_mmpc_update", n_vars=n, n_groups=G, phase=phase, out_bytes=G * n * 24, alpha=alpha, state_bytes=n * n * 8,
         result_bytes=n * 16, **h)
    g = lambda k: be.get(h[k]).copy()
    new = SimpleNamespace(cpc=[int(v) for v in g("cpc_next")], cand=[int(v) for v in g("cand_next")], last=[int(v) for v in g("last")],
                          pmax=g("pmax"), smin=g("smin"), sepset=g("sepset"))
    return new, int(g("refused")[0]), g("result")


def same_state(a, b):
    return (a.cpc == b.cpc and a.cand == b.cand and a.last == b.last and a.pmax.tobytes() == b.pmax.tobytes()
            and a.smin.tobytes() == b.smin.tobytes() and a.sepset.tobytes() == b.sepset.tobytes())


def assert_update(be, n, phase, groups, out, alpha, st, what):
    want = update_ref(n, phase, groups, out, alpha, st)
    got = run_update(be, n, phase, groups, out, alpha, st)
    assert same_state(got[0], want[0]), (what, vars(got[0]), vars(want[0]))
    assert got[1] == want[1] and got[2].tobytes() == want[2].tobytes(), (what, got[1:], want[1:])
    again = run_update(be, n, phase, groups, out, alpha, st)
    assert same_state(again[0], got[0]) and again[1:][0] == got[1] and again[2].tobytes() == got[2].tobytes()
    return want


def hand_round():
    """n = 7, alpha = 0.05.  Target 0: a tie on p broken by the statistic.  Target 1: a tie on both, broken by the index.  Target
    2: p = 0 and p = 5e-324 tie, and the statistic decides for the denormal one.  Target 3: NaN cells counted and ignored; a
    candidate that an earlier group dismissed is not looked at again (its later NaN is not counted, its later small p not
    used).  Target 4: every candidate leaves: last = -1.  Target 5: no group at all, no candidate: last = -1.  Target 6: a
    group under another target's name is ignored (read, it would dismiss every candidate): with nothing seen, the index decides."""
    n, nan = 7, float("nan")
    full = (1 << n) - 1
    rows = [  # (target, cond, candidates, {x: (stat, p)})
        (0, 0b0000000, full & ~1, {1: (9.0, 0.01), 2: (12.0, 0.01), 3: (30.0, 0.02), 4: (1.0, 0.5), 5: (8.0, 0.01), 6: (7.0, 0.03)}),
        (1, 0b0000000, 0b1111101, {0: (5.0, 0.02), 2: (4.0, 0.001), 3: (4.0, 0.001), 4: (4.0, 0.001), 5: (3.0, 0.001), 6: (2.0, 0.04)}),
        (2, 0b0000001, 0b1111010, {1: (900.0, 0.0), 3: (950.0, 5e-324), 4: (800.0, 1e-310), 5: (3.0, 0.04), 6: (2.0, 0.05)}),
        (2, 0b0000011, 0b1111000, {3: (940.0, 0.0), 4: (960.0, 0.0), 5: (2.5, 0.045), 6: (0.1, 0.9)}),
        (3, 0b0000001, 0b1110110, {1: (nan, nan), 2: (0.5, 0.7), 4: (6.0, 0.02), 5: (nan, nan), 6: (5.0, 0.03)}),
        (3, 0b0000010, 0b1110100, {2: (nan, nan), 4: (5.0, 0.03), 5: (7.0, 0.01), 6: (nan, nan)}),
        (3, 0b0000011, 0b1110100, {2: (99.0, 0.0), 4: (4.0, 0.04), 5: (6.0, 0.02), 6: (6.0, 0.02)}),
        (4, 0b0000000, 0b1101111, {x: (0.1, 0.9) for x in (0, 1, 2, 3, 5, 6)}),
        (0, 0b0000000, 0b0111111, {x: (0.1, 0.9) for x in range(6)}),
    ]
    out = np.full((len(rows), n, 3), nan)
    for g, (_, _, _, cells) in enumerate(rows):
        for x, (s, p) in cells.items():
            out[g, x] = (s, 1.0, p)
    groups = ([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [0, 1, 2, 4, 7, 8, 8, 9])
    st = new_state(n)
    st.cand[1] = 0b1111101
    st.cand[2] = 0b1111010
    st.cand[3] = 0b1110110
    st.cand[5] = 0
    st.cpc[5] = 0b0000011
    st.pmax[3, 5], st.smin[3, 5] = 0.015, 6.5                # carried in from an earlier round
    st.pmax[3, 1], st.smin[3, 1] = 0.04, 2.0                 # likewise: in this round variable 1 is refused only
    return n, groups, out, st


def check_update_hand(be):
    n, groups, out, st = hand_round()
    want, refused, result = assert_update(be, n, 0, groups, out, 0.05, st, "hand forward")
    assert want.last == [2, 2, 3, 5, -1, -1, 0], want.last
    assert result[:, 1].tolist() == [1, 0, 1, 1, 6, 0, 0] and refused == 3
    assert want.cpc[:3] == [0b100, 0b100, 0b1000] and want.cpc[5] == 0b11 and want.cand[0] == 0b1101010
    assert want.pmax[2, 4] == 1e-310 and want.smin[2, 3] == 940.0 and want.sepset[2, 6] == 0b11 and want.sepset[3, 2] == 1
    assert want.pmax[3, 2] == 0.0 and want.pmax[3, 5] == 0.02 and want.smin[3, 5] == 6.0 and want.cand[6] == 0b0111110 and want.cpc[6] == 1
    # the backward phase on a state of its own: members leave by the first group that separates them, nothing is selected
    cpc = [0b0111110, 0b0001101, 0, 0b1110110, 0, 0, 0]
    back = new_state(n, cand=[0x5A] * n)
    back.cpc, back.last = cpc, [3, -1, -1, 2, -1, -1, -1]
    bgroups = ([0, 0, 1, 3, 3], [0, 0b10, 0, 0b10, 0b100], [0b0111110, 0b0111100, 0b0001101, 0b1110100, 0b1110010], [0, 2, 3, 3, 5, 5, 5, 5])
    bout = np.full((5, n, 3), float("nan"))
    for g, cells in enumerate(({1: 0.01, 2: 0.2, 3: 0.01, 4: 0.05, 5: 0.0}, {2: 0.9, 3: 0.3, 4: 0.06, 5: float("nan")}, {0: 0.01, 2: 0.01, 3: 0.01},
                               {2: 0.5, 4: 0.01, 5: 0.01, 6: float("nan")}, {1: 0.5, 4: 0.9, 5: 0.01, 6: 0.01})):
        for x, p in cells.items():
            bout[g, x] = (3.0, 1.0, p)
    want, refused, result = assert_update(be, n, 1, bgroups, bout, 0.05, back, "hand backward")
    assert want.cpc == [0b0100010, 0b0001101, 0, 0b1100000, 0, 0, 0] and refused == 2
    assert want.cand == [0x5A] * n and want.last == back.last and result.tolist() == [[-1, 3], [-1, 0], [-1, 0], [-1, 3], [-1, 0], [-1, 0], [-1, 0]]
    assert [int(want.sepset[0, x]) for x in (2, 3, 4)] == [0, 0b10, 0b10] and int(want.sepset[3, 1]) == 0b100
    # n = 1: one group that asks nothing
    one = assert_update(be, 1, 0, ([0], [0], [0], [0, 1]), np.full((1, 1, 3), float("nan")), 0.05, new_state(1), "n = 1")[0]
    assert one.last == [-1] and one.cpc == [0] and one.cand == [0]


def check_update_seeded(be, n, seed, rounds=3):
    """seeded p-values and statistics from small sets (so that ties of every kind occur), several rounds on the evolving state,
    then a backward round; n = 48 uses every lane a data set can have"""
    rng = np.random.default_rng(seed)
    full = (1 << n) - 1
    st = new_state(n)
    saw_tie = 0
    for r in range(rounds + 1):
        phase = 1 if r == rounds else 0
        target, cond, candidates, offsets = [], [], [], [0]
        for t in range(n):
            k = int(rng.integers(0, 4)) if n > 1 else 1
            zs = sorted(int(z) for z in rng.integers(0, 1 << min(n, 20), k))
            pool = st.cand[t] if phase == 0 else st.cpc[t]
            for z in zs:
                target.append(t)
                cond.append(z)
                candidates.append(pool & ~z & int(rng.integers(0, 1 << n)) | (int(rng.integers(0, 1 << n)) & full & ~pool & ~(1 << t) if rng.random() < 0.2 else 0))
            offsets.append(len(target))
        if not target:
            target, cond, candidates, offsets = [0], [0], [0], [0] + [1] * n
        G = len(target)
        out = np.full((G, n, 3), np.nan)
        for g in range(G):
            for x in bits(candidates[g]):
                p = rng.choice([0.0, 5e-324, 1e-310, 3e-308, 0.001, 0.02, 0.05, 0.050001, 0.4, np.nan], p=[0.15, 0.1, 0.1, 0.05, 0.2, 0.15, 0.05, 0.05, 0.1, 0.05])
                out[g, x] = (np.nan, np.nan, np.nan) if np.isnan(p) else (float(rng.choice([1.5, 40.0, 40.000001, 700.0])), 2.0, p)
        ties = []
        update_ref(n, phase, (target, cond, candidates, offsets), out, 0.05, st,
                   watch=lambda kind, *a: ties.append(a) if kind == "selection" else None)
        saw_tie += sum(1 for F, still in ties if sum(1 for x, pm, sm in still if flushed(pm) == flushed(dict((c[0], c[1]) for c in still)[F])) > 1)
        st = assert_update(be, n, phase, (target, cond, candidates, offsets), out, 0.05, st, (n, seed, r))[0]
    assert n == 1 or saw_tie > 0
    return st


# ---------------------------------------------------------------------------------------------------------------------
# 3. The algorithm restated
# ---------------------------------------------------------------------------------------------------------------------
def subsets_up_to(members, most):
    ids = bits(members)
    return [pc.mask_of(s) for k in range(min(most, len(ids)) + 1) for s in itertools.combinations(ids, k)]


def ref_marginal_groups(n, cand):
    ts = [t for t in range(n) if cand[t]]
    return ts, [0] * len(ts), [cand[t] for t in ts], [sum(1 for u in ts if u < t) for t in range(n + 1)]


def ref_forward_groups(n, st, max_cond):
    target, cond, candidates, offsets = [], [], [], [0]
    for t in range(n):
        F = st.last[t]
        if F >= 0 and max_cond >= 1:
            for z in sorted((1 << F) | s for s in subsets_up_to(st.cpc[t] & ~(1 << F), max_cond - 1)):
                target.append(t)
                cond.append(z)
                candidates.append(st.cand[t])
        offsets.append(len(target))
    return target, cond, candidates, offsets


def ref_backward_groups(n, st, max_cond):
    target, cond, candidates, offsets = [], [], [], [0]
    for t in range(n):
        for z in sorted(subsets_up_to(st.cpc[t], max_cond)):
            target.append(t)
            cond.append(z)
            candidates.append(st.cpc[t] & ~z)
        offsets.append(len(target))
    return target, cond, candidates, offsets


def finish(n, st, forward, per_round, refused):
    skeleton = [sum(1 << x for x in bits(st.cpc[t]) if (st.cpc[x] >> t) & 1) for t in range(n)]
    return SimpleNamespace(forward=forward, cpc=list(st.cpc), skeleton=skeleton, sepset=st.sepset, groups_per_round=per_round,
                           refused=refused, asymmetric=sum(popcount(st.cpc[t] & ~skeleton[t]) for t in range(n)))


def mmpc_driver(n, max_cond, round_fn):
    """the rounds of local.py's mmpc, with `round_fn(phase, groups, state) -> (state, refused)` doing a round's tests and update"""
    st = new_state(n)
    per_round, refused = [], 0
    groups = ref_marginal_groups(n, st.cand)
    while groups[0]:
        st, r = round_fn(0, groups, st)
        refused += r
        per_round.append(len(groups[0]))
        groups = ref_forward_groups(n, st, max_cond)
    if max_cond == 0:
        st.cpc, st.cand = [c | d for c, d in zip(st.cpc, st.cand)], [0] * n
    forward = list(st.cpc)
    groups = ref_backward_groups(n, st, max_cond)
    if groups[0]:
        st, r = round_fn(1, groups, st)
        refused += r
        per_round.append(len(groups[0]))
    return finish(n, st, forward, per_round, refused)


def mmpc_ref(n, tester, alpha=pc.ALPHA, max_cond=3, watch=None):
    """MMPC with `tester(x, t, zmask) -> (statistic, p)` (or None: refused) answering every test"""
    def round_fn(phase, groups, st):
        target, cond, candidates, _ = groups
        out = np.full((len(target), n, 3), np.nan)
        for g, (t, z, c) in enumerate(zip(target, cond, candidates)):
            for x in bits(c):
                r = tester(x, t, z)
                if r is not None:
                    out[g, x] = (r[0], 1.0, r[1])
        new, refused, _ = update_ref(n, phase, groups, out, alpha, st, watch)
        return new, refused
    return mmpc_driver(n, max_cond, round_fn)


def mmpc_raw(be, data, card, typ, alpha=pc.ALPHA, max_cond=3):
    """MMPC through the raw C ABI on a back end: the launch sequence of dags_vae_search_amd/local.py"""
    S, n = data.shape
    dh, ch = be.put(sc.pack(data)), be.put(card)
    cardl = [int(c) for c in card]
    hstatus = be.put(np.zeros(1, np.int32))
    dev = SimpleNamespace(last=be.put(np.full(n, -1, np.int32)), pmax=be.put(np.zeros((n, n))), smin=be.put(np.full((n, n), np.inf)),
                          sepset=be.put(np.zeros((n, n), U64)), refused=be.put(np.zeros(1, np.int32)), result=be.put(np.zeros((n, 2), np.int64)))

    def round_fn(phase, groups, st):
        target, cond, candidates, offsets = groups
        G = len(target)
        need = max(sum(pc.cells_of(cardl, x, t, bits(z)) for x in bits(c)) for t, z, c in zip(target, cond, candidates))
        ht, hz, hc = be.put(np.array(target, np.int32)), be.put(np.array(cond, U64)), be.put(np.array(candidates, U64))
        out = be.put(np.zeros((G, n, 3)))
        call(be, "dvs_ci_tests_group", n_groups=G, n_vars=n, n_samples=S, data=dh, card=ch, target=ht, cond=hz, candidates=hc,
             test_type=pc.TYPE_ID[typ], lds_cells=max(1, min(need, MAX_CELLS)), out=out, out_bytes=G * n * 24, status=hstatus)
        cpc_next, cand_next = be.put(np.zeros(n, U64)), be.put(np.zeros(n, U64))
        call(be, "dvs_mmpc_update", n_vars=n, n_groups=G, phase=phase, target=ht, cond=hz, candidates=hc,
             group_offsets=be.put(np.array(offsets, np.int64)), out=out, out_bytes=G * n * 24, alpha=alpha, cpc=be.put(np.array(st.cpc, U64)),
             cand=be.put(np.array(st.cand, U64)), cpc_next=cpc_next, cand_next=cand_next, last=dev.last, pmax=dev.pmax, smin=dev.smin,
             sepset=dev.sepset, state_bytes=n * n * 8, refused=dev.refused, result=dev.result, result_bytes=n * 16)
        new = SimpleNamespace(cpc=[int(v) for v in be.get(cpc_next)], cand=[int(v) for v in be.get(cand_next)],
                              last=[int(v) for v in be.get(dev.last)], pmax=None, smin=None, sepset=be.get(dev.sepset).copy())
        return new, int(be.get(dev.refused)[0])
    got = mmpc_driver(n, max_cond, round_fn)
    got.status = int(be.get(hstatus)[0])
    return got


E2E_CASES = pc.E2E_CASES
EMU_E2E_CASES = pc.EMU_E2E_CASES
# what the prototype of the definition measured, pinned: asia 4 forward rounds and 58 groups with its skeleton rows, sachs 7
# forward rounds and 246 groups with 16 edges (the last entry of groups_per_round is the backward pass)
KNOWN = {("asia", 5000, "mi"): dict(groups_per_round=[8, 7, 10, 4, 29], edges=5, skeleton=[0, 24, 32, 34, 130, 12, 0, 16]),
         ("sachs", 5000, "mi"): dict(groups_per_round=[11, 11, 22, 20, 21, 22, 16, 123], edges=16)}
# the pmax values in (0, 2^-1000) that selections of the reference meet, ascending: none anywhere else (see "flushing" above)
TINY_ALLOWED = {("sachs", 5000, "mi"): [2.129199600088871e-303, 2.129199600088871e-303, 2.1291996000891124e-303],
                ("sachs", 5000, "x2"): [1.83668426e-315]}


@functools.lru_cache(maxsize=None)
def e2e_reference(name, S, typ, max_cond=3):
    """mmpc_ref on the data with its guards: the closest decision, the narrowest selection, the ties on p"""
    data, card = pc.e2e_data(name, S)
    cardl = [int(c) for c in card]
    seen = SimpleNamespace(decision=float("inf"), gap=float("inf"), ties=0, tiny=[], at_flush=0)

    def watch(kind, *a):
        if kind == "decision":
            seen.decision = min(seen.decision, abs(a[0] - pc.ALPHA) / pc.ALPHA)
            return
        F, still = a
        mine = next(c for c in still if c[0] == F)
        seen.tiny += [pm for _, pm, _ in still if 0.0 < pm < TINY]
        seen.at_flush += sum(1 for _, pm, _ in still if FLUSH / 2 <= pm <= FLUSH * 2)
        for x, pm, sm in still:
            if x == F:
                continue
            if flushed(pm) != flushed(mine[1]):
                gap = (abs(pm - mine[1]) - 2 * pc.P_FLOOR) / max(pm, mine[1])
            else:
                seen.ties += 1
                gap = abs(sm - mine[2]) / max(sm, mine[2]) if sm != mine[2] else 0.0
            seen.gap = min(seen.gap, gap)

    @functools.lru_cache(maxsize=None)
    def tester(x, t, z):
        if pc.cells_of(cardl, x, t, bits(z)) > MAX_CELLS:
            return None
        stat, _, p = pc.data_test(data, card, x, t, z, typ)
        return stat, p
    ref = mmpc_ref(data.shape[1], tester, pc.ALPHA, max_cond, watch)
    ref.seen = seen
    ref.tests = tester.cache_info().currsize
    return ref


def check_mmpc_guard(name, S, typ):
    ref = e2e_reference(name, S, typ)
    s = ref.seen
    print(f"{name} S {S} {typ}: groups {ref.groups_per_round} = {sum(ref.groups_per_round)}, distinct tests {ref.tests}, edges "
          f"{sum(popcount(a) for a in ref.skeleton) // 2}, asymmetric {ref.asymmetric}, closest |p - alpha| / alpha {s.decision:.3e}, "
          f"narrowest selection gap {s.gap:.3e}, ties on p {s.ties}, pmax in (0, 2^-1000) {sorted(s.tiny)}, next to 2^-1022 {s.at_flush} "
          f"(guard {GUARD:.1e})")
    assert s.decision > GUARD and s.gap > GUARD and s.at_flush == 0, (name, S, typ, vars(s))
    allowed = TINY_ALLOWED.get((name, S, typ), [])
    assert len(s.tiny) == len(allowed) and all(abs(a - b) <= 1e-6 * b for a, b in zip(sorted(s.tiny), allowed)), (name, S, typ, s.tiny)
    facts = dict(groups_per_round=ref.groups_per_round, edges=sum(popcount(a) for a in ref.skeleton) // 2, skeleton=ref.skeleton)
    for key, value in KNOWN.get((name, S, typ), {}).items():
        assert facts[key] == value, (name, S, typ, key, facts[key], value)
    return ref


def assert_same_mmpc(got, ref, what):
    assert got.groups_per_round == ref.groups_per_round, (what, got.groups_per_round, ref.groups_per_round)
    assert got.forward == ref.forward, (what, "forward", got.forward, ref.forward)
    assert got.cpc == ref.cpc, (what, "cpc")
    assert got.skeleton == ref.skeleton, (what, "skeleton")
    assert got.sepset.tobytes() == ref.sepset.tobytes(), (what, "sepsets")
    assert (got.refused, got.asymmetric) == (ref.refused, ref.asymmetric), what


def check_e2e_raw(be, name, S, typ):
    ref = check_mmpc_guard(name, S, typ)
    data, card = pc.e2e_data(name, S)
    got = mmpc_raw(be, data, card, typ)
    assert got.refused == 0 and got.status == 0
    assert_same_mmpc(got, ref, (name, S, typ))
    if (name, S, typ) == ("asia", 5000, "mi"):
        assert ref.skeleton == pc.e2e_reference(name, S, typ).adj           # on this case MMPC and PC-stable agree
        for cap in (0, 1):
            assert_same_mmpc(mmpc_raw(be, data, card, typ, max_cond=cap), e2e_reference(name, S, typ, cap), ("cap", cap))
    return got


def check_oracle_all_dags(n):
    """mmpc_ref fed by exact d-separation returns the skeleton of every labelled DAG on n vertices (once per equivalence class)"""
    seen = {}
    for P in cp.all_dags(n):
        key = cp.class_key(P)
        if key in seen:
            continue
        independent = pc.dsep_oracle(P)
        # a dependent pair: p = 0 with a statistic that does not say more than that; an independent one: p = 1
        r = mmpc_ref(n, lambda x, t, z: (0.0, 1.0) if independent(x, t, z) else (1.0, 0.0), max_cond=3)
        kids = cp.children_rows(P)
        assert r.skeleton == [int(P[v]) | int(kids[v]) for v in range(n)], (P, r.skeleton)
        seen[key] = r
    assert len(seen) == cp.CLASS_COUNTS[n]
    return len(seen), sum(r.asymmetric for r in seen.values())


# ---------------------------------------------------------------------------------------------------------------------
# 4. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []
    nan = float("nan")
    c = entry("dvs_ci_tests_group", cases, n_groups=8, n_vars=12, n_samples=100, data=D, card=D, target=D, cond=D, candidates=D,
              test_type=0, lds_cells=729, out=D, out_bytes=2304, status=D, stream=None)
    c(2, "n_groups and n_samples must be > 0", n_groups=0)
    c(2, "n_groups and n_samples must be > 0", n_samples=-1)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(12, "test_type is not a dvs_ci_type", test_type=4)
    c(12, "test_type is not a dvs_ci_type", test_type=-1)
    c(13, "lds_cells must be in [1, 36864]", lds_cells=0)
    c(13, "lds_cells must be in [1, 36864]", lds_cells=36865)
    c(2, "n_groups * n_vars must be < 2^31", n_groups=1 << 27, n_vars=16, out_bytes=1 << 40)
    for name in ("data", "card", "target", "cond", "candidates", "out", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "out_bytes < n_groups * n_vars * 24 = 2304", out_bytes=2303)
    c(2, "n_groups and n_samples must be > 0", n_groups=0, n_vars=49)                  # sizes before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, test_type=9)                          # n_vars before the type
    c(12, "test_type is not a dvs_ci_type", test_type=9, lds_cells=0)                  # the type before lds_cells
    c(13, "lds_cells must be in [1, 36864]", lds_cells=0, n_groups=1 << 30)            # lds_cells before the product
    c(2, "n_groups * n_vars must be < 2^31", n_groups=1 << 30, data=None)              # the product before null
    c(10, "null pointer", status=None, out_bytes=0)                                    # null before out_bytes

    c = entry("dvs_mmpc_update", cases, n_vars=12, n_groups=30, phase=0, target=D, cond=D, candidates=D, group_offsets=D, out=D,
              out_bytes=8640, alpha=0.05, cpc=D, cand=D, cpc_next=D, cand_next=D, last=D, pmax=D, smin=D, sepset=D, state_bytes=1152,
              refused=D, result=D, result_bytes=192, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_groups must be > 0", n_groups=0)
    c(2, "n_groups * n_vars must be < 2^31", n_groups=1 << 28, out_bytes=1 << 40)
    c(13, "phase must be 0 (forward) or 1 (backward)", phase=2)
    c(13, "phase must be 0 (forward) or 1 (backward)", phase=-1)
    c(13, "alpha must be in [0, 1]", alpha=nan)
    c(13, "alpha must be in [0, 1]", alpha=1.5)
    c(13, "alpha must be in [0, 1]", alpha=-0.1)
    for name in ("target", "cond", "candidates", "group_offsets", "out", "cpc", "cand", "cpc_next", "cand_next", "last", "pmax", "smin",
                 "sepset", "refused", "result"):
        c(10, "null pointer", **{name: None})
    c(14, "out_bytes < n_groups * n_vars * 24 = 8640", out_bytes=8639)
    c(14, "state_bytes < n_vars^2 * 8 = 1152", state_bytes=1151)
    c(14, "result_bytes < n_vars * 16 = 192", result_bytes=191)
    c(3, "n_vars must be in [1, 48]", n_vars=49, n_groups=0)                           # n_vars before n_groups
    c(2, "n_groups must be > 0", n_groups=0, phase=5)                                  # n_groups before the phase
    c(13, "phase must be", phase=5, alpha=nan)                                         # the phase before alpha
    c(13, "alpha must be in [0, 1]", alpha=2.0, target=None)                           # alpha before null
    c(10, "null pointer", result=None, out_bytes=0)                                    # null before out_bytes
    c(14, "out_bytes <", out_bytes=0, state_bytes=0)                                   # out_bytes before state_bytes
    c(14, "state_bytes <", state_bytes=0, result_bytes=0)                              # state_bytes before result_bytes
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_ci_tests_group", "dvs_mmpc_update"}
    run(lib, cases)
