"""TEST HELPER: cases, references and the checks themselves for constraint-based structure learning (csrc/dvs_citest.h:
dvs_ci_tests, dvs_pc_expand, dvs_pc_reduce, dvs_pc_orient; dags_vae_search_amd/pc.py), written once and run by
tests/test_emu_pc.py (emulator build) and tests/test_gpu_pc.py (device) on the back ends of tests/scoring_corpus.py.

References (numpy, mpmath and plain Python, nothing shared with the kernels)
  ci_reference    the statistics of include/dvs.h (dvs_ci_tests) cell by cell in mpmath at 50 digits, the two df as integers.
  gamma_q         mpmath's regularised upper incomplete gamma function.
  ref_level       the tests of a PC-stable level from itertools.combinations sorted by mask.
  reduce_ref      the decisions of dvs_pc_reduce, test by test.
  orient_ref      section 3 of the definitions: colliders, conflicts, Meek's rules, the cycle flag.
  pc_ref          the whole algorithm, driven either by a d-separation oracle (dsep) or by data (numpy counts, p by gamma_q).

Tolerances
  statistic   fp64 on the device.  A workgroup thread adds at most 36 864 / 256 = 144 cell terms, each a few roundings, then a
              tree of 8 levels: the error is below (144 + 12) * 2^-53 * T <= 2e-14 * T, with T = sum |term| + sum (n_xyz + e):
              the second sum covers the rounding of the ratio inside the logarithm (absolute 2^-53 in log r, times n_xyz) and of
              e inside (n_xyz - e)^2 / e (absolute 2^-52 e in the difference), which do not shrink with the term.  Asserted:
              |got - ref| <= CI_RTOL * T with CI_RTOL = 1e-12, as tests/scoring_corpus.py does for the scores.
  df          equal to the integer reference.
  p-value     compared with gamma_q at the device's own statistic and df, so that the statistic's error stays out of it.
              P_RTOL_EMU is the largest relative error measured on the emulator build over this corpus (the data cases of every
              type and sample count, df from 0 to 32 400); the device's log / exp / lgamma differ from libm by a few ulp and
              lgamma's absolute error scales with its argument, so the device is allowed P_RTOL = 4 * P_RTOL_EMU.  Both builds
              assert P_RTOL and print what they measure.  A p-value below the smallest normal fp64 number cannot carry a
              relative error: 2^-1022 is allowed on top, absolutely.
  guard       pc_ref on data records how close any p-value it evaluates comes to alpha, relative to alpha; the end-to-end
              cases assert that distance > 100 * P_RTOL.  Otherwise the decision would not be defined by the data.
"""
import functools
import itertools
import math
from collections import namedtuple
from types import SimpleNamespace

import mpmath
import numpy as np

from tests import cpdag_corpus as cp
from tests import scoring_corpus as sc
from tests.abi_cases import at, call, call_rc, entry, run

U64 = np.uint64
MAX_CELLS = 36864
CI_RTOL = 1e-12
P_RTOL_EMU = 1.5e-12         # measured on the emulator build over CI_CASE_NAMES x TYPES: 1.457e-12 (largedf, df = 3600)
P_RTOL = 4 * P_RTOL_EMU
P_FLOOR = 2.0 ** -1022
GUARD_FACTOR = 100
TYPES = ("mi", "x2", "mi-adf", "x2-adf")
TYPE_ID = {"mi": 0, "x2": 1, "mi-adf": 2, "x2-adf": 3}
mpmath.mp.dps = 50


def mask_of(zs):
    m = 0
    for z in zs:
        m |= 1 << int(z)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# 1. CI tests: reference
# ---------------------------------------------------------------------------------------------------------------------
def ci_table(data, card, x, y, zs):
    """int64 [q, r_x, r_y] counts, configuration index mixed radix with the lowest variable id fastest"""
    zs = sorted(int(z) for z in zs)
    key = np.zeros(len(data), np.int64)
    q = 1
    for z in zs:
        key += data[:, z].astype(np.int64) * q
        q *= int(card[z])
    rx, ry = int(card[x]), int(card[y])
    flat = (key * rx + data[:, x]) * ry + data[:, y]
    return np.bincount(flat, minlength=q * rx * ry).reshape(q, rx, ry)


@functools.lru_cache(maxsize=None)
def _ci_reference(case_name, x, y, zs):
    case = ci_case(case_name)
    tab = ci_table(case.data, case.card, x, y, zs)
    q, rx, ry = tab.shape
    mp = mpmath.mpf
    g2 = x2 = t_g2 = t_x2 = mp(0)
    adf = 0
    for j in np.nonzero(tab.sum((1, 2)))[0]:
        plane = tab[j]
        nx, ny, nz = plane.sum(1), plane.sum(0), int(plane.sum())
        adf += max(int((nx > 0).sum()) - 1, 0) * max(int((ny > 0).sum()) - 1, 0)
        for i in np.nonzero(nx)[0]:
            for k in np.nonzero(ny)[0]:
                c = int(plane[i, k])
                e = mp(int(nx[i])) * int(ny[k]) / nz
                term = (c - e) ** 2 / e
                x2 += term
                t_x2 += term + c + e
                if c:
                    term = c * mpmath.log(mp(c) * nz / (int(nx[i]) * int(ny[k])))
                    g2 += term
                    t_g2 += abs(term) + c
    return SimpleNamespace(g2=2 * g2, x2=x2, t_g2=float(2 * t_g2), t_x2=float(t_x2), df=(rx - 1) * (ry - 1) * q, adf=adf)


def ci_reference(case_name, x, y, zs, typ):
    """(statistic as mpf, df, T)"""
    r = _ci_reference(case_name, int(x), int(y), tuple(sorted(int(z) for z in zs)))
    stat, T = (r.g2, r.t_g2) if typ.startswith("mi") else (r.x2, r.t_x2)
    return max(stat, mpmath.mpf(0)), (r.adf if typ.endswith("adf") else r.df), T


def gamma_q(df, stat):
    if df == 0:
        return mpmath.mpf(1)
    return mpmath.gammainc(mpmath.mpf(df) / 2, mpmath.mpf(stat) / 2, mpmath.inf, regularized=True)


# ---------------------------------------------------------------------------------------------------------------------
# 1. CI tests: cases.  tests: (x, y, conditioning variables); refused: indices of tests that must come back NaN
# ---------------------------------------------------------------------------------------------------------------------
CiCase = namedtuple("CiCase", "name data card tests refused max_cells")
SIX_CARDS = [3, 4, 16, 2, 1, 16]             # variable 1 never takes its top level; variable 4 is constant
SIX_TESTS = [(0, 1, ()), (1, 0, ()), (0, 3, (1,)), (2, 5, ()), (2, 5, (0,)), (0, 1, (2, 3)), (3, 0, (1, 2, 5)),
             (0, 2, (1, 3, 4)), (4, 0, ()), (4, 0, (1,)), (0, 5, (1, 3)), (1, 3, (0,)), (5, 1, (3, 0, 4))]
SIX_BAD = [(2, 2, ()), (0, 1, (0,)), (0, 1, (3, 1)), (6, 0, ()), (0, -1, ()), (0, 1, (6,)), (0, 1, (63,))]
SAMPLE_COUNTS = (1, 37, 256, 257, 1000)      # 256 and 257: either side of one pass of the workgroup over the samples
CI_CASE_NAMES = tuple(f"sixS{s}" for s in SAMPLE_COUNTS) + ("boundary", "largedf")


def cells_of(card, x, y, zs):
    c = int(card[x]) * int(card[y])
    for z in zs:
        c *= int(card[z])
    return c


@functools.lru_cache(maxsize=None)
def _six():
    return sc.synthetic_dataset(6, 1000, SIX_CARDS, seed=181, drop_top=(1,))


@functools.lru_cache(maxsize=None)
def ci_case(name):
    if name.startswith("sixS"):
        data, card = _six()
        S = int(name[4:])
        tests = SIX_TESTS + SIX_BAD
        return CiCase(name, data[:S], card, tests, frozenset(range(len(SIX_TESTS), len(tests))), MAX_CELLS)
    if name == "boundary":
        # exactly 36 864 cells (16 * 16 * 16 * 9) and the nearest table size above it that level counts 1 .. 16 can reach
        above = sc.level_factors(sc.smooth_neighbours(MAX_CELLS)[1])
        cards = [16, 16, 16, 3, 3] + above
        data, card = sc.synthetic_dataset(len(cards), 1000, cards, seed=182)
        exact, over = (0, 1, (2, 3, 4)), (5, 6, tuple(range(7, len(cards))))
        assert cells_of(card, *exact) == MAX_CELLS < cells_of(card, *over) < MAX_CELLS + 1024
        return CiCase(name, data, card, [exact, over, (3, 4, (0,))], frozenset([1]), MAX_CELLS)
    if name == "largedf":
        # independent uniform columns, 20 000 samples over 4096 cells: the statistic is near df = 3600 and p mid-range
        rng = np.random.default_rng(183)
        data = rng.integers(0, 16, (20000, 3)).astype(np.uint8)
        return CiCase(name, data, np.array([16, 16, 16], np.uint8), [(0, 1, (2,)), (1, 2, (0,)), (0, 2, ())], frozenset(), 4096)
    raise KeyError(name)


def run_ci(be, data_h, card_h, n, S, tests, typ, max_cells):
    """one dvs_ci_tests on device handles of the data -> (rc, out [T, 3], status)"""
    T = len(tests)
    pairs = np.array([[x, y] for x, y, _ in tests], np.int32)
    cond = np.array([mask_of(zs) for _, _, zs in tests], U64)
    h = dict(pairs=be.put(pairs), cond=be.put(cond), out=be.put(np.full((T, 3), -7.0)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_ci_tests", n_tests=T, n_vars=n, n_samples=S, data=data_h, card=card_h, test_type=TYPE_ID[typ],
                 max_cells=max_cells, out_bytes=T * 24, **h)
    return rc, be.get(h["out"]).copy(), int(be.get(h["status"])[0])


def p_error(got_p, df, stat):
    """|got - Q(df / 2, stat / 2)| relative to the reference, after the absolute floor"""
    ref = gamma_q(int(df), float(stat))
    err = abs(mpmath.mpf(float(got_p)) - ref)
    return float(max(err - P_FLOOR, 0) / ref) if ref > 0 else float(err)


def check_ci_case(be, name, typ):
    """statistic, df and p-value of every test of one case for one type; returns the worst relative p error"""
    case = ci_case(name)
    S, n = case.data.shape
    dh, ch = be.put(sc.pack(case.data)), be.put(case.card)
    rc, out, status = run_ci(be, dh, ch, n, S, case.tests, typ, case.max_cells)
    assert rc == 0 and status == (16 if case.refused else 0), (name, typ, rc, status)
    worst = 0.0
    saw = set()
    for t, (x, y, zs) in enumerate(case.tests):
        if t in case.refused:
            assert np.isnan(out[t]).all(), (name, typ, t, out[t])
            continue
        stat, df, T = ci_reference(name, x, y, zs, typ)
        assert out[t, 1] == df, (name, typ, t, out[t, 1], df)
        err = abs(mpmath.mpf(float(out[t, 0])) - stat)
        print(f"{name} {typ} test {t}: stat {out[t, 0]!r} df {df} p {out[t, 2]!r} stat err / T {float(err) / max(T, 1e-300):.2e}")
        assert out[t, 0] >= 0.0 and err <= CI_RTOL * T, (name, typ, t, out[t, 0], float(stat), float(err), T)
        pe = p_error(out[t, 2], df, out[t, 0])
        assert 0.0 <= out[t, 2] <= 1.0 and pe <= P_RTOL, (name, typ, t, out[t].tolist(), pe)
        worst = max(worst, pe)
        classic = ci_reference(name, x, y, zs, typ[:2])[1]
        saw |= {"df0"} if df == 0 else set()
        saw |= {"adf<df"} if typ.endswith("adf") and 0 < df < classic else set()
        if df == 0:
            assert out[t, 2] == 1.0
    if name == "sixS1000":
        assert "df0" in saw and (not typ.endswith("adf") or "adf<df" in saw), (typ, saw)
    rc, again, status2 = run_ci(be, dh, ch, n, S, case.tests, typ, case.max_cells)
    assert rc == 0 and again.tobytes() == out.tobytes() and status2 == status                 # two runs give equal bytes
    print(f"{name} {typ}: worst relative p error {worst:.3e} (allowed {P_RTOL:.1e})")
    return worst


def check_ci_max_cells(be):
    """max_cells below a table's size refuses that test alone; at the size it is evaluated, to the same bytes as with room"""
    case = ci_case("sixS257")
    S, n = case.data.shape
    dh, ch = be.put(sc.pack(case.data)), be.put(case.card)
    tests = [(2, 5, (0,)), (0, 1, ()), (0, 3, (1,))]                  # 768, 12 and 24 cells
    _, roomy, st = run_ci(be, dh, ch, n, S, tests, "mi", MAX_CELLS)
    assert st == 0 and not np.isnan(roomy).any()
    _, tight, st = run_ci(be, dh, ch, n, S, tests, "mi", 768)
    assert st == 0 and tight.tobytes() == roomy.tobytes()
    _, small, st = run_ci(be, dh, ch, n, S, tests, "mi", 767)
    assert st == 16 and np.isnan(small[0]).all() and small[1:].tobytes() == roomy[1:].tobytes()
    _, small, st = run_ci(be, dh, ch, n, S, tests, "x2-adf", 12)
    assert st == 16 and np.isnan(small[[0, 2]]).all() and not np.isnan(small[1]).any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. Expand and reduce
# ---------------------------------------------------------------------------------------------------------------------
def ref_level(adj, level, every_pair=False):
    """(pair_xy, offsets, tests [(x, y, mask)]) of one level.  every_pair: list the adjacent pairs without tests too."""
    n = len(adj)
    pair_xy, offsets, tests = [], [0], []
    for x, y in itertools.combinations(range(n), 2):
        if not (adj[x] >> y) & 1:
            continue
        mine = []
        for a, b in (((x, y), (y, x)) if level else ((x, y),)):
            cand = [u for u in cp.bits(adj[a] & ~(1 << b))]
            mine += sorted(mask_of(s) for s in itertools.combinations(cand, level))
        if mine or every_pair:
            pair_xy.append([x, y])
            tests += [(x, y, m) for m in mine]
            offsets.append(len(tests))
    return pair_xy, offsets, tests


def random_adjacency(n, degree, seed):
    rng = np.random.default_rng(seed)
    adj = [0] * n
    for x, y in itertools.combinations(range(n), 2):
        if rng.random() < degree / (n - 1):
            adj[x] |= 1 << y
            adj[y] |= 1 << x
    return adj


def run_expand(be, adj, level, pair_xy, offsets):
    T, P, n = offsets[-1], len(pair_xy), len(adj)
    h = dict(adj=be.put(np.array(adj, U64)), pair_xy=be.put(np.array(pair_xy, np.int32)), offsets=be.put(np.array(offsets, np.int64)),
             pairs=be.put(np.full((T, 2), -7, np.int32)), cond=be.put(np.full(T, 0xA5A5A5A5A5A5A5A5, U64)))
    call(be, "dvs_pc_expand", n_pairs=P, n_vars=n, level=level, n_tests=T, tests_bytes=T * 8, **h)
    return be.get(h["pairs"]).copy(), be.get(h["cond"]).copy()


def check_expand(be):
    """equal bytes against itertools.combinations sorted by mask: n = 48 with neighbours up to bit 47, levels 0 .. 4, a pair
    with one empty side, pairs without tests in the list"""
    n = 48
    adj = random_adjacency(n, 6.0, seed=191)
    for u in (40, 43, 45, 46, 47):                                  # vertex 0 sees the top bits; 47 sees many
        for a, b in ((0, u), (47, u - 20)):
            adj[a] |= 1 << b
            adj[b] |= 1 << a
    for v, keep in ((1, (2,)), (2, (1, 3, 4))):                     # 1 - 2 only: side 1 is empty from level 1 on, and
        for u in range(n):                                          # 2 - {1, 3, 4}: the pair has no test from level 3 on
            adj[u] &= ~(1 << v)
        adj[v] = mask_of(keep)
        for u in keep:
            adj[u] |= 1 << v
    total = 0
    for level in range(5):
        pair_xy, offsets, tests = ref_level(adj, level, every_pair=True)
        assert [1, 2] in pair_xy and (level == 0 or len(set(np.diff(offsets))) > 2) and (level < 3 or 0 in np.diff(offsets))
        pairs, cond = run_expand(be, adj, level, pair_xy, offsets)
        assert pairs.tobytes() == np.array([[x, y] for x, y, _ in tests], np.int32).tobytes(), level
        assert cond.tobytes() == np.array([m for _, _, m in tests], U64).tobytes(), level
        assert level == 0 or int(cond.max()) >> 47
        total += len(tests)
    # offsets that promise a pair more tests than its rows have: the surplus comes back as (-1, -1), which dvs_ci_tests refuses
    pair_xy, offsets, tests = ref_level(adj, 2)
    pairs, cond = run_expand(be, adj, 2, pair_xy, offsets[:-1] + [offsets[-1] + 3])
    assert (pairs[-3:] == -1).all() and not cond[-3:].any() and pairs[:-3].tobytes() == np.array([t[:2] for t in tests], np.int32).tobytes()
    return total


def reduce_ref(n, adj, pair_xy, offsets, cond, p, alpha, sepset):
    """-> (adj_next, sepset, result [P, 2], refused)"""
    adj, sepset = list(adj), sepset.copy()
    result = np.zeros((len(pair_xy), 2), np.int64)
    for k, (x, y) in enumerate(pair_xy):
        idx = [t for t in range(offsets[k], offsets[k + 1]) if p[t] > alpha]          # NaN > alpha is False
        result[k] = (idx[0] if idx else -1, sum(1 for t in range(offsets[k], offsets[k + 1]) if math.isnan(p[t])))
        if idx:
            adj[x] &= ~(1 << y)
            adj[y] &= ~(1 << x)
            sepset[x, y] = sepset[y, x] = cond[idx[0]]
    return adj, sepset, result, int(result[:, 1].sum())


def run_reduce(be, n, adj, pair_xy, offsets, cond, out, alpha, sepset):
    P, T = len(pair_xy), offsets[-1]
    h = dict(pair_xy=be.put(np.array(pair_xy, np.int32)), offsets=be.put(np.array(offsets, np.int64)), cond=be.put(np.array(cond, U64)),
             out=be.put(np.ascontiguousarray(out, np.float64)), adj=be.put(np.array(adj, U64)), sepset=be.put(sepset.copy()),
             adj_next=be.put(np.full(n, 0xA5A5A5A5A5A5A5A5, U64)), result=be.put(np.full((P, 2), -7, np.int64)),
             refused=be.put(np.full(1, -7, np.int32)))
    call(be, "dvs_pc_reduce", n_pairs=P, n_vars=n, n_tests=T, alpha=alpha, sepset_bytes=n * n * 8, result_bytes=P * 16, **h)
    g = lambda k: be.get(h[k]).copy()
    return [int(v) for v in g("adj_next")], g("sepset"), g("result"), int(g("refused")[0])


def check_reduce(be):
    """hand-made p arrays: ties with alpha, NaNs, several passing tests, none, a pair of 200 tests whose first passing test is
    in the wave's third pass; seeded arrays on a larger graph"""
    nan, alpha = float("nan"), 0.05
    n = 6
    adj = [0b111110, 0b111101, 0b111011, 0b110111, 0b101111, 0b011111]
    pair_xy = [[0, 1], [0, 2], [1, 2], [2, 3], [3, 4], [4, 5], [0, 5]]
    ps = [[0.01, 0.05, 0.04],                      # a tie with alpha does not pass
          [0.01, 0.2, 0.9, 0.06],                  # several pass: the lowest index wins
          [nan, nan],                              # refused only
          [nan, 0.5, nan, 0.7],                    # NaN before the passing test
          [0.0499999],
          [0.0] * 150 + [nan, 0.050000001] + [1.0] * 48,
          [1.0]]
    offsets = [0] + list(np.cumsum([len(x) for x in ps]))
    p = np.array([v for x in ps for v in x])
    T = len(p)
    cond = [(0x1234567 * (t + 3)) & 0x3F for t in range(T)]
    out = np.stack([np.full(T, 3.5), np.full(T, 2.0), p], 1)
    sep0 = np.arange(n * n, dtype=U64).reshape(n, n) + U64(1000)
    want = reduce_ref(n, adj, pair_xy, [int(o) for o in offsets], cond, p, alpha, sep0)
    assert [r[0] >= 0 for r in want[2]] == [False, True, False, True, False, True, True] and want[3] == 5
    got = run_reduce(be, n, adj, pair_xy, [int(o) for o in offsets], cond, out, alpha, sep0)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]
    n = 33
    adj = random_adjacency(n, 5.0, seed=192)
    pair_xy, offsets, tests = ref_level(adj, 2, every_pair=True)
    rng = np.random.default_rng(193)
    p = rng.choice([0.0, 0.01, 0.05, 0.050001, 0.3, nan], len(tests), p=[0.5, 0.3, 0.05, 0.05, 0.05, 0.05])
    out = np.stack([rng.random(len(tests)), np.ones(len(tests)), p], 1)
    cond = [m for _, _, m in tests]
    sep0 = np.zeros((n, n), U64)
    want = reduce_ref(n, adj, pair_xy, offsets, cond, p, alpha, sep0)
    got = run_reduce(be, n, adj, pair_xy, offsets, cond, out, alpha, sep0)
    assert 0 < (want[2][:, 0] >= 0).sum() < len(pair_xy) and want[3] > 0
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes() and got[3] == want[3]


# ---------------------------------------------------------------------------------------------------------------------
# 3. The algorithm restated: skeleton by levels, orientation
# ---------------------------------------------------------------------------------------------------------------------
def meek_ref(adj, D):
    """Meek's R1 - R3 from directed-in rows D on the skeleton adj, a round's orientations applied together -> (D, U)"""
    n = len(adj)
    D = list(D)
    Dout = cp.children_rows(D)
    U = [adj[v] & ~D[v] & ~Dout[v] for v in range(n)]
    for _ in range(n * (n - 1) // 2 + 1):
        O = [0] * n
        for v in range(n):
            for u in cp.bits(U[v]):
                S = U[u] & D[v]
                if (D[u] & ~adj[v] & ~(1 << v)) or (Dout[u] & D[v]) or any(S & ~adj[w] & ~(1 << w) for w in cp.bits(S)):
                    O[v] |= 1 << u
        if not any(O):
            break
        for v in range(n):
            D[v] |= O[v]
            U[v] &= ~O[v]
            for u in cp.bits(O[v]):
                U[u] &= ~(1 << v)
        Dout = cp.children_rows(D)
    return D, U


def orient_ref(adj, sepset):
    """(pdag rows, conflicts, flag) of dvs_pc_orient for legal rows"""
    n = len(adj)
    C = [0] * n
    for z in range(n):
        for x, y in itertools.combinations(list(cp.bits(adj[z])), 2):
            if not (adj[x] >> y) & 1 and not (int(sepset[x][y]) >> z) & 1:
                C[z] |= (1 << x) | (1 << y)
    Cout = cp.children_rows(C)
    both = [C[v] & Cout[v] for v in range(n)]
    conflicts = sum(bin(b).count("1") for b in both) // 2
    D, U = meek_ref(adj, [C[v] & ~both[v] for v in range(n)])
    return [D[v] | U[v] for v in range(n)], conflicts, 1 if cp.flags_ref(D) == 1 else 0


def pc_ref(n, independent, alpha_guard=None, max_cond=None):
    """PC-stable with `independent(x, y, mask) -> bool` deciding every test -> namespace(adj, sepset, tests_per_level)"""
    adj = [((1 << n) - 1) & ~(1 << v) for v in range(n)]
    sepset = np.zeros((n, n), U64)
    per_level = []
    level = 0
    while max_cond is None or level <= max_cond:
        pair_xy, offsets, tests = ref_level(adj, level)
        if not tests:
            break
        nxt = list(adj)
        verdict = [independent(x, y, m) for x, y, m in tests]        # no early exit within a level
        for k, (x, y) in enumerate(pair_xy):
            hit = [t for t in range(offsets[k], offsets[k + 1]) if verdict[t]]
            if hit:
                nxt[x] &= ~(1 << y)
                nxt[y] &= ~(1 << x)
                sepset[x, y] = sepset[y, x] = tests[hit[0]][2]
        adj = nxt
        per_level.append(len(tests))
        level += 1
    return SimpleNamespace(adj=adj, sepset=sepset, tests_per_level=per_level)


def dsep_oracle(P):
    """exact d-separation in the DAG with parent rows P: x and y are separated by Z iff Z cuts them in the moral graph of
    the ancestral set of {x, y} and Z"""
    n = len(P)
    anc = [P[v] | (1 << v) for v in range(n)]
    for k in range(n):
        for v in range(n):
            if (anc[v] >> k) & 1:
                anc[v] |= anc[k]

    moral = {}

    def independent(x, y, zmask):
        if ((P[x] >> y) | (P[y] >> x)) & 1:                         # adjacent vertices are never separated
            return False
        A = anc[x] | anc[y]
        for z in cp.bits(zmask):
            A |= anc[z]
        nb = moral.get(A)
        if nb is None:
            nb = moral[A] = [0] * n
            for c in cp.bits(A):
                for u in cp.bits(P[c]):
                    nb[u] |= (P[c] | (1 << c)) & ~(1 << u)
                    nb[c] |= 1 << u
        seen, frontier = 1 << x, 1 << x
        while frontier:
            new = 0
            for v in cp.bits(frontier):
                new |= nb[v]
            frontier = new & ~seen & ~zmask
            seen |= frontier
        return not (seen >> y) & 1
    return independent


@functools.lru_cache(maxsize=None)
def oracle_pc(n):
    """[(adj, sepset)] over cp.all_dags(n).  d-separation depends on a DAG through its Markov equivalence class alone (Verma
    and Pearl), which cp.class_key names: the restatement runs once per class."""
    memo, out = {}, []
    for P in cp.all_dags(n):
        key = cp.class_key(P)
        if key not in memo:
            r = pc_ref(n, dsep_oracle(P))
            memo[key] = (r.adj, r.sepset)
        out.append(memo[key])
    assert len(memo) == cp.CLASS_COUNTS[n]
    return out


def run_orient(be, skel, sepsets):
    skel, sepsets = np.ascontiguousarray(skel, U64), np.ascontiguousarray(sepsets, U64)
    B, n = skel.shape
    h = dict(skeleton=be.put(skel), sepsets=be.put(sepsets), pdag=be.put(np.full((B, n), 0xA5A5A5A5A5A5A5A5, U64)),
             conflicts=be.put(np.full(B, -7, np.int32)), flags=be.put(np.full(B, -7, np.int32)))
    call(be, "dvs_pc_orient", batch=B, n_vars=n, sepsets_bytes=B * n * n * 8, pdag_bytes=B * n * 8, **h)
    return be.get(h["pdag"]).copy(), be.get(h["conflicts"]).copy(), be.get(h["flags"]).copy()


def check_orient_all_dags(be, n):
    """every labelled DAG on n vertices in one launch: the skeleton and separating sets that PC-stable finds with an exact
    d-separation oracle give, through dvs_pc_orient, the bytes dvs_cpdag gives for the DAG itself"""
    dags, found = cp.all_dags(n), oracle_pc(n)
    P = cp.as_rows(dags)
    skel = np.array([f[0] for f in found], U64)
    assert all(int(skel[b, v]) == int(P[b, v]) | cp.children_rows(dags[b])[v] for b in range(0, len(dags), 97) for v in range(n))
    pdag, conf, fl = run_orient(be, skel, np.stack([f[1] for f in found]))
    want, wfl = cp.Driver(be).cpdag(P)
    assert not fl.any() and not conf.any() and not wfl.any()
    bad = np.nonzero((pdag != want).any(1))[0]
    assert pdag.tobytes() == want.tobytes(), (n, len(bad), [(P[b].tolist(), pdag[b].tolist(), want[b].tolist()) for b in bad[:3]])
    return len(dags)


def check_orient_hand(be):
    """conflicting colliders, a directed cycle made of collider claims, illegal rows, against orient_ref"""
    full = (1 << 48) - 1
    rows = []
    # a - b - c - d with colliders at b and at c: b - c is claimed both ways and stays undirected
    n = 8
    adj = [0] * n
    for u, v in ((0, 1), (1, 2), (2, 3)):
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    sep = np.full((n, n), full, U64)
    sep[0, 2] = sep[2, 0] = 0
    sep[1, 3] = sep[3, 1] = 0
    rows.append((adj, sep, 1, 1))        # R1 then fires on b - c from both ends in one round: a 2-cycle in the directed part
    # the square 0 - 1 - 2 - 3 - 0 with a pendant at every corner: the collider at corner k + 1 with its pendant claims
    # k -> k + 1, and the four claims close a directed cycle
    adj = [0] * n
    for k in range(4):
        for u, v in ((k, (k + 1) % 4), (k, 4 + k)):
            adj[u] |= 1 << v
            adj[v] |= 1 << u
    sep = np.full((n, n), full, U64)
    for k in range(4):
        a, c = k, 4 + (k + 1) % 4                                   # corner k and the pendant of corner k + 1
        sep[a, c] = sep[c, a] = 0
    rows.append((adj, sep, 0, 1))
    # a plain collider next to them, and Meek R1 behind it: 0 -> 2 <- 1, 2 - 3 becomes 2 -> 3
    adj = [0] * n
    for u, v in ((0, 2), (1, 2), (2, 3)):
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    sep = np.full((n, n), full, U64)
    sep[0, 1] = sep[1, 0] = 0
    rows.append((adj, sep, 0, 0))
    skel = np.array([r[0] for r in rows], U64)
    seps = np.stack([r[1] for r in rows])
    pdag, conf, fl = run_orient(be, skel, seps)
    for b, (adj, sep, conflicts, flag) in enumerate(rows):
        want = orient_ref(adj, sep)
        assert want[1:] == (conflicts, flag), (b, want)
        assert [int(v) for v in pdag[b]] == want[0] and (int(conf[b]), int(fl[b])) == (conflicts, flag), (b, pdag[b].tolist(), want)
    assert [int(v) for v in pdag[2]] == [0, 0, 0b011, 0b100, 0, 0, 0, 0]
    # illegal rows between clean ones: asymmetric, a bit >= n, a self-loop
    bad = np.repeat(skel[2:3], 5, 0)
    bad[1, 0] |= U64(1 << 5)
    bad[2, 7] |= U64(1) << U64(n)
    bad[3, 4] |= U64(1 << 4)
    pdag2, conf2, fl2 = run_orient(be, bad, np.repeat(seps[2:3], 5, 0))
    assert fl2.tolist() == [0, 2, 2, 2, 0] and not conf2.any() and not pdag2[1:4].any()
    assert pdag2[0].tobytes() == pdag[2].tobytes() == pdag2[4].tobytes()


# ---------------------------------------------------------------------------------------------------------------------
# 4. End to end on data
# ---------------------------------------------------------------------------------------------------------------------
E2E_CASES = tuple((name, S, typ) for name in ("asia", "sachs") for S in (5000, 1000) for typ in ("mi", "x2"))
EMU_E2E_CASES = tuple(c for c in E2E_CASES if c[0] == "asia") + (("sachs", 5000, "mi"),)
ALPHA = 0.05


@functools.lru_cache(maxsize=None)
def e2e_data(name, S):
    from tests.helpers import load_npz
    data = load_npz(f"bn_{name}_data.npz")["data"].astype(np.uint8)[:S]
    assert len(data) == S
    return data, (data.max(0) + 1).astype(np.uint8)


def data_test(data, card, x, y, zmask, typ):
    """(statistic, df, p) in fp64 numpy, p by gamma_q at 50 digits"""
    tab = ci_table(data, card, x, y, list(cp.bits(zmask))).astype(np.float64)
    nz, nx, ny = tab.sum((1, 2), keepdims=True), tab.sum(2, keepdims=True), tab.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = nx * ny / nz
        if typ.startswith("mi"):
            stat = 2.0 * float(np.where(tab > 0, tab * np.log(tab * nz / (nx * ny)), 0.0).sum())
        else:
            stat = float(np.where(e > 0, (tab - e) ** 2 / e, 0.0).sum())
    df = (tab.shape[1] - 1) * (tab.shape[2] - 1) * tab.shape[0]
    if typ.endswith("adf"):
        df = int((np.maximum((nx > 0).sum(1).ravel() - 1, 0) * np.maximum((ny > 0).sum(2).ravel() - 1, 0)).sum())
    stat = max(stat, 0.0)
    return stat, df, float(gamma_q(df, stat))


@functools.lru_cache(maxsize=None)
def e2e_reference(name, S, typ):
    """pc_ref on the data, its orientation, and the guard: the smallest |p - alpha| / alpha over every test evaluated"""
    data, card = e2e_data(name, S)
    closest = [float("inf")]

    def independent(x, y, zmask):
        p = data_test(data, card, x, y, zmask, typ)[2]
        closest[0] = min(closest[0], abs(p - ALPHA) / ALPHA)
        return p > ALPHA
    r = pc_ref(data.shape[1], independent)
    r.pdag, r.conflicts, r.flag = orient_ref(r.adj, r.sepset)
    r.closest = closest[0]
    return r


def pc_raw(be, data, card, typ, alpha=ALPHA, max_cond=None, chunk=65536):
    """PC-stable through the raw C ABI on a back end: the launch sequence of dags_vae_search_amd/pc.py"""
    S, n = data.shape
    dh, ch = be.put(sc.pack(data)), be.put(card)
    adj = [((1 << n) - 1) & ~(1 << v) for v in range(n)]
    hsep = be.put(np.zeros((n, n), U64))
    status, refused = be.put(np.zeros(1, np.int32)), be.put(np.zeros(1, np.int32))
    per_level, refused_total, level = [], 0, 0
    top = sorted((int(c) for c in card), reverse=True)
    while max_cond is None or level <= max_cond:
        pair_xy, offsets, _ = ref_level(adj, level)
        T, P = offsets[-1], len(pair_xy)
        if T == 0:
            break
        max_cells = max(1, min(int(np.prod(top[:level + 2])), MAX_CELLS))
        ha, hn = be.put(np.array(adj, U64)), be.put(np.zeros(n, U64))
        hx, ho = be.put(np.array(pair_xy, np.int32)), be.put(np.array(offsets, np.int64))
        pairs, cond, out = be.put(np.zeros((T, 2), np.int32)), be.put(np.zeros(T, U64)), be.put(np.zeros((T, 3)))
        res = be.put(np.zeros((P, 2), np.int64))
        call(be, "dvs_pc_expand", n_pairs=P, n_vars=n, level=level, adj=ha, pair_xy=hx, offsets=ho, n_tests=T, pairs=pairs,
             cond=cond, tests_bytes=T * 8)
        for t0 in range(0, T, chunk):
            m = min(chunk, T - t0)
            call(be, "dvs_ci_tests", n_tests=m, n_vars=n, n_samples=S, data=dh, card=ch, pairs=at(be, pairs, t0 * 8),
                 cond=at(be, cond, t0 * 8), test_type=TYPE_ID[typ], max_cells=max_cells, out=at(be, out, t0 * 24), out_bytes=m * 24,
                 status=status)
        call(be, "dvs_pc_reduce", n_pairs=P, n_vars=n, pair_xy=hx, offsets=ho, n_tests=T, cond=cond, out=out, alpha=alpha, adj=ha,
             adj_next=hn, sepset=hsep, sepset_bytes=n * n * 8, result=res, result_bytes=P * 16, refused=refused)
        adj = [int(v) for v in be.get(hn)]
        refused_total += int(be.get(refused)[0])
        per_level.append(T)
        level += 1
    sepset = be.get(hsep).copy()
    pdag, conf, fl = run_orient(be, np.array([adj], U64), sepset[None])
    return SimpleNamespace(adj=adj, sepset=sepset, tests_per_level=per_level, refused=refused_total,
                           pdag=[int(v) for v in pdag[0]], conflicts=int(conf[0]), flag=int(fl[0]))


def assert_same_result(got, ref, what):
    assert got.tests_per_level == ref.tests_per_level, (what, got.tests_per_level, ref.tests_per_level)
    assert got.adj == ref.adj, (what, "skeleton")
    assert got.sepset.tobytes() == ref.sepset.tobytes(), (what, "sepsets")
    assert (got.pdag, got.conflicts, got.flag) == (ref.pdag, ref.conflicts, ref.flag), (what, "orientation")


def check_guard(name, S, typ):
    ref = e2e_reference(name, S, typ)
    print(f"{name} S {S} {typ}: tests {ref.tests_per_level}, edges {sum(bin(a).count('1') for a in ref.adj) // 2}, conflicts "
          f"{ref.conflicts}, closest |p - alpha| / alpha {ref.closest:.3e} (guard {GUARD_FACTOR * P_RTOL:.1e})")
    assert ref.closest > GUARD_FACTOR * P_RTOL, (name, S, typ, ref.closest)
    return ref


def check_e2e_raw(be, name, S, typ):
    ref = check_guard(name, S, typ)
    data, card = e2e_data(name, S)
    got = pc_raw(be, data, card, typ)
    assert got.refused == 0
    assert_same_result(got, ref, (name, S, typ))
    if (name, S, typ) == ("asia", 5000, "mi"):                     # ragged chunks, and a cap, give what they should
        small = pc_raw(be, data, card, typ, chunk=37)
        assert_same_result(small, ref, "chunk 37")
        capped = pc_raw(be, data, card, typ, max_cond=1)
        assert capped.tests_per_level == ref.tests_per_level[:2]
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 5. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []

    nan = float("nan")
    c = entry("dvs_ci_tests", cases, n_tests=8, n_vars=12, n_samples=100, data=D, card=D, pairs=D, cond=D, test_type=0,
              max_cells=729, out=D, out_bytes=192, status=D, stream=None)
    c(2, "n_tests and n_samples must be > 0", n_tests=0)
    c(2, "n_tests and n_samples must be > 0", n_samples=-1)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(12, "test_type is not a dvs_ci_type", test_type=4)
    c(12, "test_type is not a dvs_ci_type", test_type=-1)
    c(13, "max_cells must be in [1, 36864]", max_cells=0)
    c(13, "max_cells must be in [1, 36864]", max_cells=36865)
    for name in ("data", "card", "pairs", "cond", "out", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "out_bytes < n_tests * 24 = 192", out_bytes=191)
    c(2, "n_tests and n_samples must be > 0", n_tests=0, n_vars=49)                    # sizes before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, test_type=9)                          # n_vars before the type
    c(12, "test_type is not a dvs_ci_type", test_type=9, max_cells=0)                  # the type before max_cells
    c(13, "max_cells must be in [1, 36864]", max_cells=0, data=None)                   # max_cells before null
    c(10, "null pointer", status=None, out_bytes=0)                                    # null before out_bytes

    c = entry("dvs_pc_expand", cases, n_pairs=10, n_vars=12, level=2, adj=D, pair_xy=D, offsets=D, n_tests=300, pairs=D,
              cond=D, tests_bytes=2400, stream=None)
    c(2, "n_pairs must be in [1, 1128]", n_pairs=0)
    c(2, "n_pairs must be in [1, 1128]", n_pairs=1129)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_tests must be in [1, 2^31 - 1]", n_tests=0)
    c(2, "n_tests must be in [1, 2^31 - 1]", n_tests=1 << 31, tests_bytes=1 << 40)
    c(13, "level must be in [0, 46]", level=-1)
    c(13, "level must be in [0, 46]", level=47)
    for name in ("adj", "pair_xy", "offsets", "pairs", "cond"):
        c(10, "null pointer", **{name: None})
    c(14, "tests_bytes < n_tests * 8 = 2400", tests_bytes=2399)
    c(2, "n_pairs must be in [1, 1128]", n_pairs=0, n_vars=49)                         # n_pairs before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=0, n_tests=0)                             # n_vars before n_tests
    c(2, "n_tests must be in [1, 2^31 - 1]", n_tests=0, level=47)                      # n_tests before the level
    c(13, "level must be in [0, 46]", level=47, adj=None)                              # the level before null
    c(10, "null pointer", cond=None, tests_bytes=0)                                    # null before tests_bytes

    c = entry("dvs_pc_reduce", cases, n_pairs=10, n_vars=12, pair_xy=D, offsets=D, n_tests=300, cond=D, out=D, alpha=0.05,
              adj=D, adj_next=D, sepset=D, sepset_bytes=1152, result=D, result_bytes=160, refused=D, stream=None)
    c(2, "n_pairs must be in [1, 1128]", n_pairs=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_tests must be in [1, 2^31 - 1]", n_tests=0)
    c(13, "alpha must be in [0, 1]", alpha=nan)
    c(13, "alpha must be in [0, 1]", alpha=1.5)
    c(13, "alpha must be in [0, 1]", alpha=-0.1)
    for name in ("pair_xy", "offsets", "cond", "out", "adj", "adj_next", "sepset", "result", "refused"):
        c(10, "null pointer", **{name: None})
    c(14, "sepset_bytes < n_vars^2 * 8 = 1152", sepset_bytes=1151)
    c(14, "result_bytes < n_pairs * 16 = 160", result_bytes=159)
    c(2, "n_tests must be in [1, 2^31 - 1]", n_tests=0, alpha=nan)                     # n_tests before alpha
    c(13, "alpha must be in [0, 1]", alpha=2.0, pair_xy=None)                          # alpha before null
    c(10, "null pointer", refused=None, sepset_bytes=0)                                # null before sepset_bytes
    c(14, "sepset_bytes <", sepset_bytes=0, result_bytes=0)                            # sepset_bytes before result_bytes

    c = entry("dvs_pc_orient", cases, batch=8, n_vars=12, skeleton=D, sepsets=D, sepsets_bytes=9216, pdag=D, pdag_bytes=768,
              conflicts=D, flags=D, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48, sepsets_bytes=1 << 40, pdag_bytes=1 << 40)
    for name in ("skeleton", "sepsets", "pdag", "conflicts", "flags"):
        c(10, "null pointer", **{name: None})
    c(14, "sepsets_bytes < batch * n_vars^2 * 8 = 9216", sepsets_bytes=9215)
    c(14, "pdag_bytes < batch * n_vars * 8 = 768", pdag_bytes=767)
    c(2, "batch must be > 0", batch=0, n_vars=49)                                      # batch before n_vars
    c(3, "n_vars must be in [1, 48]", batch=1 << 30, n_vars=49)                        # n_vars before the product
    c(2, "batch * n_vars^2 must be < 2^31", batch=1 << 20, n_vars=48, skeleton=None)   # the product before null
    c(10, "null pointer", flags=None, sepsets_bytes=0)                                 # null before sepsets_bytes
    c(14, "sepsets_bytes <", sepsets_bytes=0, pdag_bytes=0)                            # sepsets_bytes before pdag_bytes
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_ci_tests", "dvs_pc_expand", "dvs_pc_reduce", "dvs_pc_orient"}
    run(lib, cases)
