"""TEST HELPER: cases, restatement and the checks themselves for the Monte Carlo permutation CI tests (csrc/dvs_permtest.h:
dvs_ci_perm_tests; include/dvs_permtest.h; dags_vae_search_amd/pc.py), written once and run by tests/test_permtest_ref.py (CPU
only), tests/test_emu_permtest.py (emulator build) and tests/test_gpu_permtest.py (device) on the back ends of
tests/scoring_corpus.py.  The data cases, mpmath's gamma_q and the tolerances P_RTOL / P_RTOL_EMU are those of tests/pc_corpus.py.

Restatement (numpy, nothing shared with the kernels)
  draws           include/dvs_permtest.h's counter-based draws in numpy u32 / u64, all permutations of a test at once.
  perm_reference  the tables of every permutation, V_b and V_obs in fp64 numpy, the exceed flags, the per-block counts and sums.
  exact_*         every table with the margins of a small test, enumerated; its probability under permutation (the multivariate
                  hypergeometric law) as a Fraction; "exceeds" decided exactly: prod c^c as integers for mi, Fractions for x2.

What is compared how
  decisions   a permutation exceeds when V_b >= V_obs (1 - 2^-32).  The device's log differs from numpy's by a few ulp and V is a
              sum in another machine's rounding, so each decision is first asserted to be guarded on the restatement:
              |V_b / V_obs - 1| is below 2^-36 (a tie, within the header's derived error of a mathematically equal statistic:
              exceeds on both sides) or above 2^-20 (decided, far beyond both errors).  The seeds below were chosen on the CPU so
              that this holds for every permutation of every case; nothing is skipped.  Then counts, masks, used and the mc / smc
              p-value (an exact quotient of integers) are compared as bytes.
  sp df       df = mean_b s_b with s_b = 2 (V_b - C) (mi) or V_b - S_counted (x2).  Device and restatement each carry a relative
              error below 2^-36 in V_b and in C (the header's bound), so |s_b - s_b'| <= 2 * 2^-36 * (V_b + C) * 2 for mi and
              2^-36 * V_b for x2: the cancellation shows as the ratio of V + C to their difference.  The mean of 256-blocks adds
              at most (8 + blocks) * 2^-53 relative to mean |s_b|.  Asserted: |df - df'| <= SP_EPS * mean_b (V_b + C) with
              SP_EPS = 2^-33, eight times what the bound gives for mi; a df clamped at 0 on one side must be within that of 0.
  sp p        against mpmath's gammainc at the device's own df and statistic, within pc_corpus's P_RTOL (emulator: P_RTOL_EMU).
"""
import functools
import itertools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from tests import cpdag_corpus as cp
from tests import pc_corpus as pc
from tests import scoring_corpus as sc
from tests.abi_cases import at, run
from tests.eliminate_corpus import call_rc, entry

U32, U64 = np.uint32, np.uint64
TYPES = ("mc-mi", "mc-x2", "smc-mi", "smc-x2", "sp-mi", "sp-x2")
TYPE_ID = {t: i for i, t in enumerate(TYPES)}
TIE, DECIDED = 2.0 ** -36, 2.0 ** -20
SLACK = 1.0 - 2.0 ** -32
SP_EPS = 2.0 ** -33
NAN3 = np.array([np.nan]).tobytes() * 3


# ---------------------------------------------------------------------------------------------------------------------
# 1. The restatement
# ---------------------------------------------------------------------------------------------------------------------
def fmix32(v):
    v = np.asarray(v, U32).copy()
    v ^= v >> U32(16)
    v *= U32(0x85EBCA6B)
    v ^= v >> U32(13)
    v *= U32(0xC2B2AE35)
    v ^= v >> U32(16)
    return v


def key_of_test(seed, gt):
    seed = int(seed) & (2 ** 64 - 1)
    lo, hi = U32(seed & 0xFFFFFFFF), U32(seed >> 32)
    with np.errstate(over="ignore"):
        k = fmix32(lo ^ U32((801 * 0x632BE5AB) & 0xFFFFFFFF))
        return fmix32(k ^ hi ^ U32(((int(gt) & 0xFFFFFFFF) * 0x9E3779B1) & 0xFFFFFFFF))


def draws(key_b, j, m):
    """u uniform on [0, m) for draw ordinal j of every permutation (key_b: u32 [B])"""
    with np.errstate(over="ignore"):
        h0 = fmix32(key_b ^ U32((j * 0x9E3779B1) & 0xFFFFFFFF))
        prod = h0.astype(U64) * U64(m)
        thr = (2 ** 32 - m) % m
        a = 1
        while True:
            again = (prod & U64(0xFFFFFFFF)) < U64(thr)
            if not again.any():
                return (prod >> U64(32)).astype(np.int64)
            h = fmix32(h0 ^ U32((a * 0x632BE5AB) & 0xFFFFFFFF))
            prod = np.where(again, h.astype(U64) * U64(m), prod)
            a += 1


def klnk(c):
    c = np.asarray(c, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(c > 1, c * np.log(c), 0.0)


def permuted_tables(tab, seed, gt, B):
    """int64 [B, q, rx, ry]: the table every permutation b of global test gt draws from the observed tab [q, rx, ry]"""
    q, rx, ry = tab.shape
    with np.errstate(over="ignore"):
        key_b = fmix32(key_of_test(seed, gt) ^ (np.arange(B, dtype=U32) * U32(0x9E3779B1)))
    out = np.zeros((B, q, rx, ry), np.int64)
    j = 0
    lanes = np.arange(B)
    for z in range(q):
        n_xz, m = tab[z].sum(1), int(tab[z].sum())
        if m == 0:
            continue
        pool = np.repeat(tab[z].sum(0)[None], B, 0)
        occupied = [i for i in range(rx) if n_xz[i]]
        for i in occupied[:-1]:
            for _ in range(int(n_xz[i])):
                u = draws(key_b, j, m)
                k = (np.cumsum(pool, 1) > u[:, None]).argmax(1)
                out[lanes, z, i, k] += 1
                pool[lanes, k] -= 1
                j += 1
                m -= 1
        out[:, z, occupied[-1]] = pool
    return out


def v_of(tabs, margins_of, g2):
    """V of tables [..., q, rx, ry] with the margins of `margins_of` [q, rx, ry], the sums in the header's order"""
    V = np.zeros(tabs.shape[:-3])
    q, rx, ry = margins_of.shape
    for z in range(q):
        n_xz, n_yz, n_z = margins_of[z].sum(1), margins_of[z].sum(0), int(margins_of[z].sum())
        if n_z == 0:
            continue
        if g2:
            for i in range(rx):
                if n_xz[i]:
                    for k in range(ry):
                        V = V + klnk(tabs[..., z, i, k])
        else:
            rows = np.zeros(tabs.shape[:-3])
            for i in range(rx):
                if n_xz[i]:
                    s = np.zeros(tabs.shape[:-3])
                    for k in range(ry):
                        if n_yz[k]:
                            c = tabs[..., z, i, k].astype(np.float64)
                            s = s + c * c / float(n_yz[k])
                    rows = rows + s / float(n_xz[i])
            V = V + float(n_z) * rows
    return V


def margin_of(tab, g2):
    """C (mi) or S_counted (x2) in the header's order"""
    M = 0.0
    for z in range(tab.shape[0]):
        n_z = int(tab[z].sum())
        if n_z == 0:
            continue
        if not g2:
            M += float(n_z)
            continue
        Mz = 0.0
        for c in tab[z].sum(0):
            Mz += float(klnk(c))
        for c in tab[z].sum(1):
            if c:
                Mz = float(klnk(c)) + Mz
        M += Mz - float(klnk(n_z))
    return M


def block_tree(x):
    """the dvs_block_sum256 tree over 256 slots"""
    x = np.array(x, np.float64)
    s = 128
    while s:
        x[:s] += x[s:2 * s]
        s >>= 1
    return float(x[0])


def perm_reference(tab, g2, B, seed, gt):
    """everything the kernels derive from one observed table, and the guard of every decision"""
    tabs = permuted_tables(tab, seed, gt, B)
    assert (tabs.sum(3) == tab.sum(2)).all() and (tabs.sum(2) == tab.sum(1)).all()             # the margins are kept
    V, v_obs = v_of(tabs, tab, g2), float(v_of(tab, tab, g2))
    if v_obs > 0.0:
        rel = np.abs(V / v_obs - 1.0)
        guarded = bool(((rel < TIE) | (rel > DECIDED)).all())
    else:
        guarded = True                                       # V_b >= 0 = V_obs: everything exceeds, on any machine
    exceed = V >= v_obs * SLACK
    M = margin_of(tab, g2)
    s = 2.0 * (V - M) if g2 else V - M
    blocks = (B + 255) // 256
    pad = np.zeros(blocks * 256)
    pad[:B] = s
    flags = np.zeros(blocks * 256, bool)
    flags[:B] = exceed
    sums = [block_tree(pad[j * 256:(j + 1) * 256]) for j in range(blocks)]
    masks = np.zeros((blocks, 4), U64)
    for j, w in itertools.product(range(blocks), range(4)):
        masks[j, w] = sum(1 << l for l in range(64) if flags[j * 256 + 64 * w + l])
    total = 0.0
    for v in sums:
        total += v
    return SimpleNamespace(V=V, v_obs=v_obs, guarded=guarded, exceed=exceed, counts=flags.reshape(blocks, 256).sum(1).astype(np.int32),
                           sums=np.array(sums), masks=masks, df_sp=max(total / B, 0.0), scale=float(np.mean(V + abs(M))), blocks=blocks)


def results_of(ref, typ, B, alpha):
    """(p or None for sp, used, blocks the finish kernel reads) by a strictly sequential walk over the permutations"""
    if typ.startswith("smc"):
        E = math.floor(alpha * B) + 1
        count = 0
        for b in range(B):
            count += int(ref.exceed[b])
            if count == E:
                return E / B, b + 1, b // 256 + 1
        return count / B, B, ref.blocks
    return (None if typ.startswith("sp") else int(ref.exceed.sum()) / B), B, ref.blocks


# ---------------------------------------------------------------------------------------------------------------------
# 2. The restatement is right: enumeration in exact rationals
# ---------------------------------------------------------------------------------------------------------------------
def tables_with_margins(rows, cols):
    """every non-negative integer table with these row and column sums"""
    if len(rows) == 1:
        yield (tuple(cols),)
        return
    def first_rows(k, left, room):
        if k == len(cols) - 1:
            if left <= room[k]:
                yield (left,)
            return
        for c in range(min(left, room[k]) + 1):
            for rest in first_rows(k + 1, left - c, room):
                yield (c,) + rest
    for r in first_rows(0, rows[0], cols):
        for rest in tables_with_margins(rows[1:], [c - v for c, v in zip(cols, r)]):
            yield (r,) + rest


def table_probability(t, rows, cols):
    f = math.factorial
    num = math.prod(f(r) for r in rows) * math.prod(f(c) for c in cols)
    return Fraction(num, f(sum(rows)) * math.prod(f(c) for r in t for c in r))


EXACT_CASES = {                                                  # name: the observed planes, one per configuration
    "2x2": [[[3, 1], [1, 4]]],
    "2x2 independent": [[[2, 2], [3, 3]]],
    "2x3": [[[3, 0, 2], [1, 4, 1]]],
    "3x3": [[[3, 0, 1], [0, 3, 1], [1, 1, 2]]],
    "3x3 extreme": [[[4, 0, 0], [0, 4, 0], [0, 0, 4]]],           # the observed table is the most extreme: exact p is tiny
    "two configurations": [[[3, 1], [0, 4]], [[1, 2, 0], [2, 0, 3]]],
    "one occupied row": [[[0, 0], [3, 4]], [[2, 1], [1, 2]]],     # the first configuration draws nothing
}


def exact_case(name):
    planes = EXACT_CASES[name]
    rx, ry = max(len(p) for p in planes), max(len(p[0]) for p in planes)
    tab = np.zeros((len(planes), rx, ry), np.int64)
    for z, p in enumerate(planes):
        tab[z, :len(p), :len(p[0])] = p
    assert tab.sum() <= 24 and tab.sum((1, 2)).max() <= 12
    return tab


def exact_statistic(tab, margins, g2):
    """an exactly comparable stand-in of V: prod c^c (an integer, monotone in sum c ln c) or V as a Fraction"""
    if g2:
        return math.prod(int(c) ** int(c) for c in tab.ravel() if c > 1)
    V = Fraction(0)
    for z in range(tab.shape[0]):
        n_xz, n_yz = margins[z].sum(1), margins[z].sum(0)
        V += int(margins[z].sum()) * sum(Fraction(int(tab[z, i, k]) ** 2, int(n_xz[i]) * int(n_yz[k]))
                                         for i in range(tab.shape[1]) for k in range(tab.shape[2]) if n_xz[i] and n_yz[k])
    return V


def exact_law(tab, g2):
    """(exact p, exact mean and variance of the permuted statistic as floats via mpmath) over the product distribution"""
    mp = pc.mpmath
    per_z = []
    for z in range(tab.shape[0]):
        rows, cols = [int(v) for v in tab[z].sum(1)], [int(v) for v in tab[z].sum(0)]
        if sum(rows) == 0:
            per_z.append([(np.zeros(tab.shape[1:], np.int64), Fraction(1))])
            continue
        live = [i for i, r in enumerate(rows) if r]
        plane = []
        for t in tables_with_margins([rows[i] for i in live], cols):
            full = np.zeros(tab.shape[1:], np.int64)
            full[live] = t
            plane.append((full, table_probability(t, [rows[i] for i in live], cols)))
        assert sum(p for _, p in plane) == 1
        per_z.append(plane)
    obs = exact_statistic(tab, tab, g2)
    p_exact, m1, m2 = Fraction(0), mp.mpf(0), mp.mpf(0)
    M = mp.mpf(0)
    if g2:
        f = lambda c: mp.mpf(int(c)) * mp.log(int(c)) if c > 1 else mp.mpf(0)
        for z in range(tab.shape[0]):
            M += sum(f(c) for c in tab[z].sum(0)) + sum(f(c) for c in tab[z].sum(1)) - f(tab[z].sum())
    else:
        M = mp.mpf(int(tab.sum()))
    for combo in itertools.product(*per_z):
        t = np.stack([c[0] for c in combo])
        prob = math.prod((c[1] for c in combo), start=Fraction(1))
        st = exact_statistic(t, tab, g2)
        if st >= obs:
            p_exact += prob
        s = 2 * (sum(f(c) for c in t.ravel()) - M) if g2 else mp.mpf(st.numerator) / st.denominator - M
        w = mp.mpf(prob.numerator) / prob.denominator
        m1 += w * s
        m2 += w * s * s
    return p_exact, float(m1), float(m2 - m1 * m1)


def check_restatement_against_enumeration(name, typ, B=4000, seed=2801):
    """the Monte Carlo p of the restatement lies within 5 standard errors of the exact permutation p (equal where that is 0 or
    1); so does the sp mean, against the exact expectation"""
    g2 = typ.endswith("mi")
    tab = exact_case(name)
    p_exact, mean_exact, var_exact = exact_law(tab, g2)
    ref = perm_reference(tab, g2, B, seed, gt=7)
    assert ref.guarded, (name, typ)
    p_mc = float(ref.exceed.mean())
    se = math.sqrt(float(p_exact * (1 - p_exact)) / B)
    print(f"{name} {typ}: exact p {float(p_exact):.6f}, Monte Carlo {p_mc:.6f} (se {se:.2e}); exact mean {mean_exact:.6f}, "
          f"Monte Carlo {ref.df_sp:.6f} (se {math.sqrt(max(var_exact, 0) / B):.2e})")
    if p_exact in (0, 1):
        assert p_mc == float(p_exact)
    else:
        assert abs(p_mc - float(p_exact)) <= 5 * se, (name, typ, p_mc, float(p_exact), se)
    assert mean_exact >= -1e-12                             # the statistic is non-negative, so no clamp is in the way
    assert abs(ref.df_sp - mean_exact) <= 5 * math.sqrt(max(var_exact, 0.0) / B) + 1e-12, (name, typ, ref.df_sp, mean_exact)
    # every draw of a permutation is made: a uniform table law would fail the 5 se above; the margins are asserted inside
    return p_mc


# ---------------------------------------------------------------------------------------------------------------------
# 3. The kernel is the restatement
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 600), (37, 1), (256, 255), (257, 256), (300, 257), (300, 600))      # (S, B)
MAX_CELLS = 768                                              # (2, 5 | 0) is exactly at it, (2, 5 | 0, 3) above it
TESTS = [(0, 1, ()), (1, 0, ()), (0, 3, (1,)), (2, 5, ()), (2, 5, (0,)), (0, 1, (2, 3)), (4, 0, ()), (4, 0, (1,)), (0, 5, (1, 3)),
         (5, 1, (3, 0)), (3, 0, (4,)),                       # the dependent columns of pc_corpus's six-variable case: p near 0
         (6, 7, ()), (7, 6, ()), (6, 8, (7,)), (7, 8, (6, 9)), (9, 6, (3,)), (8, 9, ()), (9, 7, (1,)), (6, 3, (8,))]     # mid-range p
BAD = [(2, 5, (0, 3)), (2, 2, ()), (0, 1, (0,)), (10, 0, ()), (0, 1, (63,))]
SEED = 2811                                                  # chosen on the CPU: every decision of every case is guarded
ALPHA = 0.05
TEST_OFFSET = 0xFFFFFFF0                                     # the global test index wraps mod 2^32 inside the batch


@functools.lru_cache(maxsize=None)
def perm_case(S):
    """(data [S, 10], card): the six dependent columns of pc_corpus's case (level counts 3, 4 with its top level unobserved, 16,
    2, 1, 16) beside four independent uniform ones (2, 3, 3, 4), whose tests have p-values away from 0"""
    six = pc.ci_case(f"sixS{S}")
    rng = np.random.default_rng(2802)
    extra = np.stack([rng.integers(0, c, 1000) for c in (2, 3, 3, 4)], 1).astype(np.uint8)[:S]
    return np.ascontiguousarray(np.hstack([six.data, extra])), np.concatenate([six.card, np.array([2, 3, 3, 4], np.uint8)])


def all_tests():
    return TESTS[:6] + BAD[:1] + TESTS[6:] + BAD[1:]


@functools.lru_cache(maxsize=None)
def reference(S, B, g2, seed=SEED, offset=TEST_OFFSET):
    """{index in all_tests(): perm_reference} of the tests that are not refused"""
    data, card = perm_case(S)
    refs = {}
    for t, (x, y, zs) in enumerate(all_tests()):
        if (x, y, zs) in BAD:
            continue
        refs[t] = perm_reference(pc.ci_table(data, card, x, y, zs), g2, B, seed, offset + t)
        assert refs[t].guarded, (S, B, g2, t, "choose another SEED")
    return refs


def run_perm(be, data_h, card_h, n, S, tests, typ, B, alpha=ALPHA, seed=SEED, offset=0, slices=1, max_cells=MAX_CELLS):
    """one dvs_ci_perm_tests -> namespace(rc, out [T, 3], used [T], status, counts / sums [T, blocks], masks [T, blocks, 4]); out
    and used sit between sentinels that must come back untouched"""
    T, blocks = len(tests), (B + 255) // 256
    need = int(be.lib.dvs_ci_perm_workspace_bytes(T, B))
    up = lambda v: (v + 255) & ~255
    assert need == up(T * blocks * 4) + up(T * blocks * 8) + up(T * blocks * 32), need
    pairs = np.array([[x, y] for x, y, _ in tests], np.int32)
    cond = np.array([pc.mask_of(zs) for _, _, zs in tests], U64)
    out, used = be.put(np.full((T + 2, 3), -7.0)), be.put(np.full(T + 2, -7, np.int32))
    work = be.put(np.full(need, 0xA5, np.uint8))
    h = dict(pairs=be.put(pairs), cond=be.put(cond), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_ci_perm_tests", n_tests=T, n_vars=n, n_samples=S, data=data_h, card=card_h, perm_type=TYPE_ID[typ], n_perm=B,
                 alpha=alpha, seed=seed, test_offset=offset & 0xFFFFFFFF, slices=slices, max_cells=max_cells, workspace=work,
                 workspace_bytes=need, out=at(be, out, 24), out_bytes=T * 24, used=at(be, used, 4), **h)
    o, u, w = be.get(out).copy(), be.get(used).copy(), be.get(work).copy()
    assert (o[0] == -7.0).all() and (o[-1] == -7.0).all() and u[0] == -7 and u[-1] == -7, "written outside out / used"
    a, b = up(T * blocks * 4), up(T * blocks * 4) + up(T * blocks * 8)
    return SimpleNamespace(rc=rc, out=o[1:-1], used=u[1:-1], status=int(be.get(h["status"])[0]),
                           counts=w[:T * blocks * 4].view(np.int32).reshape(T, blocks),
                           sums=w[a:a + T * blocks * 8].view(np.float64).reshape(T, blocks),
                           masks=w[b:b + T * blocks * 32].view(U64).reshape(T, blocks, 4))


def check_kernel_is_restatement(be, S, B, typ, p_rtol):
    """checks 2, 3 and 5 of one (S, B, type): bytes against the restatement and against dvs_ci_tests, every slices value, the
    batch cut in two, two runs"""
    data, card = perm_case(S)
    n, g2 = data.shape[1], typ.endswith("mi")
    dh, ch = be.put(sc.pack(data)), be.put(card)
    tests, blocks = all_tests(), (B + 255) // 256
    refs = reference(S, B, g2)
    got = run_perm(be, dh, ch, n, S, tests, typ, B, offset=TEST_OFFSET)
    assert got.rc == 0 and got.status == 16, (got.rc, got.status, be.lib.dvs_last_error())
    rc, classic, _ = pc.run_ci(be, dh, ch, n, S, tests, "mi" if g2 else "x2", MAX_CELLS)
    assert rc == 0
    worst = 0.0
    for t, (x, y, zs) in enumerate(tests):
        if t not in refs:
            assert got.out[t].tobytes() == NAN3 and got.used[t] == 0 and np.isnan(classic[t]).all(), (t, got.out[t])
            continue
        ref = refs[t]
        assert got.out[t, 0].tobytes() == classic[t, 0].tobytes(), (typ, t, "observed statistic")
        p, used, read = results_of(ref, typ, B, ALPHA)
        assert got.used[t] == used, (typ, t, got.used[t], used)
        assert got.counts[t, :read].tobytes() == ref.counts[:read].tobytes(), (typ, t, got.counts[t], ref.counts)
        assert got.masks[t, :read].tobytes() == ref.masks[:read].tobytes(), (typ, t)
        if not typ.startswith("sp"):
            assert got.out[t, 1].tobytes() == classic[t, 1].tobytes(), (typ, t, "classic df")
            assert got.out[t, 2].tobytes() == np.float64(p).tobytes(), (typ, t, got.out[t, 2], p)
            continue
        df = float(got.out[t, 1])
        bound = SP_EPS * ref.scale
        print(f"S {S} B {B} {typ} test {t}: df {df!r} restated {ref.df_sp!r} (bound {bound:.2e}), p {got.out[t, 2]!r}")
        assert df >= 0.0 and abs(df - ref.df_sp) <= bound, (typ, t, df, ref.df_sp, bound)
        if df == 0.0:
            assert got.out[t, 2] == 1.0
        else:
            ref_p = pc.mpmath.gammainc(pc.mpmath.mpf(df) / 2, pc.mpmath.mpf(float(got.out[t, 0])) / 2, pc.mpmath.inf, regularized=True)
            err = abs(pc.mpmath.mpf(float(got.out[t, 2])) - ref_p)
            pe = float(max(err - pc.P_FLOOR, 0) / ref_p) if ref_p > 0 else float(err)
            assert 0.0 <= got.out[t, 2] <= 1.0 and pe <= p_rtol, (typ, t, df, pe)
            worst = max(worst, pe)
    # invariance: every slices value, the batch cut in two by test_offset, two runs
    fixed = lambda r: (r.out.tobytes(), r.used.tobytes())
    whole = not typ.startswith("smc")                        # an early stop leaves later blocks to whichever slice owns them
    for slices in sorted({1, min(2, blocks), blocks}):
        r = run_perm(be, dh, ch, n, S, tests, typ, B, offset=TEST_OFFSET, slices=slices)
        assert r.rc == 0 and fixed(r) == fixed(got), (typ, slices)
        if whole:
            live = sorted(refs)
            assert r.counts[live].tobytes() == got.counts[live].tobytes() and r.sums[live].tobytes() == got.sums[live].tobytes()
    cut = 9
    a = run_perm(be, dh, ch, n, S, tests[:cut], typ, B, offset=TEST_OFFSET, slices=blocks)
    b = run_perm(be, dh, ch, n, S, tests[cut:], typ, B, offset=TEST_OFFSET + cut)
    assert a.out.tobytes() + b.out.tobytes() == got.out.tobytes() and a.used.tobytes() + b.used.tobytes() == got.used.tobytes()
    other = run_perm(be, dh, ch, n, S, tests, typ, B, offset=TEST_OFFSET + 1)
    if S > 1 and B > 1 and not typ.startswith("sp"):
        assert other.masks[sorted(refs)].tobytes() != got.masks[sorted(refs)].tobytes()      # the offset does reach the draws
    return worst


def check_shapes_covered():
    """the corpus holds what it says: level counts 1, 2, 3, 16, 0 to 2 conditioning variables, an unobserved level, a
    configuration with one occupied row among others, a table at max_cells and one above"""
    data, card = perm_case(300)
    card = [int(c) for c in card]
    assert {card[v] for x, y, _ in TESTS for v in (x, y)} >= {1, 2, 3, 16} and {len(zs) for _, _, zs in TESTS} == {0, 1, 2}
    assert data[:, 1].max() + 1 < card[1]                                               # an unobserved level
    assert pc.cells_of(card, 2, 5, (0,)) == MAX_CELLS < pc.cells_of(card, *BAD[0])
    tab = pc.ci_table(data, card, 0, 1, (2, 3))
    occupied = (tab.sum(2) > 0).sum(1)
    assert (occupied == 1).any() and (occupied > 1).any() and (tab.sum((1, 2)) == 0).any()


def check_klnk_paths(be):
    """k ln k comes from an LDS table when 8 (S + 1) bytes fit beside the counts in 159 744 bytes of dynamic LDS, from log
    otherwise: at max_cells = 36 864 the table holds S <= 1535.  Either side of that threshold, and with a small max_cells
    (the table path at both sizes), the bytes are equal, block sums included, and the sp df is the restatement's within its
    bound.  (At these row counts the values of V lie too densely for the decision guard, so the counts are compared between
    the paths, not with numpy; check_kernel_is_restatement does that at its sizes.)"""
    rng = np.random.default_rng(2803)
    cards = np.array([2, 3, 3, 4], np.uint8)
    full = np.stack([rng.integers(0, c, 1536) for c in cards], 1).astype(np.uint8)
    tests, B = [(0, 1, ()), (1, 2, (0,)), (2, 3, (0, 1))], 256
    for S in (1535, 1536):
        assert (8 * (S + 1) + 4 * pc.MAX_CELLS <= 159744) == (S == 1535)
        data = full[:S]
        dh, ch = be.put(sc.pack(data)), be.put(cards)
        for typ in ("mc-mi", "sp-mi"):
            big = run_perm(be, dh, ch, 4, S, tests, typ, B, seed=SEED + 1, max_cells=pc.MAX_CELLS)
            small = run_perm(be, dh, ch, 4, S, tests, typ, B, seed=SEED + 1, max_cells=72)
            assert big.rc == 0 and small.rc == 0 and big.status == 0 and small.status == 0
            assert big.out.tobytes() == small.out.tobytes() and big.counts.tobytes() == small.counts.tobytes(), (S, typ)
            assert big.sums.tobytes() == small.sums.tobytes() and big.masks.tobytes() == small.masks.tobytes(), (S, typ)
            assert 0 < big.counts.sum() < 3 * B
            for t, (x, y, zs) in enumerate(tests if typ == "sp-mi" else ()):
                ref = perm_reference(pc.ci_table(data, cards, x, y, zs), True, B, SEED + 1, t)
                assert abs(big.out[t, 1] - ref.df_sp) <= SP_EPS * ref.scale, (S, t, big.out[t, 1], ref.df_sp)


def check_smc_stops(be):
    """check 4 at S = 300, B = 600 (three blocks): the stop in the first block, inside the second, exactly at a block boundary,
    never, and in a later slice than the first, against the strictly sequential walk"""
    S, B = 300, 600
    data, card = perm_case(S)
    n = data.shape[1]
    dh, ch = be.put(sc.pack(data)), be.put(card)
    tests = all_tests()
    seen = set()
    for typ in ("smc-mi", "smc-x2"):
        by_test = reference(S, B, typ.endswith("mi"))
        live = sorted(by_test)
        refs = [by_test[t] for t in live]
        # an alpha whose E-th exceeding permutation is b = 255 or b = 511 of some test: the stop exactly at a block boundary
        edge = [(int(r.exceed[:b + 1].sum()) - 0.5) / B for r in refs for b in (255, 511) if r.exceed[b]]
        assert edge, "no test exceeds at b = 255 or b = 511"
        for alpha in (0.05, 0.3, 0.45, edge[0]):
            want = [results_of(r, typ, B, alpha) for r in refs]
            for slices in (1, 2, 3):
                got = run_perm(be, dh, ch, n, S, tests, typ, B, alpha=alpha, offset=TEST_OFFSET, slices=slices)
                assert got.rc == 0 and got.status == 16
                for t, (p, used, read), ref in zip(live, want, refs):
                    assert got.used[t] == used and got.out[t, 2].tobytes() == np.float64(p).tobytes(), (typ, alpha, slices, t, got.used[t], used)
                    assert got.counts[t, :read].tobytes() == ref.counts[:read].tobytes()
            E = math.floor(alpha * B) + 1
            for (p, used, read), r in zip(want, refs):
                stopped = int(r.exceed.sum()) >= E
                seen |= {"never"} if not stopped else set()
                seen |= {"first block"} if stopped and used <= 256 else set()
                seen |= {"inside the second block"} if stopped and 257 <= used < 512 else set()
                seen |= {"at a block boundary"} if stopped and used in (256, 512) else set()
                seen |= {"in a later slice"} if stopped and used > 256 else set()              # slices = 2, 3: not slice 0
    assert seen == {"never", "first block", "inside the second block", "at a block boundary", "in a later slice"}, seen


# ---------------------------------------------------------------------------------------------------------------------
# 4. PC-stable over the restatement
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pc_reference(name, S, typ, B, seed, alpha):
    """pc_corpus.pc_ref with every test decided by the restatement: p = count / B > alpha, the tests numbered on across levels"""
    data, card = pc.e2e_data(name, S)
    g2 = typ.endswith("mi")
    counter = itertools.count()

    def independent(x, y, zmask):
        ref = perm_reference(pc.ci_table(data, card, x, y, list(cp.bits(zmask))), g2, B, seed, next(counter))
        assert ref.guarded, (x, y, zmask)
        return results_of(ref, typ, B, alpha)[0] > alpha
    return pc.pc_ref(data.shape[1], independent)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []
    nan = float("nan")
    c = entry("dvs_ci_perm_tests", cases, n_tests=8, n_vars=12, n_samples=100, data=D, card=D, pairs=D, cond=D, perm_type=0,
              n_perm=600, alpha=0.05, seed=1, test_offset=0, slices=3, max_cells=729, workspace=D, workspace_bytes=1280, out=D,
              out_bytes=192, used=D, status=D, stream=None)
    c(2, "n_tests and n_samples must be > 0", n_tests=0)
    c(2, "n_tests and n_samples must be > 0", n_samples=-1)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(12, "perm_type is not a dvs_ci_perm_type", perm_type=6)
    c(12, "perm_type is not a dvs_ci_perm_type", perm_type=-1)
    c(13, "n_perm must be in [1, 2^20]", n_perm=0)
    c(13, "n_perm must be in [1, 2^20]", n_perm=(1 << 20) + 1)
    for typ in (2, 3):
        for bad in (0.0, 1.0, -0.1, nan):
            c(13, "alpha must be in (0, 1)", perm_type=typ, alpha=bad)
    c(13, "slices must be in [1, ceil(n_perm / 256)]", slices=0)
    c(13, "slices must be in [1, ceil(n_perm / 256)]", slices=4)
    c(13, "max_cells must be in [1, 36864]", max_cells=0)
    c(13, "max_cells must be in [1, 36864]", max_cells=36865)
    c(2, "n_tests * blocks must be < 2^31", n_tests=1 << 20, n_perm=1 << 20, slices=1, workspace_bytes=1 << 50, out_bytes=1 << 40)
    for name in ("data", "card", "pairs", "cond", "workspace", "out", "used", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "workspace_bytes < dvs_ci_perm_workspace_bytes = 1280", workspace_bytes=1279)
    c(14, "out_bytes < n_tests * 24 = 192", out_bytes=191)
    c(2, "n_tests and n_samples must be > 0", n_tests=0, n_vars=49)                    # sizes before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, perm_type=9)                          # n_vars before the type
    c(12, "perm_type is not a dvs_ci_perm_type", perm_type=9, n_perm=0)                # the type before n_perm
    c(13, "n_perm must be in [1, 2^20]", n_perm=0, perm_type=2, alpha=nan)             # n_perm before alpha
    c(13, "alpha must be in (0, 1)", perm_type=2, alpha=nan, slices=0)                 # alpha before slices
    c(13, "slices must be in", slices=0, max_cells=0)                                  # slices before max_cells
    c(13, "max_cells must be in [1, 36864]", max_cells=0, data=None)                   # max_cells before null
    c(10, "null pointer", status=None, workspace_bytes=0)                              # null before workspace_bytes
    c(14, "workspace_bytes <", workspace_bytes=0, out_bytes=0)                         # workspace_bytes before out_bytes
    for typ in (0, 1, 4, 5):                                                           # alpha is read for smc only
        c(10, "null pointer", perm_type=typ, alpha=nan, status=None)
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_ci_perm_tests"}
    run(lib, cases)
    # the size query: 0 with a message for an argument out of range, the stated layout otherwise
    assert lib.dvs_ci_perm_workspace_bytes(8, 600) == 1280 and lib.dvs_ci_perm_workspace_bytes(1, 1) == 768
    for bad, text in (((0, 600), "n_tests must be > 0"), ((8, 0), "n_perm must be in [1, 2^20]"), ((8, (1 << 20) + 1), "n_perm must be in"),
                      ((1 << 20, 1 << 20), "n_tests * blocks must be < 2^31")):
        assert lib.dvs_ci_perm_workspace_bytes(*bad) == 0
        msg = lib.dvs_last_error().decode()
        assert msg.startswith("dvs_ci_perm_workspace_bytes:") and text in msg, (bad, msg)
