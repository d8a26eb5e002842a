"""TEST HELPER: references and checks for dvs_bn_scores (csrc/k_bic.hip: loglik, aic, bic, bde, bds, k2, bdj), written once
and run by tests/test_emu_bn_scores.py (emulator build) and tests/test_gpu_bn_scores.py (device).  The data, masks, cases,
backends and `expected_path` are those of tests/scoring_corpus.py — imported, not copied — so the new score types cover the
range include/dvs.h promises for dvs_bic_scores: one and several data words, level counts 1-16, both sides of the dense /
sort switch, batches of 1 / 255 / 256 / 257, the real asia and sachs data, the three refusals.

References
  reference_local: bnlearn's documented definitions (include/dvs.h restates them) in mpmath at 60 digits over the occupied
        cells only, so that 16^15 configurations are representable; q is a Python integer, iss / (r q) an mpmath quotient.
  second_local: the same sums in float64 with scipy.special.gammaln / math.log / math.fsum over per-cell arrays (no
        multiplicity table, no mpmath): an independent second evaluation, asserted equal to the first at the tolerance
        below wherever a reference is made.
  Neither is a bnlearn run: R and bnlearn are not available to this suite and the reference project holds recorded values
  for "bic" only, so parity of the other types rests on the definitions.  The anchors of this module (k2
  against exact factorials, score equivalence of bde / bic / aic / loglik under a covered-edge reversal and its failure
  for k2 / bdj, bic's bytes against dvs_bic_scores) do not use the restated formulas.

Tolerance (derived, the convention of tests/scoring_corpus.py): fp64 on both sides; a local score is a sum of at most 2 S
        terms, each a few roundings (an addition, lgamma or division + log, a subtraction or product), added at most
        2 S / 256 per lane and then in a tree of 8 levels, so the error is below (2 S / 256 + 14) * 2^-53 * T with T the sum
        of the absolute values of every lgamma or N log term entering the score plus |penalty| — 4e-14 * T at S = 40 000 —
        provided lgamma itself is good to a few units in the last place OF ITS OWN VALUE.  Asserted: |got - ref| <=
        1e-12 * T per local score.  libm's lgamma against mpmath: <= 6e-17 * T (spot check).  What the emulator build and
        the device give is printed per type by the tests and recorded in their docstrings.
"""
import functools
import math
from collections import Counter, namedtuple

import mpmath
import numpy as np
from scipy.special import gammaln

from tests import scoring_corpus as sc
from tests.abi_cases import call_rc

MP = mpmath.mp.clone()
MP.dps = 60
RTOL = sc.BIC_RTOL                                       # 1e-12, the project's convention
TYPE_CODE = {"loglik": 0, "aic": 1, "bic": 2, "bde": 3, "bds": 4, "k2": 5, "bdj": 6}      # dvs_score_type (include/dvs.h)
PENALISED = ("loglik", "aic", "bic")
# (type, argument or None for the type's default): every type at its default, each argument once away from it
VARIANTS = (("loglik", None), ("aic", None), ("aic", 2.5), ("bic", None), ("bic", 0.75), ("bde", None), ("bde", 10.0),
            ("bds", None), ("bds", 10.0), ("k2", None), ("bdj", None))
NAN = float("nan")

Counts = namedtuple("Counts", "S r q njk nj_cell nj_row")
Counts.__doc__ = """occupied cells of one (variable, parent set): njk int64 [cells] > 0, nj_cell int64 [cells] the N_j of each
cell's configuration, nj_row int64 [observed configurations] > 0; r, q Python integers."""


@functools.lru_cache(maxsize=None)
def _counts_cached(case_name, v, parents):
    case = sc.bic_case(case_name)
    return cell_counts(case.data, case.card, v, parents)


def cell_counts(data, card, v, parents):
    parents = sorted(int(p) for p in parents)
    assert v not in parents and len(set(parents)) == len(parents)
    S = data.shape[0]
    q = 1
    for p in parents:
        q *= int(card[p])
    cells, njk = np.unique(data[:, parents + [v]], axis=0, return_counts=True)
    if parents:
        _, inv = np.unique(cells[:, :-1], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        nj_row = np.bincount(inv, weights=njk).astype(np.int64)
        nj_cell = nj_row[inv]
    else:
        nj_row = np.asarray([S], np.int64)
        nj_cell = np.full(len(njk), S, np.int64)
    assert int(njk.sum()) == S == int(nj_row.sum()) and (njk > 0).all()
    return Counts(S, int(card[v]), q, njk.astype(np.int64), nj_cell, nj_row)


def _prior(typ, arg, r, q, q_observed, div):
    """(a_j, a_jk) of the Dirichlet scores; `div(x, y)` is the division of the arithmetic in use."""
    if typ == "k2":
        return r, 1
    if typ == "bdj":
        return div(r, 2), div(1, 2)
    iss = 1.0 if arg is None else arg
    qq = q_observed if typ == "bds" else q
    return div(iss, qq), div(iss, r * qq)


def reference_local(c, typ, arg):
    """(local score, T) at 60 digits, from multiplicity tables of the occupied cells."""
    mpf, fabs = MP.mpf, MP.fabs
    if typ in PENALISED:
        total = T = mpf(0)
        for (n, nj), mult in Counter(zip(c.njk.tolist(), c.nj_cell.tolist())).items():
            t = n * MP.log(mpf(n) / nj)
            total += mult * t
            T += mult * fabs(t)
        k = 0 if typ == "loglik" else arg if arg is not None else 1 if typ == "aic" else MP.log(c.S) / 2
        pen = mpf(k) * (c.r - 1) * c.q
        return float(total - pen), float(T + fabs(pen))
    aj, ajk = _prior(typ, arg, c.r, c.q, len(c.nj_row), lambda x, y: mpf(x) / mpf(y))
    lg_aj, lg_ajk = MP.loggamma(aj), MP.loggamma(ajk)
    total = T = mpf(0)
    for nj, mult in Counter(c.nj_row.tolist()).items():
        t = MP.loggamma(aj + nj)
        total += mult * (lg_aj - t)
        T += mult * (fabs(lg_aj) + fabs(t))
    for n, mult in Counter(c.njk.tolist()).items():
        t = MP.loggamma(ajk + n)
        total += mult * (t - lg_ajk)
        T += mult * (fabs(t) + fabs(lg_ajk))
    return float(total), float(T)


def second_local(c, typ, arg):
    """The same local score in float64 (scipy.special.gammaln, math.log, math.fsum), cell by cell."""
    if typ in PENALISED:
        terms = [n * math.log(n / nj) for n, nj in zip(c.njk.tolist(), c.nj_cell.tolist())]
        k = 0.0 if typ == "loglik" else arg if arg is not None else 1.0 if typ == "aic" else 0.5 * math.log(c.S)
        return math.fsum(terms) - k * (c.r - 1) * c.q
    aj, ajk = _prior(typ, arg, c.r, c.q, len(c.nj_row), lambda x, y: float(x) / float(y))
    rows = gammaln(float(aj)) - gammaln(aj + c.nj_row.astype(np.float64))
    cells = gammaln(ajk + c.njk.astype(np.float64)) - gammaln(float(ajk))
    return math.fsum(rows.tolist() + cells.tolist())


_ref_cache = {}


def bn_reference(case, typ, arg):
    """(local [B, n], T [B, n]); NaN in the refused cells.  Asserts the second evaluation on every distinct cell."""
    key = (case.name, typ, arg)
    if key in _ref_cache:
        return _ref_cache[key]
    B, n = case.masks.shape
    loc = np.full((B, n), np.nan)
    tol = np.full((B, n), np.nan)
    memo = {}
    for b in range(B):
        for v in range(n):
            if (b, v) in case.refused:
                assert sc.expected_path(case, b, v) == "refused", (case.name, b, v)
                continue
            assert sc.expected_path(case, b, v) != "refused", (case.name, b, v)
            ps = tuple(u for u in sc.mask_bits(case.masks[b, v]) if u != v)
            if (v, ps) not in memo:
                c = _counts_cached(case.name, v, ps)
                memo[v, ps] = reference_local(c, typ, arg)
                second = second_local(c, typ, arg)
                assert abs(second - memo[v, ps][0]) <= RTOL * memo[v, ps][1], (case.name, typ, arg, v, ps, second, memo[v, ps])
            loc[b, v], tol[b, v] = memo[v, ps]
    _ref_cache[key] = (loc, tol)
    return loc, tol


def run_bn(be, data, card, masks, typ, arg=None, type_code=None):
    """one dvs_bn_scores call -> (return code, scratch [B, n], out [B], status)."""
    B, n = masks.shape
    h = dict(data=be.put(sc.pack(data)), card=be.put(card), parents=be.put(np.ascontiguousarray(masks, sc.U64)),
             scratch=be.put(np.full((B, n), -7.0)), out=be.put(np.full(B, -7.0)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bn_scores", batch=B, n_vars=n, n_samples=data.shape[0], **h,
                 score_type=TYPE_CODE[typ] if type_code is None else type_code, score_arg=NAN if arg is None else float(arg))
    return rc, be.get(h["scratch"]).copy(), be.get(h["out"]).copy(), int(be.get(h["status"])[0])


def check_bn_case(be, case, typ, arg, twice=True):
    """scoring_corpus.check_bic_case for one (type, argument): local scores and per-DAG sums against the reference at
    1e-12 * T, refused cells NaN with status 16 and every other cell intact, the case's bitwise-equal pairs and exact
    zeros, two calls equal bytes.  Returns (worst |got - ref| / T, the cell it was seen at)."""
    loc, tol = bn_reference(case, typ, arg)
    rc, scratch, out, status = run_bn(be, case.data, case.card, case.masks, typ, arg)
    assert rc == 0 and status == case.status, (case.name, typ, rc, status)
    B, n = case.masks.shape
    worst, where = 0.0, None
    bad_dags = {b for b, _ in case.refused}
    for b in range(B):
        for v in range(n):
            if (b, v) in case.refused:
                assert np.isnan(scratch[b, v]), (case.name, typ, b, v, scratch[b, v])
                continue
            err = abs(scratch[b, v] - loc[b, v])
            assert err <= RTOL * tol[b, v], (case.name, typ, arg, "dag", b, "variable", v, sc.expected_path(case, b, v),
                                             scratch[b, v], loc[b, v], err / max(tol[b, v], 1e-300))
            if tol[b, v] > 0 and err / tol[b, v] > worst:
                worst, where = err / tol[b, v], (case.name, b, v)
        if b in bad_dags:
            assert np.isnan(out[b]), (case.name, typ, b, out[b])
        else:
            assert abs(out[b] - math.fsum(loc[b])) <= RTOL * math.fsum(tol[b]), (case.name, typ, "dag", b, out[b])
    for (b0, v0), (b1, v1) in case.bitwise_pairs:
        assert scratch[b0, v0].tobytes() == scratch[b1, v1].tobytes(), (case.name, typ, (b0, v0), (b1, v1))
    for b, v in case.zero_cells:
        assert scratch[b, v] == 0.0, (case.name, typ, b, v, scratch[b, v])
    if twice:
        rc, scratch2, out2, status2 = run_bn(be, case.data, case.card, case.masks, typ, arg)
        assert rc == 0 and status2 == status and scratch2.tobytes() == scratch.tobytes() and out2.tobytes() == out.tobytes()
    return worst, where


def check_all_variants(be, case, twice, worst_by_type):
    for typ, arg in VARIANTS:
        w, where = check_bn_case(be, case, typ, arg, twice)
        if w > worst_by_type.get(typ, (0.0, None))[0]:
            worst_by_type[typ] = (w, where)


def report(worst_by_type, where):
    for typ in TYPE_CODE:
        if typ in worst_by_type:
            w, cell = worst_by_type[typ]
            print(f"\n{where} {typ}: worst |got - ref| / T = {w:.3g} at {cell} (asserted <= {RTOL:g})")


# ---------------------------------------------------------------------------------------------------------------------
# Anchors that do not use the restated formulas
# ---------------------------------------------------------------------------------------------------------------------
def check_shared_condition():
    """What scoring_corpus promises about its cases and this module relies on: the refused cells of a case are exactly the
    ones the documented limits refuse and sit in at most one DAG in four."""
    for name in sc.BIC_CASE_NAMES:
        case = sc.bic_case(name)
        B, n = case.masks.shape
        want = {(b, v) for b in range(B) for v in range(n) if sc.expected_path(case, b, v) == "refused"}
        assert want == set(case.refused), name
        assert len({b for b, _ in want}) * 4 <= B, name
        assert case.status == (16 if want else 0), name


def check_k2_against_factorials(be):
    """k2 of a parentless binary variable with counts (a, b) is log(a! b! / (a + b + 1)!): exact integers, one logarithm
    each at 60 digits.  T: the three logarithms' absolute values."""
    for a, b in ((1, 1), (5, 3), (0, 7), (300, 700), (12345, 4000)):
        data = np.concatenate([np.zeros(a, np.uint8), np.ones(b, np.uint8)])[:, None]
        rc, scratch, out, status = run_bn(be, data, np.asarray([2], np.uint8), np.zeros((1, 1), sc.U64), "k2")
        logs = [MP.log(math.factorial(x)) for x in (a, b, a + b + 1)]
        want, T = float(logs[0] + logs[1] - logs[2]), float(sum(MP.fabs(x) for x in logs))
        assert rc == 0 and status == 0
        assert abs(scratch[0, 0] - want) <= RTOL * T and out[0] == scratch[0, 0], ((a, b), scratch[0, 0], want)


def check_covered_edge_reversal(be):
    """A -> B against B -> A under a common child C (a covered edge: the two DAGs are Markov equivalent): bde, bic, aic and
    loglik are score equivalent, k2 and bdj are not (they differ by more than 1e-3 on this dependent data)."""
    data, card = sc.synthetic_dataset(3, 800, [3, 4, 2], seed=808)
    masks = sc.masks_of(3, {1: [0], 2: [0, 1]}, {0: [1], 2: [0, 1]})
    case = sc._case("coverededge", data, card, masks)
    for typ, arg in (("bde", None), ("bde", 10.0), ("bic", None), ("aic", None), ("loglik", None), ("k2", None), ("bdj", None)):
        rc, scratch, out, status = run_bn(be, data, card, masks, typ, arg)
        assert rc == 0 and status == 0
        T = sum(reference_local(cell_counts(data, card, v, sc.mask_bits(masks[b, v])), typ, arg)[1]
                for b in range(2) for v in range(3))
        if typ in ("k2", "bdj"):
            assert abs(out[0] - out[1]) > 1e-3, (typ, out)
        else:
            assert abs(out[0] - out[1]) <= RTOL * T, (typ, arg, out, T)
            assert scratch[0, 2].tobytes() == scratch[1, 2].tobytes()          # the common child's local score
            assert abs(scratch[0, 0] - scratch[1, 0]) > 1e-3                   # ... while the two ends' own scores move
    return case


BYTES_CASES = ("asia", "sachs", "levels", "boundary", "keybits64", "wide48", "batch257", "sortS257")


def check_bic_bytes_and_aic_relations(be, name):
    """bic with the default argument gives dvs_bic_scores' bytes (local scores, sums, status; refused cells included);
    aic with k = log(S) / 2 equals bic within tolerance; aic with k = 0 equals loglik bitwise."""
    case = sc.bic_case(name)
    rc0, scratch0, out0, status0 = sc.run_bic(be, case.data, case.card, case.masks)
    rc1, scratch1, out1, status1 = run_bn(be, case.data, case.card, case.masks, "bic")
    assert rc0 == rc1 == 0 and status0 == status1 == case.status
    assert scratch0.tobytes() == scratch1.tobytes() and out0.tobytes() == out1.tobytes(), name
    _, tol = bn_reference(case, "bic", None)
    rc, scratch, out, _ = run_bn(be, case.data, case.card, case.masks, "aic", 0.5 * math.log(case.data.shape[0]))
    ok = ~np.isnan(tol)
    assert rc == 0 and (np.abs(scratch - scratch1)[ok] <= RTOL * tol[ok]).all(), name
    assert np.array_equal(np.isnan(scratch), ~ok)
    rc2, scratch2, out2, _ = run_bn(be, case.data, case.card, case.masks, "aic", 0.0)
    rc3, scratch3, out3, _ = run_bn(be, case.data, case.card, case.masks, "loglik")
    assert rc2 == rc3 == 0 and scratch2.tobytes() == scratch3.tobytes() and out2.tobytes() == out3.tobytes(), name
    rc4, scratch4, _, _ = run_bn(be, case.data, case.card, case.masks, "aic")
    assert rc4 == 0 and (scratch4[ok] <= scratch3[ok]).all() and (scratch4[ok] < scratch3[ok]).any()   # default k = 1, not 0


BDS_CASES = ("levels", "asia", "sachs", "batch257", "wide17", "sortS1000")


def check_bds_against_bde(be, name, iss=10.0):
    """bds equals bde wherever every parent configuration is observed (and always for a variable without parents) and
    differs wherever one is not; on the `levels` data, whose variable 5 never takes its top level, the children of 5 are
    such cells and their two scores are more than 1e-3 apart.  Returns (cells equal, cells different)."""
    case = sc.bic_case(name)
    ref_e, tol_e = bn_reference(case, "bde", iss)
    ref_s, tol_s = bn_reference(case, "bds", iss)
    _, bde, _, _ = run_bn(be, case.data, case.card, case.masks, "bde", iss)
    _, bds, _, _ = run_bn(be, case.data, case.card, case.masks, "bds", iss)
    B, n = case.masks.shape
    same = diff = 0
    for b in range(B):
        for v in range(n):
            if (b, v) in case.refused:
                continue
            ps = tuple(u for u in sc.mask_bits(case.masks[b, v]) if u != v)
            c = _counts_cached(case.name, v, ps)
            if len(c.nj_row) == c.q:
                assert abs(bds[b, v] - bde[b, v]) <= RTOL * (tol_e[b, v] + tol_s[b, v]), (name, b, v)
                same += 1
            elif abs(ref_s[b, v] - ref_e[b, v]) > 2e-3:
                assert abs(bds[b, v] - bde[b, v]) > 1e-3, (name, b, v, bds[b, v], bde[b, v])
                diff += 1
    if name == "levels":
        for b, v in ((0, 6), (0, 12), (1, 6)):                              # parents include variable 5
            assert 5 in sc.mask_bits(case.masks[b, v]) and abs(ref_s[b, v] - ref_e[b, v]) > 2e-3
            assert abs(bds[b, v] - bde[b, v]) > 1e-3
    return same, diff


def check_dense_and_sort_paths_agree(be):
    """One table counted by both paths.  Child 0 (16 levels) with parents 1, 2, 3 (16, 16, 9 levels) is a dense table of
    exactly 36 864 cells; adding parent 4, a copy of column 1, leaves every count as it was and multiplies q by 16: 589 824
    cells, the sort path.  The observed configurations are the same, so bds (and k2, bdj, loglik) must agree directly; bde
    sees q, so it agrees at 16 times the imaginary sample size (a_jk = iss / (r q) is then the same double).  The same
    with the nearest smaller dense table (a 15-level child: 34 560 cells)."""
    worst = 0.0
    for child_levels in (16, 15):
        base, _ = sc.synthetic_dataset(4, 1500, [child_levels, 16, 16, 9], seed=4242 + child_levels)
        data = np.concatenate([base, base[:, 1:2]], 1)
        card = np.asarray([child_levels, 16, 16, 9, 16], np.uint8)
        masks = sc.masks_of(5, {0: [1, 2, 3]}, {0: [1, 2, 3, 4]})
        case = sc._case("densesort", data, card, masks)
        assert sc.expected_path(case, 0, 0) == "dense" and sc.expected_path(case, 1, 0) == "sort"
        assert sc.cells_of(card, 0, [1, 2, 3]) == (sc.MAX_BINS if child_levels == 16 else 34560)
        c = cell_counts(data, card, 0, [1, 2, 3])
        assert len(c.nj_row) < c.q                                          # bds has something to count
        for typ, arg, arg_sort in (("bds", 10.0, 10.0), ("bds", None, None), ("k2", None, None), ("bdj", None, None),
                                   ("loglik", None, None), ("bde", 10.0, 160.0), ("bde", None, 16.0)):
            _, T = reference_local(c, typ, arg)
            rc0, s0, _, st0 = run_bn(be, data, card, masks, typ, arg)
            rc1, s1, _, st1 = run_bn(be, data, card, masks, typ, arg_sort)
            assert rc0 == rc1 == 0 and st0 == st1 == 0
            err = abs(s0[0, 0] - s1[1, 0])
            assert err <= 2 * RTOL * T, (child_levels, typ, arg, s0[0, 0], s1[1, 0])
            worst = max(worst, err / T)
            ref = reference_local(c, typ, arg)[0]
            assert abs(s0[0, 0] - ref) <= RTOL * T and abs(s1[1, 0] - ref) <= RTOL * T
    return worst


def check_argument_refusals(lib, ptr):
    """dvs_bn_scores validates before it enqueues: `ptr` is any non-null pointer value (never dereferenced)."""
    be, p = sc.EmuBackend(lib), ptr                          # nothing is moved: dummy pointers as they are, the null stream
    call = lambda code, arg, B=4, n=8, S=100, d=p, st=p: call_rc(
        be, "dvs_bn_scores", batch=B, n_vars=n, n_samples=S, data=d, card=p, parents=p, score_type=code, score_arg=arg, scratch=p,
        out=p, status=st)
    inf = float("inf")
    for code in (-1, 7, 100):
        assert call(code, NAN) == 12 and b"score_type" in lib.dvs_last_error()
    for typ in ("bde", "bds"):
        for arg in (0.0, -1.0, inf, -inf):
            assert call(TYPE_CODE[typ], arg) == 13 and b"iss" in lib.dvs_last_error(), (typ, arg)
    for typ in ("aic", "bic"):
        for arg in (-1e-9, -1.0, inf, -inf):
            assert call(TYPE_CODE[typ], arg) == 13 and b"k must" in lib.dvs_last_error(), (typ, arg)
    for typ in ("loglik", "k2", "bdj"):
        assert call(TYPE_CODE[typ], 1.0) == 13
    assert call(TYPE_CODE["bde"], 1.0, B=0) == 2 and call(TYPE_CODE["bde"], 1.0, S=0) == 2
    assert call(TYPE_CODE["bde"], 1.0, n=0) == 3 and call(TYPE_CODE["bde"], 1.0, n=49) == 3
    assert call(TYPE_CODE["bde"], 1.0, d=None) == 10 and call(TYPE_CODE["bde"], 1.0, st=None) == 10
