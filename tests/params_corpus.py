"""TEST HELPER: cases, references and the checks themselves for the BN-parameter calls of csrc/dvs_params.h (dvs_bn_fit,
dvs_bn_sample_workspace_bytes, dvs_bn_sample, dvs_bn_loglik; definitions in include/dvs.h).  Plain numpy, no GPU:
tests/test_emu_params.py (emulator build) and tests/test_gpu_params.py (device) run the same checks and differ only in the
backend that moves buffers (tests/scoring_corpus.py); tests/test_params_ref.py checks the restatements themselves.

References
  fit      exact rationals (fractions.Fraction) from integer counts, rounded once by float().
  sample   sample_ref: the thresholds and the draws of include/dvs.h restated with oracle.rng.site_key / draw as they are.
  loglik   math.fsum of math.log over the cells a row reads.

Tolerances are derived, not measured.
  fit, mle     one correctly rounded fp64 division of two exact integers: equal bits.
  fit, bayes   (N_jk + a) / (N_j + r a), a = iss / (r q): a carries the roundings of r q (exact: an integer below 2^53) and of
               the division, r a one more, each sum one more, the last division one more.  Numerator and denominator are each
               within 2 * 2^-53 of exact (the error of a enters a sum no larger than itself), their quotient within 4 * 2^-53
               plus its own rounding; against the correctly rounded reference, 2^-51 relative, as the issue sets it.
               A row of r such cells sums to 1 within r * 2^-52 (each cell within 2^-52 of exact in the same direction at worst).
  loglik       fp64 on both sides; a row term is a sum of n logarithms of one rounding each, out a tree over 256 rows and a
               chain over the chunks: the error is below (n + 8 + chunks) * 2^-53 * T <= 1e-13 * T at these sizes, with T the sum
               of |log theta| over the terms read.  Asserted: sc.BIC_RTOL * T, the project's convention (tests/scoring_corpus.py).
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle import rng as orng
from tests import scoring_corpus as sc
from tests.abi_cases import call_rc, entry, run

U64 = np.uint64
MAX_CELLS = 36864            # include/dvs.h: the dense table of dvs_bn_fit
LDS_CELLS = 8192             # include/dvs.h: thresholds are staged in LDS up to here
SITE_BN_SAMPLE = 500
SENTINEL = -7.0              # pre-fill of every output: a cell that still holds it was not written
ROW_COUNTS = (1, 255, 256, 257, 1000)
ISS_VALUES = (0.5, 1.0, 10.0)
FIT_BAYES_RTOL = 2.0 ** -51
LOG_RTOL = sc.BIC_RTOL


# ---------------------------------------------------------------------------------------------------------------------
# Layout
# ---------------------------------------------------------------------------------------------------------------------
def parents_of(mask, v):
    return [u for u in sc.mask_bits(mask) if u != v]


def family_shape(card, mask, v):
    """(parents, q, r) of variable v under the parent row `mask`"""
    ps = parents_of(mask, v)
    q = 1
    for p in ps:
        q *= int(card[p])
    return ps, q, int(card[v])


def offsets_of(card, masks):
    """int64 [B * n + 1]: the slots of every family, packed without gaps"""
    B, n = masks.shape
    off = [0]
    for b in range(B):
        for v in range(n):
            _, q, r = family_shape(card, masks[b, v], v)
            off.append(off[-1] + q * r)
    return np.asarray(off, np.int64)


def config_keys(levels, card, ps):
    """mixed-radix parent configuration of every row, lowest variable id fastest"""
    key = np.zeros(levels.shape[0], np.int64)
    stride = 1
    for p in ps:
        key += levels[:, p].astype(np.int64) * stride
        stride *= int(card[p])
    return key


def family_counts(data, card, mask, v):
    ps, q, r = family_shape(card, mask, v)
    idx = config_keys(data, card, ps) * r + data[:, v].astype(np.int64)
    return np.bincount(idx, minlength=q * r).reshape(q, r)


def tables_of(cpt, card, masks, offsets):
    """[[table [q, r] of variable v] of structure b] as views of the flat buffer"""
    B, n = masks.shape
    out = []
    for b in range(B):
        row = []
        for v in range(n):
            _, q, r = family_shape(card, masks[b, v], v)
            lo = int(offsets[b * n + v])
            row.append(cpt[lo:lo + q * r].reshape(q, r))
        out.append(row)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# 1. Fit
# ---------------------------------------------------------------------------------------------------------------------
def fit_reference(counts, method, iss, unobserved):
    """counts int [q, r] -> (theta f64 [q, r] rounded once from exact rationals, the exact row sums' check is the caller's)"""
    q, r = counts.shape
    out = np.empty((q, r))
    a = Fraction(iss) / (r * q) if method == 1 else None
    for j in range(q):
        nj = int(counts[j].sum())
        for k in range(r):
            c = int(counts[j, k])
            if method == 1:
                out[j, k] = float((c + a) / (nj + r * a))
            elif nj:
                out[j, k] = float(Fraction(c, nj))
            else:
                out[j, k] = 1.0 / r if unobserved else math.nan
    return out


def run_fit(be, data, card, masks, method, iss, unobserved, offsets=None, cpt_cells=None):
    """one dvs_bn_fit -> (rc, cpt f64 [cells] pre-filled with SENTINEL, status)"""
    B, n = masks.shape
    offsets = offsets_of(card, masks) if offsets is None else offsets
    cells = int(offsets[-1]) if cpt_cells is None else cpt_cells
    h = dict(data=be.put(sc.pack(data)), card=be.put(card), parents=be.put(masks), offsets=be.put(offsets),
             cpt=be.put(np.full(max(cells, B * n), SENTINEL)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bn_fit", batch=B, n_vars=n, n_samples=data.shape[0], method=method, iss=float(iss), unobserved=unobserved,
                 cpt_bytes=max(cells, B * n) * 8, **h)
    return rc, be.get(h["cpt"]).copy(), int(be.get(h["status"])[0])


FitCase = namedtuple("FitCase", "name data card masks refused")
SIX_CARDS = [3, 4, 16, 2, 1, 16]             # a variable with one level (constant), two with 16; variable 1 never takes its top level


@functools.lru_cache(maxsize=None)
def _six():
    return sc.synthetic_dataset(6, 1000, SIX_CARDS, seed=191, drop_top=(1,))


def six_masks():
    """B = 3, different structures: the slot lengths differ from structure to structure"""
    return sc.masks_of(6, {1: [0], 3: [2, 5], 5: [4], 2: [0, 1]}, {}, {0: [1, 3], 2: [5], 4: [0, 2], 5: [3]})


def boundary_cards():
    above = sc.level_factors(sc.smooth_neighbours(MAX_CELLS)[1])
    return [9, 16, 16, 16] + above, above


FIT_CASE_NAMES = ("single",) + tuple(f"sixS{s}" for s in ROW_COUNTS) + ("wide48", "boundary")


@functools.lru_cache(maxsize=None)
def fit_case(name):
    if name == "single":                             # n = 1, no parents
        data, card = sc.synthetic_dataset(1, 300, [5], seed=192)
        return FitCase(name, data, card, sc.masks_of(1, {}, {0: [0]}), frozenset())      # a lone self bit is ignored
    if name.startswith("sixS"):
        data, card = _six()
        return FitCase(name, data[:int(name[4:])], card, six_masks(), frozenset())
    if name == "wide48":                             # parents in all three data words of a child in the second
        rng = np.random.default_rng(193)
        data, card = sc.synthetic_dataset(48, 600, rng.integers(2, 4, 48), seed=194)
        m = sc.masks_of(48, {20: [15, 16, 17, 47], 0: [47], 47: [16]}, {15: [16, 17, 47], 33: [0, 31, 32]})
        return FitCase(name, data, card, m, frozenset())
    if name == "boundary":                           # exactly 36 864 cells, and the nearest reachable size above it
        cards, above = boundary_cards()
        data, card = sc.synthetic_dataset(len(cards), 1500, cards, seed=195)
        big = 4
        m = sc.masks_of(len(cards), {0: [1, 2, 3], big: list(range(big + 1, len(cards))), 1: [2]})
        assert sc.cells_of(card, 0, [1, 2, 3]) == MAX_CELLS < sc.cells_of(card, big, range(big + 1, len(cards))) < MAX_CELLS + 1024
        return FitCase(name, data, card, m, frozenset([(0, big)]))
    raise KeyError(name)


def _check_fit(case, cpt, status, offsets, method, iss, unobserved, refused):
    B, n = case.masks.shape
    assert status == (16 if refused else 0), (case.name, status)
    worst, saw_unobserved = 0.0, False
    for b in range(B):
        for v in range(n):
            ps, q, r = family_shape(case.card, case.masks[b, v], v)
            lo = int(offsets[b * n + v])
            hi = int(offsets[b * n + v + 1])
            got = cpt[lo:hi]
            if (b, v) in refused:
                assert (got == SENTINEL).all(), (case.name, "refused family written", b, v)
                continue
            got = got.reshape(q, r)
            counts = family_counts(case.data, case.card, case.masks[b, v], v)
            ref = fit_reference(counts, method, iss, unobserved)
            saw_unobserved |= bool((counts.sum(1) == 0).any())
            if method == 0:
                assert got.tobytes() == ref.tobytes(), (case.name, "mle", b, v, np.argwhere(got != ref)[:3])
            else:
                err = np.abs(got - ref) / ref
                assert (err <= FIT_BAYES_RTOL).all(), (case.name, "bayes", iss, b, v, float(err.max()))
                worst = max(worst, float(err.max()))
                assert (np.abs(got.sum(1) - 1.0) <= r * 2.0 ** -52).all(), (case.name, "row sums", iss, b, v)
    if cpt.size > int(offsets[-1]):
        assert (cpt[int(offsets[-1]):] == SENTINEL).all()
    return worst, saw_unobserved


def check_fit_case(be, name):
    """mle under both `unobserved` settings (equal bits) and bayes (2^-51) of one case; returns the worst bayes error"""
    case = fit_case(name)
    offsets = offsets_of(case.card, case.masks)
    worst = 0.0
    for unobserved in (0, 1):
        rc, cpt, status = run_fit(be, case.data, case.card, case.masks, 0, 1.0, unobserved)
        assert rc == 0, (name, rc)
        _, saw = _check_fit(case, cpt, status, offsets, 0, None, unobserved, case.refused)
        if name in ("sixS1", "sixS255"):
            assert saw, name                                   # these cases do have unobserved configurations
        rc, again, status2 = run_fit(be, case.data, case.card, case.masks, 0, 1.0, unobserved)
        assert rc == 0 and again.tobytes() == cpt.tobytes() and status2 == status      # two runs give equal bytes
    for iss in (ISS_VALUES if name != "boundary" else (1.0,)):
        rc, cpt, status = run_fit(be, case.data, case.card, case.masks, 1, iss, 0)
        assert rc == 0, (name, rc)
        w, _ = _check_fit(case, cpt, status, offsets, 1, iss, 0, case.refused)
        worst = max(worst, w)
    print(f"fit {name}: worst bayes relative error {worst:.3e} (allowed {FIT_BAYES_RTOL:.3e})")
    return worst


def check_fit_bad_slots(be):
    """a slot one cell too long, and a slot that ends beyond cpt_bytes: that family alone is refused"""
    case = fit_case("sixS257")
    B, n = case.masks.shape
    offsets = offsets_of(case.card, case.masks)
    fam = 1 * n + 2                                            # structure 1, variable 2
    longer = offsets.copy()
    longer[fam + 1:] += 1
    rc, cpt, status = run_fit(be, case.data, case.card, case.masks, 0, 1.0, 0, offsets=longer)
    assert rc == 0
    _check_fit(case, cpt, status, longer, 0, None, 0, frozenset([(1, 2)]))
    short = int(offsets[-1]) - 1                               # the last family's last cell is beyond the buffer
    rc, cpt, status = run_fit(be, case.data, case.card, case.masks, 0, 1.0, 0, cpt_cells=short)
    assert rc == 0 and status == 16
    lo = int(offsets[-2])
    assert (cpt[lo:short] == SENTINEL).all() and not (cpt[:lo] == SENTINEL).any()
    bit = case.masks.copy()
    bit[2, 3] |= U64(1) << U64(6)                              # a parent bit >= n_vars
    wrong = FitCase("parentbit", case.data, case.card, bit, frozenset([(2, 3)]))
    rc, cpt, status = run_fit(be, case.data, case.card, bit, 1, 1.0, 0, offsets=offsets)
    assert rc == 0
    _check_fit(wrong._replace(masks=case.masks), cpt, status, offsets, 1, 1.0, 0, wrong.refused)


# ---------------------------------------------------------------------------------------------------------------------
# 2. Forward sampling
# ---------------------------------------------------------------------------------------------------------------------
Network = namedtuple("Network", "name card masks tables")
Network.__doc__ = "card u8 [n], masks u64 [n] (one structure), tables: list of f64 [q, r]"


def thresholds(table):
    """u64 [q, r]: T_k = min(floor(c_k 2^31), 2^31), c added sequentially; 2^31 from the last positive level on"""
    q, r = table.shape
    T = np.zeros((q, r), U64)
    for j in range(q):
        c, last = 0.0, 0
        for k in range(r):
            t = float(table[j, k])
            if t > 0.0:
                last = k
            c += t
            T[j, k] = min(int(math.floor(c * 2147483648.0)), 1 << 31)
        T[j, last:] = 1 << 31
    return T


def topological_order(masks):
    n = len(masks)
    placed, order = 0, []
    while len(order) < n:
        v = next(v for v in range(n) if not (placed >> v) & 1 and not (int(masks[v]) & ~(1 << v) & ~placed))
        order.append(v)
        placed |= 1 << v
    return order


def sample_ref(net, n_rows, seed, row_offset=0):
    """u8 [n_rows, n] levels as dvs_bn_sample draws them"""
    n = len(net.card)
    g = (np.arange(n_rows, dtype=np.uint64) + U64(row_offset)) & U64(0xFFFFFFFF)
    key = orng.site_key(int(seed), SITE_BN_SAMPLE, g)
    levels = np.zeros((n_rows, n), np.uint8)
    for v in topological_order(net.masks):
        ps, q, r = family_shape(net.card, net.masks[v], v)
        T = thresholds(net.tables[v])[config_keys(levels, net.card, ps)]           # [rows, r]
        h = orng.draw(key, np.full(n_rows, v, np.uint64)) >> U64(1)
        levels[:, v] = (h[:, None] >= T[:, :r - 1]).sum(1)
    return levels


def unpack(packed, n):
    return np.stack([((packed[:, i // 16] >> U64(4 * (i % 16))) & U64(15)).astype(np.uint8) for i in range(n)], 1)


def flat_network(net):
    """(offsets i64 [n + 1], cpt f64 [cells])"""
    offsets = offsets_of(net.card, net.masks[None, :])
    return offsets, np.concatenate([t.reshape(-1) for t in net.tables])


def run_sample(be, net, n_rows, seed, row_offset=0, offsets=None, cpt=None):
    """one dvs_bn_sample -> (rc, packed u64 [n_rows, words] pre-filled with a pattern, status)"""
    n = len(net.card)
    if offsets is None:
        offsets, cpt = flat_network(net)
    n_cells = int(offsets[-1] - offsets[0])
    ws_bytes = int(be.lib.dvs_bn_sample_workspace_bytes(n_cells, n))
    assert ws_bytes >= 256 + 4 * n_cells
    h = dict(card=be.put(net.card), parents=be.put(net.masks), offsets=be.put(offsets), cpt=be.put(cpt),
             workspace=be.put(np.zeros(ws_bytes // 8 + 1, np.int64)), status=be.put(np.zeros(1, np.int32)),
             data_out=be.put(np.full((n_rows, (n + 15) // 16), 0xAAAAAAAAAAAAAAAA, U64)))
    rc = call_rc(be, "dvs_bn_sample", n_vars=n, n_rows=n_rows, n_cells=n_cells, seed=seed, row_offset=row_offset,
                 workspace_bytes=ws_bytes, **h)
    return rc, be.get(h["data_out"]).copy(), int(be.get(h["status"])[0])


def random_tables(card, masks, seed, zero_one=False):
    rng = np.random.default_rng(seed)
    tables = []
    for v in range(len(card)):
        _, q, r = family_shape(card, masks[v], v)
        t = rng.dirichlet(np.ones(r), q)
        if zero_one:                                           # exact 0 / 1 rows and rows with zeros in the middle and at both ends
            for j in range(q):
                kind = (j + v) % 4
                if kind == 0:
                    t[j] = 0.0
                    t[j, int(rng.integers(0, r))] = 1.0
                elif kind == 1 and r > 2:
                    t[j, int(rng.integers(1, r - 1))] = 0.0
                    t[j] /= t[j].sum()
                elif kind == 2 and r > 1:
                    t[j, 0] = 0.0
                    t[j, r - 1] = 0.0 if r > 2 else t[j, r - 1]
                    t[j] /= t[j].sum()
        tables.append(np.ascontiguousarray(t))
    return tables


NETWORK_NAMES = ("chain48", "zeroone", "small", "padded", "hand")


@functools.lru_cache(maxsize=None)
def network(name):
    if name == "chain48":                            # every arc from the higher to the lower index: the order is 47, 46, ..., 0
        card = np.asarray([2 + (v * 7) % 3 for v in range(48)], np.uint8)
        masks = sc.masks_of(48, {v: [v + 1] for v in range(47)})[0]
        assert topological_order(masks) == list(range(47, -1, -1))
        return Network(name, card, masks, random_tables(card, masks, 201))
    if name == "zeroone":
        card = np.asarray([3, 4, 2, 5, 16], np.uint8)
        masks = sc.masks_of(5, {1: [0], 2: [0, 1], 3: [2], 4: [3, 1]})[0]
        return Network(name, card, masks, random_tables(card, masks, 202, zero_one=True))
    if name in ("small", "padded"):                  # the same tables below the LDS budget and, one large table more, above it
        card = np.asarray(SIX_CARDS + ([16] if name == "padded" else []), np.uint8)
        dag = {1: [0], 3: [2, 5], 5: [4], 2: [0, 1], 0: [4]}
        if name == "padded":
            dag[6] = [1, 2, 5]
        masks = sc.masks_of(len(card), dag)[0]
        tables = random_tables(card[:6], masks[:6], 203)
        if name == "padded":
            tables.append(random_tables(card, masks, 204)[6])
        cells = sum(t.size for t in tables)
        assert (cells <= LDS_CELLS) == (name == "small"), cells
        return Network(name, card, masks, tables)
    if name == "hand":                               # hand-written tables: rain -> sprinkler, both -> wet
        card = np.asarray([2, 2, 2], np.uint8)
        masks = sc.masks_of(3, {1: [0], 2: [0, 1]})[0]
        tables = [np.array([[0.8, 0.2]]), np.array([[0.6, 0.4], [0.99, 0.01]]),
                  np.array([[1.0, 0.0], [0.2, 0.8], [0.1, 0.9], [0.01, 0.99]])]
        return Network(name, card, masks, tables)
    raise KeyError(name)


def check_sample(be, name, n_rows, seed=12345, row_offset=0):
    net = network(name)
    n = len(net.card)
    rc, out, status = run_sample(be, net, n_rows, seed, row_offset)
    assert rc == 0 and status == 0, (name, rc, status)
    ref = sample_ref(net, n_rows, seed, row_offset)
    assert out.tobytes() == sc.pack(ref).tobytes(), (name, n_rows, np.argwhere(unpack(out, n) != ref)[:4])
    return ref


def check_sample_zero_levels(be):
    """100 000 rows of the tables with exact 0 / 1 rows: equal bytes, and no row carries a level of probability zero"""
    net = network("zeroone")
    levels = check_sample(be, "zeroone", 100000, seed=7)
    hit = 0
    for v in range(len(net.card)):
        ps, _, _ = family_shape(net.card, net.masks[v], v)
        theta = net.tables[v][config_keys(levels, net.card, ps), levels[:, v]]
        assert (theta > 0.0).all(), (v, int((theta == 0.0).sum()))
        hit += int((net.tables[v] == 0.0).sum())
    assert hit > 20                                            # the tables do have zero cells


def check_sample_lds_and_global(be):
    """the six shared variables draw the same bytes whether the thresholds were staged in LDS or read from memory"""
    small = check_sample(be, "small", 1000, seed=99)
    padded = check_sample(be, "padded", 1000, seed=99)
    assert np.array_equal(small, padded[:, :6])


def check_sample_chunks(be):
    net = network("small")
    whole = run_sample(be, net, 1000, 5)[1]
    first, rest = run_sample(be, net, 400, 5)[1], run_sample(be, net, 600, 5, row_offset=400)[1]
    assert whole.tobytes() == np.concatenate([first, rest]).tobytes()
    assert run_sample(be, net, 1000, 6)[1].tobytes() != whole.tobytes()                # the seed matters
    hi = run_sample(be, net, 300, 5, row_offset=(1 << 32) - 100)[1]                    # g wraps at 2^32
    assert hi[100:].tobytes() == whole[:200].tobytes()


def _with_row(net, v, j, row):
    tables = [t.copy() for t in net.tables]
    tables[v][j] = row
    return net._replace(tables=tables)


def check_sample_refusals(be):
    net = network("hand")
    untouched = np.full((50, 1), 0xAAAAAAAAAAAAAAAA, U64).tobytes()
    cyc = net._replace(masks=sc.masks_of(3, {1: [0], 2: [0, 1], 0: [2]})[0], tables=[np.full((2, 2), 0.5)] + net.tables[1:])
    for bad, bit in ((cyc, 1), (_with_row(net, 1, 1, [math.nan, 0.5]), 64), (_with_row(net, 2, 3, [-0.25, 1.25]), 64),
                     (_with_row(net, 2, 0, [0.5, 0.5 + 2e-9]), 64), (_with_row(net, 2, 0, [0.5, 0.5 - 2e-9]), 64),
                     (_with_row(net, 0, 0, [math.inf, 0.0]), 64)):
        rc, out, status = run_sample(be, bad, 50, 3)
        assert rc == 0 and status == bit and out.tobytes() == untouched, (bit, status)
    for near in ([0.5, 0.5 + 1e-10], [0.5, 0.5 - 1e-10]):
        ok = _with_row(net, 2, 0, near)
        rc, out, status = run_sample(be, ok, 50, 3)
        assert rc == 0 and status == 0 and out.tobytes() == sc.pack(sample_ref(ok, 50, 3)).tobytes()
    # malformed: a slot of the wrong length, n_cells that does not match, a parent bit >= n_vars
    offsets, cpt = flat_network(net)
    wrong = offsets.copy()
    wrong[2:] += 2
    rc, out, status = run_sample(be, net, 50, 3, offsets=wrong, cpt=np.concatenate([cpt, [0.5, 0.5]]))
    assert rc == 0 and status == 16 and out.tobytes() == untouched
    bit = net._replace(masks=net.masks | np.array([0, 0, 8], U64))
    rc, out, status = run_sample(be, bit, 50, 3, offsets=offsets, cpt=cpt)
    assert rc == 0 and status == 16 and out.tobytes() == untouched


# ---------------------------------------------------------------------------------------------------------------------
# 3. Log-likelihood
# ---------------------------------------------------------------------------------------------------------------------
def _log(t):
    if t != t or t < 0.0:
        return math.nan
    return -math.inf if t == 0.0 else math.log(t)


def loglik_reference(data, card, masks, tables):
    """(per_row f64 [B, S], T [B, S]) with math.fsum of math.log; a -inf or NaN term makes the row's sum that value"""
    B, n = masks.shape
    S = data.shape[0]
    per_row, tol = np.zeros((B, S)), np.zeros((B, S))
    for b in range(B):
        terms = np.empty((S, n))
        for v in range(n):
            ps, _, _ = family_shape(card, masks[b, v], v)
            logs = np.array([[_log(float(t)) for t in row] for row in tables[b][v]])
            terms[:, v] = logs[config_keys(data, card, ps), data[:, v]]
        for s in range(S):
            row = terms[s]
            if np.isfinite(row).all():
                per_row[b, s] = math.fsum(row)
            else:
                per_row[b, s] = math.nan if np.isnan(row).any() else -math.inf
            tol[b, s] = math.fsum(np.abs(row))
    return per_row, tol


def loglik_workspace_bytes(B, n, rows, cells):
    up = lambda x: (x + 255) & ~255
    return up(B * ((rows + 255) // 256) * 8) + up(B * n * 4) + cells * 8


def run_loglik(be, data, card, masks, offsets, cpt, per_row=True, ws_bytes=None):
    """one dvs_bn_loglik -> (rc, per_row f64 [B, S] or None, out f64 [B], status)"""
    B, n = masks.shape
    S = data.shape[0]
    need = loglik_workspace_bytes(B, n, S, int(offsets[-1] - offsets[0]))
    ws_bytes = need if ws_bytes is None else ws_bytes
    h = dict(data=be.put(sc.pack(data)), card=be.put(card), parents=be.put(masks), offsets=be.put(offsets), cpt=be.put(cpt),
             workspace=be.put(np.zeros(max(need, ws_bytes) // 8 + 1, np.int64)),
             per_row=be.put(np.full((B, S), SENTINEL)) if per_row else None, out=be.put(np.full(B, SENTINEL)),
             status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bn_loglik", batch=B, n_vars=n, n_rows=S, workspace_bytes=ws_bytes, **h)
    return rc, be.get(h["per_row"]).copy() if per_row else None, be.get(h["out"]).copy(), int(be.get(h["status"])[0])


@functools.lru_cache(maxsize=None)
def loglik_inputs():
    """the six-variable data with B = 3 structures and their bayes tables (every cell positive), computed on the host"""
    data, card = _six()
    masks = six_masks()
    offsets = offsets_of(card, masks)
    cpt = np.concatenate([fit_reference(family_counts(data, card, masks[b, v], v), 1, 1.0, 0).reshape(-1)
                          for b in range(3) for v in range(6)])
    return data, card, masks, offsets, cpt


def _close(got, ref, tol, what):
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), what
    err = np.abs(got[fin] - ref[fin])
    assert (err <= LOG_RTOL * tol[fin]).all(), (what, float((err / np.maximum(tol[fin], 1e-300)).max()))
    return float((err / np.maximum(tol[fin], 1e-300)).max()) if fin.any() else 0.0


def _total(per_row, tol):
    return (np.array([math.fsum(r) if np.isfinite(r).all() else (math.nan if np.isnan(r).any() else -math.inf) for r in per_row]),
            np.array([math.fsum(t[np.isfinite(t)]) for t in tol]))


def check_loglik_rows(be, n_rows):
    data, card, masks, offsets, cpt = loglik_inputs()
    data = data[:n_rows]
    ref, tol = loglik_reference(data, card, masks, tables_of(cpt, card, masks, offsets))
    rc, rows, out, status = run_loglik(be, data, card, masks, offsets, cpt)
    assert rc == 0 and status == 0
    worst = _close(rows, ref, tol, ("per_row", n_rows))
    worst = max(worst, _close(out, *_total(ref, tol), ("out", n_rows)))
    rc, _, out2, status = run_loglik(be, data, card, masks, offsets, cpt, per_row=False)
    assert rc == 0 and status == 0 and out2.tobytes() == out.tobytes()               # per_row null: the same out bytes
    rc, rows3, out3, _ = run_loglik(be, data, card, masks, offsets, cpt)
    assert rows3.tobytes() == rows.tobytes() and out3.tobytes() == out.tobytes()     # two calls give equal bytes
    print(f"loglik rows {n_rows}: worst error / T {worst:.3e} (allowed {LOG_RTOL:.1e})")
    return worst


def check_loglik_special(be):
    """theta = 0 gives -inf, a NaN cell NaN, a level >= card and a malformed slot status bit 4 and NaN"""
    data, card, masks, offsets, cpt = loglik_inputs()
    data = data[:300]
    n = 6

    def cell(b, v, s):
        ps, _, r = family_shape(card, masks[b, v], v)
        return int(offsets[b * n + v]) + int(config_keys(data[s:s + 1], card, ps)[0]) * r + int(data[s, v])

    bad = cpt.copy()
    bad[cell(1, 3, 0)] = 0.0
    bad[cell(2, 0, 1)] = math.nan
    ref, tol = loglik_reference(data, card, masks, tables_of(bad, card, masks, offsets))
    assert ref[1, 0] == -math.inf and np.isnan(ref[2, 1]) and np.isfinite(ref[0]).all()
    rc, rows, out, status = run_loglik(be, data, card, masks, offsets, bad)
    assert rc == 0 and status == 0
    _close(rows, ref, tol, "special rows")
    assert np.isfinite(out[0]) and out[1] == -math.inf and np.isnan(out[2]), out
    # a data level >= card: that row is NaN under every structure, bit 4
    high = data.copy()
    high[7, 3] = 5
    ref, tol = loglik_reference(data, card, masks, tables_of(cpt, card, masks, offsets))
    ref[:, 7] = math.nan
    rc, rows, out, status = run_loglik(be, high, card, masks, offsets, cpt)
    assert rc == 0 and status == 16 and np.isnan(out).all()
    _close(rows, ref, tol, "level >= card")
    # a slot of the wrong length in structure 1, and a workspace too small for the tables: NaN for what cannot be read
    wrong = offsets.copy()
    wrong[n + 3:] += 1
    ref[:, 7] = loglik_reference(data[7:8], card, masks, tables_of(cpt, card, masks, offsets))[0][:, 0]
    rc, rows, out, status = run_loglik(be, data, card, masks, wrong, np.concatenate([cpt, [0.5]]))
    assert rc == 0 and status == 16 and np.isnan(out[1]) and np.isnan(rows[1]).all() and np.isfinite(out[[0]]).all()
    _close(rows[0], ref[0], tol[0], "structure before the bad slot")
    need = loglik_workspace_bytes(3, n, 300, int(offsets[-1]))
    rc, rows, out, status = run_loglik(be, data, card, masks, offsets, cpt, ws_bytes=need - 8)
    assert rc == 0 and status == 16 and np.isnan(out[2]) and np.isfinite(out[:2]).all()


def real_structures(name):
    """(data, card, masks) of asia / sachs: the golden structure (asia), the empty graph and the random DAGs of the scorer's
    corpus whose families all fit the dense table"""
    from tests import hillclimb_corpus as hc
    case = sc.bic_case(name)
    masks = [m for m in case.masks if all(sc.cells_of(case.card, v, parents_of(m[v], v)) <= MAX_CELLS for v in range(len(m)))]
    masks.append(np.zeros_like(case.masks[0]))
    if name == "asia":
        masks.insert(0, sc.masks_of(8, hc.ASIA_KNOWN)[0])
    return case.data, case.card, np.stack(masks)


def check_loglik_equals_scorer(be, name):
    """log-likelihood of the device's own mle fit on its training data = dvs_bn_scores(DVS_SCORE_LOGLIK)"""
    data, card, masks = real_structures(name)
    B, n = masks.shape
    S = data.shape[0]
    offsets = offsets_of(card, masks)
    rc, cpt, status = run_fit(be, data, card, masks, 0, 1.0, 0)
    assert rc == 0 and status == 0
    rc, _, out, status = run_loglik(be, data, card, masks, offsets, cpt, per_row=False)
    assert rc == 0 and status == 0
    d, c, m = be.put(sc.pack(data)), be.put(card), be.put(masks)
    scratch, score, st = be.put(np.zeros((B, n))), be.put(np.zeros(B)), be.put(np.zeros(1, np.int32))
    rc = call_rc(be, "dvs_bn_scores", batch=B, n_vars=n, n_samples=S, data=d, card=c, parents=m, score_type=0,
                 score_arg=float("nan"), scratch=scratch, out=score, status=st)
    score = be.get(score).copy()
    assert rc == 0 and int(be.get(st)[0]) == 0
    for b in range(B):
        T = 0.0
        for v in range(n):
            counts = family_counts(data, card, masks[b, v], v).astype(np.float64)
            nj = counts.sum(1, keepdims=True)
            occ = counts > 0
            T += float((counts[occ] * np.abs(np.log((counts / np.where(nj > 0, nj, 1.0))[occ]))).sum())
        assert abs(out[b] - score[b]) <= LOG_RTOL * 2 * T, (name, b, out[b], score[b], T)
        assert T > 0 and out[b] < 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []

    nan, inf = float("nan"), float("inf")
    c = entry("dvs_bn_fit", cases, batch=4, n_vars=12, n_samples=100, data=D, card=D, parents=D, method=1, iss=1.0,
              unobserved=0, offsets=D, cpt=D, cpt_bytes=384, status=D, stream=None)
    c(2, "batch and n_samples must be > 0", batch=0)
    c(2, "batch and n_samples must be > 0", n_samples=0)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars must be < 2^31", batch=1 << 30, n_vars=48, cpt_bytes=1 << 50)
    c(12, "method is not a dvs_fit_method", method=2)
    c(12, "method is not a dvs_fit_method", method=-1)
    for bad in (0.0, -1.0, nan, inf):
        c(13, "iss must be finite and > 0", iss=bad)
    c(12, "unobserved must be 0 (NaN) or 1 (uniform)", unobserved=2)
    for name in ("data", "card", "parents", "offsets", "cpt", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "cpt_bytes < batch * n_vars * 8 = 384", cpt_bytes=383)
    c(2, "batch and n_samples must be > 0", batch=0, n_vars=49)                        # sizes before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, method=9)                             # n_vars before the method
    c(12, "method is not a dvs_fit_method", method=9, iss=nan)                         # the method before iss
    c(13, "iss must be finite and > 0", iss=nan, unobserved=2)                         # iss before unobserved
    c(12, "unobserved must be", unobserved=2, data=None)                               # unobserved before null
    c(10, "null pointer", status=None, cpt_bytes=0)                                    # null before cpt_bytes

    c = entry("dvs_bn_sample", cases, n_vars=12, n_rows=1000, card=D, parents=D, offsets=D, cpt=D, n_cells=100, seed=7,
              row_offset=0, workspace=D, workspace_bytes=768, data_out=D, status=D, stream=None)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=1 << 31)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=11)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=1 << 31, workspace_bytes=1 << 40)
    c(12, "row_offset must be >= 0", row_offset=-1)
    for name in ("card", "parents", "offsets", "cpt", "workspace", "data_out", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "workspace_bytes < dvs_bn_sample_workspace_bytes = 768", workspace_bytes=767)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0, n_vars=49)                       # n_rows before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, n_cells=0)                            # n_vars before n_cells
    c(2, "n_cells must be in", n_cells=0, row_offset=-1)                               # n_cells before row_offset
    c(12, "row_offset must be >= 0", row_offset=-1, card=None)                         # row_offset before null
    c(10, "null pointer", status=None, workspace_bytes=0)                              # null before workspace_bytes

    c = entry("dvs_bn_loglik", cases, batch=3, n_vars=6, n_rows=300, data=D, card=D, parents=D, offsets=D, cpt=D,
              per_row=None, out=D, workspace=D, workspace_bytes=656, status=D, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31", batch=1 << 30, n_vars=48, workspace_bytes=1 << 50)
    c(2, "batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31", batch=1 << 20, n_rows=1 << 30, workspace_bytes=1 << 50)
    for name in ("data", "card", "parents", "offsets", "cpt", "out", "workspace", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "workspace_bytes < partials + flags + batch * n_vars * 8 = 656", workspace_bytes=655)
    c(2, "batch must be > 0", batch=0, n_rows=0)                                       # batch before n_rows
    c(2, "n_rows must be in", n_rows=0, n_vars=49)                                     # n_rows before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, data=None)                            # n_vars before null
    c(10, "null pointer", status=None, workspace_bytes=0)                              # null before workspace_bytes
    return cases


def check_argument_refusals(lib, D):
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_bn_fit", "dvs_bn_sample", "dvs_bn_loglik"}
    run(lib, cases)
    # the fourth entry point returns a size: 0 and the reason for arguments out of range
    assert lib.dvs_bn_sample_workspace_bytes(100, 12) == 768 and lib.dvs_bn_sample_workspace_bytes(12, 12) == 512
    for n_cells, n_vars, text in ((100, 0, "n_vars must be in [1, 48]"), (100, 49, "n_vars must be in [1, 48]"),
                                  (11, 12, "n_cells must be in [n_vars, 2^31 - 1]"), (1 << 31, 12, "n_cells must be in")):
        assert lib.dvs_bn_sample_workspace_bytes(n_cells, n_vars) == 0
        msg = lib.dvs_last_error().decode()
        assert msg.startswith("dvs_bn_sample_workspace_bytes:") and text in msg, msg
    # mle takes no iss: any number passes the argument checks (the next failing check decides)
    assert call_rc(sc.EmuBackend(lib), "dvs_bn_fit", batch=4, n_vars=12, n_samples=100, data=D, card=D, parents=D, method=0,
                   iss=float("nan"), unobserved=0, offsets=D, cpt=D, cpt_bytes=0, status=D) == 14      # dummy pointers, null stream


# ---------------------------------------------------------------------------------------------------------------------
# 5. cross_validate restated (numpy)
# ---------------------------------------------------------------------------------------------------------------------
def cv_permutation(n_rows, seed):
    """the row permutation of cross_validate: numpy's default_rng(seed).permutation"""
    return np.random.default_rng(seed).permutation(n_rows)


def cv_reference(data, card, masks, folds, seed, method, iss):
    """(loss f64 [B], T [B]): -(sum over folds of the held-out log-likelihood) / S under the tables fitted on the rest"""
    S = data.shape[0]
    perm = cv_permutation(S, seed)
    B, n = masks.shape
    total, tol = [[] for _ in range(B)], [[] for _ in range(B)]
    for f in range(folds):
        lo, hi = f * S // folds, (f + 1) * S // folds
        test, train = data[perm[lo:hi]], data[np.concatenate([perm[:lo], perm[hi:]])]
        tables = [[fit_reference(family_counts(train, card, masks[b, v], v), method, iss, 0) for v in range(n)] for b in range(B)]
        rows, t = loglik_reference(test, card, masks, tables)
        for b in range(B):
            total[b].extend(rows[b])
            tol[b].extend(t[b])
    tot, T = _total(np.asarray(total), np.asarray(tol))
    return -tot / S, T / S
