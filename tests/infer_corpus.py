"""TEST HELPER: cases, references and the checks themselves for the inference calls of csrc/dvs_infer.h (dvs_bn_lw,
dvs_bn_lw_workspace_bytes, dvs_bn_blanket_posterior; definitions in include/dvs.h).  Plain numpy, no GPU:
tests/test_emu_infer.py (emulator build) and tests/test_gpu_infer.py (device) run the same checks and differ only in the
backend that moves buffers (tests/scoring_corpus.py); tests/test_infer_ref.py checks the restatements themselves against
brute-force enumeration of the joint distribution.  The networks are those of tests/params_corpus.py.

References
  lw        lw_ref: the draws (oracle.rng.site_key / draw, site 501), the thresholds, the weight products in the preparation's
            order and the summation order of include/dvs.h restated as they are; the kernels must give the same bytes.
  blanket   blanket_ref: the fp64 products in the stated order, the sum in ascending level, one division per cell: the same
            bytes again.  The restatement itself is checked against exact rationals of the same tables.

Tolerances are derived, not measured.
  blanket against enumeration   a posterior cell is a product of f factors (f - 1 roundings), divided (1 rounding) by a sum of
            r such non-negative products (r - 1 more roundings, and each term's own f - 1): relative error below
            (2 f + r) * 2^-53 to first order.  Asserted: BLANKET_ULPS_PER_FACTOR = 4 half-ulps per factor and level, i.e.
            (f + r) * 4 * 2^-53 — the "few ulp per factor" next to params_corpus.FIT_BAYES_RTOL = 2^-51.
  lw against the exact posterior   5 standard errors (the issue's bound), the standard error from the enumeration: with
            q(x) the proposal (product of the unobserved variables' thetas), w(x) the weight (product of the observed ones'),
            the estimate sum w e / sum w of P(e | evidence) = mu has the delta-method variance
            E_q[w^2 (e - mu)^2] / (M E_q[w]^2).  Preconditions asserted here, so a bad case fails on the CPU: every checked
            cell lies in [0.05, 0.95] and the exact effective sample size M E_q[w]^2 / E_q[w^2] is >= 400.
"""
import ctypes
import functools
import itertools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from oracle import rng as orng
from tests import params_corpus as pm
from tests import scoring_corpus as sc
from tests.abi_cases import call_rc, entry, run

U64 = np.uint64
SITE_BN_LW = 501
SENTINEL = pm.SENTINEL
PARTICLE_COUNTS = (1, 255, 256, 257, 1000)
ROW_COUNTS = pm.ROW_COUNTS
BLANKET_ULPS_PER_FACTOR = 4.0 * 2.0 ** -53       # see above; params_corpus.FIT_BAYES_RTOL is 2^-51 for one cell of five roundings
STAT_PARTICLES = 4096
STAT_SIGMAS = 5.0
STAT_MIN_ESS = 400.0
STAT_CELL_RANGE = (0.05, 0.95)


# ---------------------------------------------------------------------------------------------------------------------
# The summation order of include/dvs.h
# ---------------------------------------------------------------------------------------------------------------------
def _tree(x):
    """x f64 [..., 256] -> [...]: x[i] += x[i + s] for s = 128, ..., 1"""
    x = x.copy()
    s = 128
    while s:
        x[..., :s] = x[..., :s] + x[..., s:2 * s]
        s >>= 1
    return x[..., 0]


def ordered_sum(values):
    """values f64 [..., M] -> [...] in the order of dvs_bn_lw: a tree over the 256 slots of each chunk of 256 (absent
    particles +0), slot t adding the chunk sums t, t + 256, ... in ascending order from +0, then the same tree"""
    values = np.asarray(values, np.float64)
    M = values.shape[-1]
    chunks = (M + 255) // 256
    x = np.zeros(values.shape[:-1] + (chunks * 256,))
    x[..., :M] = values
    part = _tree(x.reshape(values.shape[:-1] + (chunks, 256)))              # [..., chunks]
    slots = np.zeros(values.shape[:-1] + (256,))
    for c in range(chunks):
        slots[..., c % 256] = slots[..., c % 256] + part[..., c]
    return _tree(slots)


# ---------------------------------------------------------------------------------------------------------------------
# 1. Likelihood weighting
# ---------------------------------------------------------------------------------------------------------------------
def thresholds_fast(table):
    """pm.thresholds, vectorised (np.cumsum adds sequentially in fp64, as the kernel does)"""
    c = np.cumsum(table, axis=1)
    T = np.minimum(np.floor(c * 2147483648.0), 2147483648.0).astype(U64)
    pos = table > 0.0
    last = np.where(pos.any(1), table.shape[1] - 1 - np.argmax(pos[:, ::-1], axis=1), 0)
    T[np.arange(table.shape[1])[None, :] >= last[:, None]] = 1 << 31
    return T


def _thresholds(net):
    """per call, not cached: the networks of cv_pred_reference are short-lived and an id-keyed cache could go stale"""
    return [thresholds_fast(t) for t in net.tables]


def targets_of(mask):
    return sc.mask_bits(mask)


LwRef = namedtuple("LwRef", "levels weights sums marginals bad")


def lw_ref(net, evidence, observed, M, seed, query_offset=0, event=None, targets=0):
    """evidence u8 [Q, n] levels, observed [Q] ints -> LwRef(levels u8 [Q, M, n], weights f64 [Q, M], sums [Q, 3],
    marginals [Q, T, 16], bad bool [Q]) as dvs_bn_lw computes them"""
    n = len(net.card)
    Q = len(observed)
    order = pm.topological_order(net.masks)
    thr = _thresholds(net)
    tg = targets_of(targets)
    levels = np.zeros((Q, M, n), np.uint8)
    weights = np.ones((Q, M))
    sums = np.zeros((Q, 3))
    marg = np.zeros((Q, len(tg), 16))
    bad = np.zeros(Q, bool)
    p = np.arange(M, dtype=np.uint64)
    for q in range(Q):
        obs = int(observed[q])
        if obs >> n or any((obs >> v) & 1 and int(evidence[q, v]) >= int(net.card[v]) for v in range(n)):
            bad[q] = True
            levels[q], weights[q], sums[q], marg[q] = 0, math.nan, math.nan, math.nan
            continue
        key = orng.site_key(int(seed), SITE_BN_LW, np.uint64((query_offset + q) & 0xFFFFFFFF))
        lv, w = levels[q], weights[q]
        for v in order:
            ps, _, r = pm.family_shape(net.card, net.masks[v], v)
            cfg = pm.config_keys(lv, net.card, ps)
            if (obs >> v) & 1:
                lv[:, v] = evidence[q, v]
                w *= net.tables[v][cfg, int(evidence[q, v])]
            else:
                h = orng.draw(orng.draw(key, np.uint64(v)), p) >> U64(1)
                lv[:, v] = (h[:, None] >= thr[v][cfg][:, :r - 1]).sum(1)
        inside = np.ones(M, bool)
        if event is not None:
            for v in range(n):
                inside &= ((int(event[v]) >> lv[:, v].astype(np.int64)) & 1).astype(bool)
        sums[q] = [ordered_sum(w), ordered_sum(w * w), ordered_sum(np.where(inside, w, 0.0))]
        for t, v in enumerate(tg):
            for k in range(int(net.card[v])):
                marg[q, t, k] = ordered_sum(np.where(lv[:, v] == k, w, 0.0))
    return LwRef(levels, weights, sums, marg, bad)


def pack_levels(levels):
    """u8 [..., n] -> u64 [..., words]"""
    shape = levels.shape[:-1]
    return sc.pack(levels.reshape(-1, levels.shape[-1])).reshape(shape + (-1,))


LwOut = namedtuple("LwOut", "rc sums marginals particles weights status")


def run_lw(be, net, evidence, observed, M, seed, query_offset=0, event=None, targets=0, want_particles=True, offsets=None,
           cpt=None, ws_bytes=None):
    """one dvs_bn_lw; every output pre-filled (SENTINEL, a word pattern) so that an untouched cell shows"""
    n = len(net.card)
    Q = len(observed)
    words = (n + 15) // 16
    if offsets is None:
        offsets, cpt = pm.flat_network(net)
    n_cells = int(offsets[-1] - offsets[0])
    T = len(targets_of(targets))
    need = int(be.lib.dvs_bn_lw_workspace_bytes(n_cells, n, Q, M, targets))
    up = lambda x: (x + 255) & ~255
    assert need == 256 + up(4 * n_cells) + up(4 * Q) + up(Q * ((M + 255) // 256) * (3 + 16 * T) * 8), need
    ws_bytes = need if ws_bytes is None else ws_bytes
    h = dict(card=be.put(net.card), parents=be.put(net.masks), offsets=be.put(offsets), cpt=be.put(cpt),
             evidence=be.put(pack_levels(np.asarray(evidence, np.uint8))), observed=be.put(np.asarray([int(o) for o in observed], U64)),
             event=be.put(np.asarray(event, np.uint16)) if event is not None else None,
             workspace=be.put(np.zeros(max(need, ws_bytes) // 8 + 1, np.int64)), sums=be.put(np.full((Q, 3), SENTINEL)),
             marginals=be.put(np.full((Q, T, 16), SENTINEL)) if T else None,
             particles=be.put(np.full((Q, M, words), 0xAAAAAAAAAAAAAAAA, U64)) if want_particles else None,
             particle_weights=be.put(np.full((Q, M), SENTINEL)) if want_particles else None, status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bn_lw", n_vars=n, n_queries=Q, n_particles=M, n_cells=n_cells, targets=targets, seed=seed,
                 query_offset=query_offset, workspace_bytes=ws_bytes, **h)
    get = lambda k: be.get(h[k]).copy() if h[k] is not None else None
    return LwOut(rc, get("sums"), get("marginals"), get("particles"), get("particle_weights"), int(be.get(h["status"])[0]))


def _same(got, ref, what):
    assert got.tobytes() == np.ascontiguousarray(ref).tobytes(), (what, np.argwhere(~((got == ref) | ((got != got) & (ref != ref))))[:4])


def assert_lw_equal(out, ref, what, particles=True):
    assert out.rc == 0, (what, out.rc)
    _same(out.sums, ref.sums, (what, "sums"))
    if out.marginals is not None:
        _same(out.marginals, ref.marginals, (what, "marginals"))
    if particles and out.particles is not None:
        _same(out.particles, pack_levels(ref.levels), (what, "particles"))
        _same(out.weights, ref.weights, (what, "weights"))


LW_NETWORKS = ("hand", "small", "six", "zeroone", "chain48")


@functools.lru_cache(maxsize=None)
def lw_network(name):
    """`six`: the six-variable set with two 16-level variables and a one-level variable (`small` has the same variables; here
    the 16-level ones are parent and child of each other and of the one-level variable)"""
    if name == "six":
        card = np.asarray(pm.SIX_CARDS, np.uint8)
        masks = sc.masks_of(6, {5: [2], 4: [2], 3: [4, 5], 1: [0, 3]})[0]
        return pm.Network(name, card, masks, pm.random_tables(card, masks, 401))
    return pm.network(name)


# per network: (observed mask of the mixed query, targets, event as {variable: levels})
LW_SETUP = {
    "hand": (0b100, 0b011, {0: [1]}),
    "small": (0b101010, 0b111111, {0: [0, 2], 2: [1, 3, 5, 7, 15]}),
    "six": (0b100101, 0b111111, {5: list(range(8)), 1: [0, 1]}),
    "zeroone": (0b01010, 0b11111, {4: list(range(0, 16, 2)), 0: [0, 1]}),
    "chain48": ((1 << 3) | (1 << 20) | (1 << 41), (1 << 0) | (1 << 17) | (1 << 40) | (1 << 47), {2: [0], 19: [0, 1], 44: [1]}),
}


def event_words(n, event):
    words = np.full(n, 0xFFFF, np.uint16)
    for v, ks in event.items():
        words[v] = sum(1 << k for k in ks)
    return words


def lw_queries(name, Q):
    """(evidence u8 [Q, n], observed): rows drawn from the network itself, so the evidence has positive probability.
    Q = 1: the mixed mask; Q = 3: nothing observed, everything observed, the mixed mask"""
    net = lw_network(name)
    n = len(net.card)
    mixed = LW_SETUP[name][0]
    rows = pm.sample_ref(net, 3, seed=77)
    return (rows[:1], [mixed]) if Q == 1 else (rows, [0, (1 << n) - 1, mixed])


def check_lw_case(be, name, M, seed=2024):
    """bytes of particles, weights, sums and marginals; the sums with and without the optional outputs; event null and not"""
    net = lw_network(name)
    n = len(net.card)
    _, targets, event = LW_SETUP[name]
    ev_words = event_words(n, event)
    for Q in (1, 3):
        evidence, observed = lw_queries(name, Q)
        ref = lw_ref(net, evidence, observed, M, seed, 5, None, targets)
        full = run_lw(be, net, evidence, observed, M, seed, 5, None, targets, True)
        info = 128 if (ref.sums[:, 0] == 0.0).any() else 0                       # a query whose weights sum to zero: bit 7
        assert full.status == info, (name, M, Q, full.status)
        assert_lw_equal(full, ref, (name, M, Q))
        _same(full.sums[:, 2], full.sums[:, 0], "event null: the third sum is the first")
        bare = run_lw(be, net, evidence, observed, M, seed, 5, None, 0, False)
        assert bare.rc == 0 and bare.status == info
        _same(bare.sums, full.sums, (name, M, Q, "sums without the optional outputs"))
        refe = lw_ref(net, evidence, observed, M, seed, 5, ev_words, targets)
        with_event = run_lw(be, net, evidence, observed, M, seed, 5, ev_words, targets, False)
        assert with_event.status == info
        assert_lw_equal(with_event, refe, (name, M, Q, "event"))
        if Q == 3:
            assert (ref.weights[0] == 1.0).all()                                  # nothing observed: every weight exactly 1
            assert (ref.levels[1] == evidence[1]).all() and len(set(ref.weights[1].tolist())) == 1   # everything observed
            w = 1.0
            for v in pm.topological_order(net.masks):
                ps, _, _ = pm.family_shape(net.card, net.masks[v], v)
                w *= net.tables[v][int(pm.config_keys(evidence[1:2], net.card, ps)[0]), int(evidence[1, v])]
            assert ref.weights[1, 0] == w > 0.0
            assert 0 < refe.sums[0, 2] < refe.sums[0, 0] or M < 20               # the event does cut something
    again = run_lw(be, net, evidence, observed, M, seed, 5, None, targets, True)
    assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(again[1:5], full[1:5]))     # two runs give equal bytes


def check_lw_zero_theta(be):
    """zeroone: evidence on a level of probability zero gives weight exactly 0 (and +0 cells), and no particle ever carries an
    unobserved level of probability zero"""
    net = lw_network("zeroone")
    n = len(net.card)
    base = pm.sample_ref(net, 1, seed=5)[0]
    v = 3                                                                        # child of 2
    j = next(j for j in range(net.tables[v].shape[0]) if (net.tables[v][j] == 0.0).any())
    k = int(np.argmin(net.tables[v][j]))
    ev = base.copy()
    ev[2], ev[v] = j, k
    evidence, observed = np.stack([ev, ev]), [(1 << 2) | (1 << v), 1 << v]
    M = 600
    ref = lw_ref(net, evidence, observed, M, 9, 0, None, 0b11111)
    out = run_lw(be, net, evidence, observed, M, 9, 0, None, 0b11111, True)
    assert_lw_equal(out, ref, "zero theta")
    assert out.status == 128 and (out.weights[0] == 0.0).all() and not np.signbit(out.sums[0]).any() and (out.sums[0] == 0.0).all()
    assert (out.marginals[0] == 0.0).all() and out.sums[1, 0] > 0.0 and (out.weights[1] == 0.0).any()
    lv = ref.levels[1]
    for u in range(n):
        if u != v:
            ps, _, _ = pm.family_shape(net.card, net.masks[u], u)
            assert (net.tables[u][pm.config_keys(lv, net.card, ps), lv[:, u]] > 0.0).all(), u


def _geometry_queries(net, Q, seed):
    n = len(net.card)
    evidence = pm.sample_ref(net, Q, seed=seed)
    rng = np.random.default_rng(seed)
    observed = [int(x) for x in rng.integers(0, 1 << n, Q)]
    observed[0], observed[1] = 0, (1 << n) - 1
    return evidence, observed


def check_lw_query_offset(be):
    """Q = 300 x M = 300 in one call = each query alone with query_offset = q; and enough work items (Q x chunks) that a
    workgroup walks more than one"""
    net = lw_network("small")
    evidence, observed = _geometry_queries(net, 300, 31)
    ev_words = event_words(6, LW_SETUP["small"][2])
    whole = run_lw(be, net, evidence, observed, 300, 17, 0, ev_words, 0b111111, True)
    assert whole.rc == 0 and whole.status == 0
    for q in range(300):
        one = run_lw(be, net, evidence[q:q + 1], observed[q:q + 1], 300, 17, q, ev_words, 0b111111, True)
        assert one.rc == 0 and one.status == 0
        for a, b in zip(one[1:5], whole[1:5]):
            assert a[0].tobytes() == b[q].tobytes(), q
    ref = lw_ref(net, evidence[:4], observed[:4], 300, 17, 0, ev_words, 0b111111)
    for a, b in zip((whole.sums[:4], whole.marginals[:4], whole.weights[:4]), (ref.sums, ref.marginals, ref.weights)):
        _same(a, b, "Q = 300")
    evidence, observed = _geometry_queries(net, 2500, 32)
    many = run_lw(be, net, evidence, observed, 2, 17, 0, None, 0b000101, False)
    first = run_lw(be, net, evidence[:1200], observed[:1200], 2, 17, 0, None, 0b000101, False)
    rest = run_lw(be, net, evidence[1200:], observed[1200:], 2, 17, 1200, None, 0b000101, False)
    assert many.rc == first.rc == rest.rc == 0
    _same(many.sums, np.concatenate([first.sums, rest.sums]), "cut into calls")
    _same(many.marginals, np.concatenate([first.marginals, rest.marginals]), "cut into calls")
    _same(many.sums[-3:], lw_ref(net, evidence[-3:], observed[-3:], 2, 17, 2497, None, 0).sums, "the last queries")
    wrap = run_lw(be, net, evidence[:3], observed[:3], 2, 17, (1 << 32) - 1, None, 0, False)      # g wraps at 2^32
    _same(wrap.sums[1:], run_lw(be, net, evidence[1:3], observed[1:3], 2, 17, 0, None, 0, False).sums, "wrap")


def check_lw_lds_and_global(be):
    """the six shared variables give the same bytes whether the thresholds were staged in LDS or read from memory"""
    small, padded = pm.network("small"), pm.network("padded")
    assert sum(t.size for t in padded.tables) > pm.LDS_CELLS >= sum(t.size for t in small.tables)
    evidence, observed = _geometry_queries(small, 3, 33)
    wide = np.concatenate([evidence, np.zeros((3, 1), np.uint8)], 1)
    ev_words = event_words(6, LW_SETUP["small"][2])
    a = run_lw(be, small, evidence, observed, 700, 3, 0, ev_words, 0b111111, True)
    b = run_lw(be, padded, wide, observed, 700, 3, 0, np.append(ev_words, np.uint16(0xFFFF)), 0b111111, True)
    assert a.rc == b.rc == 0 and a.status == b.status == 0
    _same(a.sums, b.sums, "sums")
    _same(a.marginals, b.marginals, "marginals")
    _same(a.weights, b.weights, "weights")
    mask6 = U64((1 << 24) - 1)
    assert np.array_equal(a.particles[..., 0] & mask6, b.particles[..., 0] & mask6)
    assert_lw_equal(b, lw_ref(padded, wide, observed, 700, 3, 0, np.append(ev_words, np.uint16(0xFFFF)), 0b111111), "padded")


def _untouched(out):
    return ((out.sums == SENTINEL).all() and (out.marginals == SENTINEL).all() and (out.weights == SENTINEL).all()
            and (out.particles == U64(0xAAAAAAAAAAAAAAAA)).all())


def check_lw_refusals(be):
    net = pm.network("hand")
    evidence, observed = np.array([[0, 0, 1], [1, 1, 1], [0, 1, 0]], np.uint8), [0b100, 0b111, 0]
    cyc = net._replace(masks=sc.masks_of(3, {1: [0], 2: [0, 1], 0: [2]})[0], tables=[np.full((2, 2), 0.5)] + net.tables[1:])
    for bad, bit in ((cyc, 1), (pm._with_row(net, 1, 1, [math.nan, 0.5]), 64), (pm._with_row(net, 2, 0, [0.5, 0.5 + 2e-9]), 64)):
        out = run_lw(be, bad, evidence, observed, 300, 3, 0, None, 0b011, True)
        assert out.rc == 0 and out.status == bit and _untouched(out), (bit, out.status)
    offsets, cpt = pm.flat_network(net)
    wrong = offsets.copy()
    wrong[2:] += 2                                                               # a slot of the wrong length
    out = run_lw(be, net, evidence, observed, 300, 3, 0, None, 0b011, True, offsets=wrong, cpt=np.concatenate([cpt, [0.5, 0.5]]))
    assert out.rc == 0 and out.status == 16 and _untouched(out)
    # an evidence level >= card: that query alone is NaN
    high = evidence.copy()
    high[1, 1] = 2
    ref = lw_ref(net, high, observed, 300, 3, 0, None, 0b011)
    assert ref.bad.tolist() == [False, True, False]
    out = run_lw(be, net, high, observed, 300, 3, 0, None, 0b011, True)
    assert out.status == 16 and np.isnan(out.sums[1]).all() and np.isnan(out.marginals[1]).all() and np.isnan(out.weights[1]).all()
    assert_lw_equal(out, ref, "level >= card")
    unread = evidence.copy()
    unread[2] = 9                                                                # nothing observed: the row is not read
    assert run_lw(be, net, unread, observed, 300, 3, 0, None, 0b011, True).status == 0
    out = run_lw(be, net, evidence, [0b100, 0b1111, 0], 300, 3, 0, None, 0b011, True)        # an observed bit >= n_vars
    assert out.status == 16 and np.isnan(out.sums[1]).all() and np.isfinite(out.sums[[0, 2]]).all()
    # impossible evidence: wet without rain or sprinkler has probability zero
    imp = np.array([[0, 0, 1], [0, 0, 0]], np.uint8)
    out = run_lw(be, net, imp, [0b111, 0b111], 257, 3, 0, None, 0b011, True)
    assert out.rc == 0 and out.status == 128, out.status
    assert out.sums[0].tobytes() == np.zeros(3).tobytes() and out.marginals[0].tobytes() == np.zeros((2, 16)).tobytes()
    assert (out.weights[0] == 0.0).all() and out.sums[1, 0] > 0
    assert_lw_equal(out, lw_ref(net, imp, [7, 7], 257, 3, 0, None, 0b011), "impossible evidence")


# ---------------------------------------------------------------------------------------------------------------------
# 2. The exact posterior of one variable given all the others
# ---------------------------------------------------------------------------------------------------------------------
def children_of(masks, t):
    return [c for c in range(len(masks)) if c != t and (int(masks[c]) >> t) & 1]


def blanket_ref(data, card, masks, tables, target, use_children):
    """data u8 [S, n], masks u64 [n], tables of ONE structure -> (posterior f64 [S, r], pred u8 [S]) as the kernel computes
    them: theta_t(k | pa), times the children in ascending id, the sum in ascending k from +0, one division"""
    S, r = data.shape[0], int(card[target])
    prod = np.empty((S, r))
    for k in range(r):
        x = data.copy()
        x[:, target] = k
        ps, _, _ = pm.family_shape(card, masks[target], target)
        p = tables[target][pm.config_keys(x, card, ps), k].copy()
        if use_children:
            for c in children_of(masks, target):
                ps, _, _ = pm.family_shape(card, masks[c], c)
                p *= tables[c][pm.config_keys(x, card, ps), x[:, c]]
        prod[:, k] = p
    total = np.zeros(S)
    for k in range(r):
        total = total + prod[:, k]
    with np.errstate(invalid="ignore", divide="ignore"):
        post = prod / total[:, None]
    pred = np.argmax(post, axis=1).astype(np.uint8)                              # the first of the maxima
    pred[np.isnan(post).any(1)] = 255
    return post, pred


BlanketOut = namedtuple("BlanketOut", "rc posterior pred status")


def run_blanket(be, data, card, masks, offsets, cpt, target, use_children, want_posterior=True, cpt_bytes=None):
    B, n = masks.shape
    S, r = data.shape[0], int(card[target])
    h = dict(data=be.put(sc.pack(data)), card=be.put(card), parents=be.put(masks), offsets=be.put(offsets), cpt=be.put(cpt),
             posterior=be.put(np.full((B, S, r), SENTINEL)) if want_posterior else None,
             pred=be.put(np.full((B, S), 77, np.uint8)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, "dvs_bn_blanket_posterior", batch=B, n_vars=n, n_rows=S, target=target, use_children=use_children,
                 cpt_bytes=cpt.size * 8 if cpt_bytes is None else cpt_bytes, **h)
    post = be.get(h["posterior"]).copy() if want_posterior else None
    return BlanketOut(rc, post, be.get(h["pred"]).copy(), int(be.get(h["status"])[0]))


@functools.lru_cache(maxsize=None)
def bayes_fit(name, iss=10.0, structures=3):
    """(data, card, masks [B, n], offsets, cpt): asia / sachs with the first structures of params_corpus.real_structures,
    bayes tables with iss computed on the host (every cell positive)"""
    data, card, masks = pm.real_structures(name)
    masks = masks[:structures]
    B, n = masks.shape
    offsets = pm.offsets_of(card, masks)
    cpt = np.concatenate([pm.fit_reference(pm.family_counts(data, card, masks[b, v], v), 1, iss, 0).reshape(-1)
                          for b in range(B) for v in range(n)])
    return data, card, masks, offsets, cpt


def check_blanket_rows(be, name, n_rows):
    """every target, both use_children values: posterior and pred equal the numpy products byte for byte"""
    data, card, masks, offsets, cpt = bayes_fit(name)
    data = data[:n_rows]
    B, n = masks.shape
    tables = pm.tables_of(cpt, card, masks, offsets)
    for target in range(n):
        for use_children in (0, 1):
            out = run_blanket(be, data, card, masks, offsets, cpt, target, use_children)
            assert out.rc == 0 and out.status == 0, (name, target, out.rc, out.status)
            for b in range(B):
                post, pred = blanket_ref(data, card, masks[b], tables[b], target, use_children)
                _same(out.posterior[b], post, (name, n_rows, target, use_children, b))
                _same(out.pred[b], pred, (name, n_rows, target, use_children, b, "pred"))
        bare = run_blanket(be, data, card, masks, offsets, cpt, target, 1, want_posterior=False)
        _same(bare.pred, out.pred, "pred without the posterior")
    other = data.copy()
    other[:, 0] = 15                                                             # the target's own column is ignored
    _same(run_blanket(be, other, card, masks, offsets, cpt, 0, 1).posterior,
          run_blanket(be, data, card, masks, offsets, cpt, 0, 1).posterior, "target column")


def check_blanket_special(be):
    """ties go to the lowest level; an all-zero row and a NaN cell give NaN and 255; a level >= card and a malformed slot set
    bit 4"""
    net = pm.network("hand")
    masks = net.masks[None, :]
    offsets, cpt = pm.flat_network(net)
    data = np.array(list(itertools.product(range(2), repeat=3)), np.uint8)[:, ::-1].copy()
    tie = [t.copy() for t in net.tables]
    tie[0][0] = [0.5, 0.5]
    out = run_blanket(be, data, net.card, masks, offsets, np.concatenate([t.reshape(-1) for t in tie]), 0, 0)
    assert out.status == 0 and (out.pred == 0).all() and (out.posterior == 0.5).all()
    # wet = 1 without rain or sprinkler: with sprinkler as the target the row (rain 0, wet 1) is possible only for sprinkler 1;
    # with tables in which it is impossible for both levels every product is zero
    zero = [t.copy() for t in net.tables]
    zero[2][2] = [1.0, 0.0]
    zcpt = np.concatenate([t.reshape(-1) for t in zero])
    out = run_blanket(be, data, net.card, masks, offsets, zcpt, 1, 1)
    post, pred = blanket_ref(data, net.card, net.masks, zero, 1, 1)
    _same(out.posterior[0], post, "all-zero row")
    _same(out.pred[0], pred, "all-zero row pred")
    hit = (data[:, 0] == 0) & (data[:, 2] == 1)
    assert out.status == 0 and np.isnan(out.posterior[0][hit]).all() and (out.pred[0][hit] == 255).all() and (out.pred[0][~hit] < 2).all()
    nan = cpt.copy()
    nan[2:4] = math.nan                                                          # sprinkler's table, configuration rain = 0
    out = run_blanket(be, data, net.card, masks, offsets, nan, 0, 1)
    assert out.status == 0 and (out.pred[0] == 255).all() and np.isnan(out.posterior).all()
    high = data.copy()
    high[3, 2] = 2
    out = run_blanket(be, high, net.card, masks, offsets, cpt, 0, 1)
    post, pred = blanket_ref(data, net.card, net.masks, net.tables, 0, 1)
    post[3], pred[3] = math.nan, 255
    assert out.status == 16
    _same(out.posterior[0], post, "level >= card")
    _same(out.pred[0], pred, "level >= card pred")
    high[3] = data[3]
    high[3, 0] = 9                                                               # ... but not the target's own
    assert run_blanket(be, high, net.card, masks, offsets, cpt, 0, 1).status == 0
    both = np.stack([net.masks, net.masks])
    off2 = np.concatenate([offsets, offsets[1:] + offsets[-1]])
    wrong = off2.copy()
    wrong[5:] += 1                                                               # structure 1, variable 1: a slot one too long
    out = run_blanket(be, data, net.card, both, wrong, np.concatenate([cpt, cpt, [0.5]]), 0, 1)
    assert out.rc == 0 and out.status == 16 and np.isnan(out.posterior[1]).all() and (out.pred[1] == 255).all()
    _same(out.posterior[0], blanket_ref(data, net.card, net.masks, net.tables, 0, 1)[0], "the structure before the bad slot")
    out = run_blanket(be, data, net.card, both, off2, np.concatenate([cpt, cpt]), 0, 1, cpt_bytes=(2 * cpt.size - 1) * 8)
    assert out.status == 16 and np.isnan(out.posterior[1]).all() and np.isfinite(out.posterior[0]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Brute-force enumeration of the joint (the checks of the restatements: tests/test_infer_ref.py)
# ---------------------------------------------------------------------------------------------------------------------
def enumerate_states(card):
    """u8 [prod card, n]: every joint state"""
    return np.array(list(itertools.product(*[range(int(c)) for c in card])), np.uint8)


def joint_factors(net, states):
    """f64 [states, n]: theta(v | pa) of every variable in every state"""
    out = np.empty(states.shape, np.float64)
    for v in range(len(net.card)):
        ps, _, _ = pm.family_shape(net.card, net.masks[v], v)
        out[:, v] = net.tables[v][pm.config_keys(states, net.card, ps), states[:, v]]
    return out


def exact_blanket(net, row, target):
    """[Fraction] over the target's levels: P(target = k | every other variable as in row), by enumeration of the joint in
    exact rationals of the fp64 tables; None when the row has probability zero"""
    joint = []
    for k in range(int(net.card[target])):
        x = np.array(row, np.uint8)[None, :].copy()
        x[0, target] = k
        f = joint_factors(net, x)[0]
        p = Fraction(1)
        for t in f:
            p *= Fraction(float(t))
        joint.append(p)
    total = sum(joint)
    return None if total == 0 else [p / total for p in joint]


def blanket_tolerance(net, target):
    factors = 1 + len(children_of(net.masks, target))
    return (factors + int(net.card[target])) * BLANKET_ULPS_PER_FACTOR


LwExact = namedtuple("LwExact", "p_evidence ess_ratio marginal marginal_se event event_se")


def lw_exact(net, evidence, observed, event=None, targets=0, M=STAT_PARTICLES):
    """Closed form of one likelihood-weighting query by enumeration: the exact posterior of every target cell and of the
    event, and the standard error of their M-particle estimates (module docstring).  ess_ratio = E_q[w]^2 / E_q[w^2]."""
    n = len(net.card)
    states = enumerate_states(net.card)
    keep = np.ones(len(states), bool)
    for v in range(n):
        if (observed >> v) & 1:
            keep &= states[:, v] == evidence[v]
    states = states[keep]
    f = joint_factors(net, states)
    obs = np.array([(observed >> v) & 1 for v in range(n)], bool)
    q = f[:, ~obs].prod(1)                                                       # the proposal
    w = f[:, obs].prod(1)                                                        # the weight
    ew, ew2 = float((q * w).sum()), float((q * w * w).sum())
    assert abs(q.sum() - 1.0) < 1e-9 and ew > 0

    def cell(ind):
        mu = float((q * w * ind).sum()) / ew
        var = float((q * w * w * (ind - mu) ** 2).sum()) / (M * ew * ew)
        return mu, math.sqrt(var)

    tg = targets_of(targets)
    marg, se = np.zeros((len(tg), 16)), np.zeros((len(tg), 16))
    for t, v in enumerate(tg):
        for k in range(int(net.card[v])):
            marg[t, k], se[t, k] = cell((states[:, v] == k).astype(np.float64))
    ev_mu = ev_se = None
    if event is not None:
        inside = np.ones(len(states), bool)
        for v in range(n):
            inside &= ((int(event[v]) >> states[:, v].astype(np.int64)) & 1).astype(bool)
        ev_mu, ev_se = cell(inside.astype(np.float64))
    return LwExact(ew, ew * ew / ew2, marg, se, ev_mu, ev_se)


@functools.lru_cache(maxsize=None)
def asia_network(iss=10.0):
    """asia's golden structure with bayes tables (iss = 10) as one Network"""
    data, card, masks, offsets, cpt = bayes_fit("asia", iss, 1)
    return pm.Network("asia", card, masks[0], [np.ascontiguousarray(t) for t in pm.tables_of(cpt, card, masks, offsets)[0]])


StatCase = namedtuple("StatCase", "network evidence event targets seed")
StatCase.__doc__ = "evidence {variable: level}, event {variable: levels} or None, targets mask: every cell of every target is checked"


@functools.lru_cache(maxsize=None)
def hand_four():
    """hand-written tables over levels (3, 2, 3, 2): 0 -> 1, (0, 1) -> 2, 2 -> 3"""
    card = np.asarray([3, 2, 3, 2], np.uint8)
    masks = sc.masks_of(4, {1: [0], 2: [0, 1], 3: [2]})[0]
    tables = [np.array([[0.3, 0.4, 0.3]]), np.array([[0.7, 0.3], [0.4, 0.6], [0.2, 0.8]]),
              np.array([[0.5, 0.3, 0.2], [0.2, 0.5, 0.3], [0.3, 0.3, 0.4], [0.25, 0.25, 0.5], [0.4, 0.4, 0.2], [0.2, 0.3, 0.5]]),
              np.array([[0.8, 0.2], [0.5, 0.5], [0.3, 0.7]])]
    return pm.Network("handfour", card, masks, tables)


def stat_network(name):
    return asia_network() if name == "asia" else hand_four() if name == "handfour" else pm.network(name)


def _stat_query(case):
    net = stat_network(case.network)
    n = len(net.card)
    evidence = np.zeros((1, n), np.uint8)
    observed = 0
    for v, k in case.evidence.items():
        evidence[0, v] = k
        observed |= 1 << v
    return net, evidence, observed, event_words(n, case.event) if case.event else None


def stat_preconditions(case, M=STAT_PARTICLES):
    """the exact posterior and standard errors of a case (LwExact), after asserting that the case is a fair one: an exact
    effective sample size >= 400 and every checked cell in [0.05, 0.95]"""
    net, evidence, observed, ev_words = _stat_query(case)
    exact = lw_exact(net, evidence[0], observed, ev_words, case.targets, M)
    assert M * exact.ess_ratio >= STAT_MIN_ESS, ("effective sample size", case, M * exact.ess_ratio)
    lo, hi = STAT_CELL_RANGE
    for t, v in enumerate(targets_of(case.targets)):
        for k in range(int(net.card[v])):
            assert lo <= exact.marginal[t, k] <= hi, ("cell out of range", case, v, k, exact.marginal[t, k])
    if case.event:
        assert lo <= exact.event <= hi, ("cell out of range", case, "event", exact.event)
    return exact


def stat_check(case, M=STAT_PARTICLES):
    """the restatement at M particles against the exact posterior: preconditions, then every cell within 5 standard errors.
    Returns the largest deviation in standard errors."""
    exact = stat_preconditions(case, M)
    net, evidence, observed, ev_words = _stat_query(case)
    ref = lw_ref(net, evidence, [observed], M, case.seed, 0, ev_words, case.targets)
    worst = 0.0
    for t, v in enumerate(targets_of(case.targets)):
        for k in range(int(net.card[v])):
            mu, se = exact.marginal[t, k], exact.marginal_se[t, k]
            dev = abs(ref.marginals[0, t, k] / ref.sums[0, 0] - mu) / se
            assert dev <= STAT_SIGMAS, (case, v, k, dev)
            worst = max(worst, dev)
    if case.event:
        dev = abs(ref.sums[0, 2] / ref.sums[0, 0] - exact.event) / exact.event_se
        assert dev <= STAT_SIGMAS, (case, "event", dev)
        worst = max(worst, dev)
    return worst


# Seeded evidence sets at M = 4096, chosen on the CPU so that the preconditions hold; every cell of every target is checked.
# asia's variables 1, 4 and 7 (smoke, bronc, dysp) are the ones whose posteriors stay inside [0.05, 0.95].
STAT_CASES = (
    StatCase("hand", {2: 1}, {0: [1]}, 0b011, 0),
    StatCase("hand", {2: 0}, None, 0b011, 1),
    StatCase("handfour", {3: 1}, {0: [0, 1]}, 0b0111, 0),
    StatCase("handfour", {2: 2}, {1: [1], 3: [0]}, 0b1011, 1),
    StatCase("handfour", {0: 1, 3: 0}, None, 0b0110, 2),
    StatCase("asia", {7: 1}, {1: [1], 4: [1]}, 0b00010010, 0),
    StatCase("asia", {4: 1}, {7: [1]}, 0b10000010, 1),
    StatCase("asia", {1: 1, 7: 1}, None, 0b00010000, 2),
    StatCase("asia", {6: 1}, {1: [1]}, 0b10010010, 0),
    StatCase("asia", {6: 0, 3: 0}, {4: [0], 7: [0]}, 0b10010010, 1),
)
# every variable but the target observed: likelihood weighting estimates what dvs_bn_blanket_posterior computes
STAT_BLANKET_CASES = (
    StatCase("asia", {0: 0, 2: 0, 3: 0, 4: 1, 5: 0, 6: 0, 7: 1}, None, 1 << 1, 0),
    StatCase("asia", {0: 0, 1: 1, 2: 0, 3: 0, 4: 1, 5: 0, 6: 0}, None, 1 << 7, 1),
    StatCase("handfour", {0: 1, 1: 0, 3: 1}, None, 1 << 2, 2),
)


def stat_check_blanket(case, M=STAT_PARTICLES):
    """stat_check, and the same bound against blanket_ref instead of the enumeration (which it must equal to rounding)"""
    worst = stat_check(case, M)
    net = stat_network(case.network)
    n = len(net.card)
    (target,) = targets_of(case.targets)
    assert set(case.evidence) == set(range(n)) - {target}
    row = np.zeros((1, n), np.uint8)
    observed = 0
    for v, k in case.evidence.items():
        row[0, v] = k
        observed |= 1 << v
    post, _ = blanket_ref(row, net.card, net.masks, net.tables, target, 1)
    exact = lw_exact(net, row[0], observed, None, case.targets, M)
    assert np.allclose(post[0], exact.marginal[0, :int(net.card[target])], rtol=1e-12, atol=0)
    ref = lw_ref(net, row, [observed], M, case.seed, 0, None, case.targets)
    dev = np.abs(ref.marginals[0, 0, :post.shape[1]] / ref.sums[0, 0] - post[0]) / exact.marginal_se[0, :post.shape[1]]
    assert (dev <= STAT_SIGMAS).all(), (case, dev)
    return max(worst, float(dev.max()))


# ---------------------------------------------------------------------------------------------------------------------
# 3b. predict and the prediction losses of cross_validate restated
# ---------------------------------------------------------------------------------------------------------------------
def predict_lw_ref(net, data, target, M, seed, query_offset=0):
    """lw_ref for predict(method = "bayes-lw") — one query per row, every variable but the target observed — vectorised over
    the rows -> (posterior f64 [S, r] = marginal / sum w, pred u8 [S]: the lowest of the maxima, 255 where sum w = 0)"""
    S, n = data.shape
    r = int(net.card[target])
    g = (np.arange(S, dtype=np.uint64) + U64(query_offset)) & U64(0xFFFFFFFF)
    key = orng.draw(orng.site_key(int(seed), SITE_BN_LW, g), np.uint64(target))                  # [S]
    h = orng.draw(key[:, None], np.arange(M, dtype=np.uint64)[None, :]) >> U64(1)                # [S, M]
    ps, _, _ = pm.family_shape(net.card, net.masks[target], target)
    T = _thresholds(net)[target][pm.config_keys(data, net.card, ps)]                            # [S, r]
    drawn = (h[:, :, None] >= T[:, None, :r - 1]).sum(2).astype(np.uint8)                        # [S, M]
    levels = np.repeat(data[:, None, :], M, axis=1).reshape(S * M, n)
    levels[:, target] = drawn.reshape(-1)
    w = np.ones(S * M)
    for v in pm.topological_order(net.masks):
        if v != target:
            ps, _, _ = pm.family_shape(net.card, net.masks[v], v)
            w *= net.tables[v][pm.config_keys(levels, net.card, ps), levels[:, v]]
    w = w.reshape(S, M)
    total = ordered_sum(w)
    marg = np.stack([ordered_sum(np.where(drawn == k, w, 0.0)) for k in range(r)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        post = marg / total[:, None]
    pred = np.argmax(post, axis=1).astype(np.uint8)
    pred[total == 0.0] = 255
    return post, pred


def cv_pred_reference(data, card, masks, folds, seed, iss, target, loss, M=500):
    """f64 [B]: the share of held-out rows predicted wrongly, with cross_validate's folds, bayes tables from exact rationals
    and blanket_ref / predict_lw_ref (query index = the row's position among the held-out rows of all folds so far)"""
    S = data.shape[0]
    perm = pm.cv_permutation(S, seed)
    B, n = masks.shape
    wrong = np.zeros(B)
    for f in range(folds):
        lo, hi = f * S // folds, (f + 1) * S // folds
        test, train = data[perm[lo:hi]], data[np.concatenate([perm[:lo], perm[hi:]])]
        for b in range(B):
            tables = [pm.fit_reference(pm.family_counts(train, card, masks[b, v], v), 1, iss, 0) for v in range(n)]
            if loss == "pred-lw":
                _, pred = predict_lw_ref(pm.Network("cv", card, masks[b], tables), test, target, M, seed, lo)
            else:
                _, pred = blanket_ref(test, card, masks[b], tables, target, 1 if loss == "pred-exact" else 0)
            wrong[b] += int((pred != test[:, target]).sum())
    return wrong / S


# ---------------------------------------------------------------------------------------------------------------------
# 4. Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []

    # (n_vars, n_queries, n_particles, card, parents, offsets, cpt, n_cells, evidence, observed, event, targets, seed,
    #  query_offset, workspace, workspace_bytes, sums, marginals, particles, particle_weights, status, stream)
    need = 256 + 512 + 256 + 1792                    # 100 cells, 3 queries; 3 * 2 chunks * (3 + 2 * 16) cells * 8 = 1680 -> 1792
    c = entry("dvs_bn_lw", cases, n_vars=12, n_queries=3, n_particles=300, card=D, parents=D, offsets=D, cpt=D, n_cells=100,
              evidence=D, observed=D, event=None, targets=0b101, seed=7, query_offset=0, workspace=D, workspace_bytes=need,
              sums=D, marginals=D, particles=None, particle_weights=None, status=D, stream=None)
    c(2, "n_queries and n_particles must be in [1, 2^31 - 1]", n_queries=0)
    c(2, "n_queries and n_particles must be in [1, 2^31 - 1]", n_particles=0)
    c(2, "n_queries and n_particles must be in [1, 2^31 - 1]", n_particles=1 << 31)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=11)
    c(2, "n_queries * ceil(n_particles / 256) must be < 2^31", n_queries=1 << 24, n_particles=1 << 16, workspace_bytes=1 << 60)
    c(12, "targets has a bit at or above n_vars", targets=1 << 12)
    c(12, "query_offset must be >= 0", query_offset=-1)
    for name in ("card", "parents", "offsets", "cpt", "evidence", "observed", "workspace", "sums", "status"):
        c(10, "null pointer", **{name: None})
    c(12, "marginals goes with targets != 0, and only with it", marginals=None)
    c(12, "marginals goes with targets != 0, and only with it", targets=0)
    c(12, "particles and particle_weights are both null or both given", particles=D)
    c(12, "particles and particle_weights are both null or both given", particle_weights=D)
    c(14, f"workspace_bytes < dvs_bn_lw_workspace_bytes = {need}", workspace_bytes=need - 1)
    c(2, "n_queries and n_particles must be in", n_queries=0, n_vars=49)               # the counts before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, n_cells=0)                            # n_vars before n_cells
    c(2, "n_cells must be in", n_cells=0, targets=1 << 12)                             # n_cells before targets
    c(12, "targets has a bit", targets=1 << 12, query_offset=-1)                       # targets before query_offset
    c(12, "query_offset must be >= 0", query_offset=-1, card=None)                     # query_offset before null
    c(10, "null pointer", status=None, marginals=None)                                 # null before marginals / targets
    c(12, "marginals goes with", marginals=None, particles=D)                          # marginals before particles
    c(12, "particles and particle_weights", particles=D, workspace_bytes=0)            # particles before workspace_bytes

    c = entry("dvs_bn_blanket_posterior", cases, batch=3, n_vars=6, n_rows=300, data=D, card=D, parents=D, offsets=D, cpt=D,
              cpt_bytes=144, target=2, use_children=1, posterior=None, pred=D, status=D, stream=None)
    c(2, "batch must be > 0", batch=0)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "batch * n_vars and batch * ceil(n_rows / 256) must be < 2^31", batch=1 << 30, n_vars=48, cpt_bytes=1 << 50)
    c(12, "target must be in [0, n_vars)", target=6)
    c(12, "target must be in [0, n_vars)", target=-1)
    c(12, "use_children must be 0 or 1", use_children=2)
    for name in ("data", "card", "parents", "offsets", "cpt", "pred", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "cpt_bytes < batch * n_vars * 8 = 144", cpt_bytes=143)
    c(2, "batch must be > 0", batch=0, n_rows=0)                                       # batch before n_rows
    c(2, "n_rows must be in", n_rows=0, n_vars=49)                                     # n_rows before n_vars
    c(3, "n_vars must be in [1, 48]", n_vars=49, target=-1)                            # n_vars before target
    c(12, "target must be in", target=6, use_children=2)                               # target before use_children
    c(12, "use_children must be", use_children=2, data=None)                           # use_children before null
    c(10, "null pointer", status=None, cpt_bytes=0)                                    # null before cpt_bytes
    return cases


def check_argument_refusals(lib, D=None):
    D = ctypes.c_void_p(4096) if D is None else D                                # never dereferenced
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {"dvs_bn_lw", "dvs_bn_blanket_posterior"}
    run(lib, cases)
    assert lib.dvs_bn_lw_workspace_bytes(100, 12, 3, 300, 0b101) == 2816
    for args, text in (((100, 0, 3, 300, 0), "n_vars must be in [1, 48]"), ((11, 12, 3, 300, 0), "n_cells must be in"),
                       ((100, 12, 0, 300, 0), "n_queries and n_particles"), ((100, 12, 3, 300, 1 << 12), "targets has a bit")):
        assert lib.dvs_bn_lw_workspace_bytes(*args) == 0
        msg = lib.dvs_last_error().decode()
        assert msg.startswith("dvs_bn_lw_workspace_bytes:") and text in msg, msg
