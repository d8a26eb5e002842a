"""TEST HELPER: networks, references and the checks themselves for exact inference by variable elimination
(csrc/dvs_eliminate.h: dvs_bn_eliminate; definitions in include/dvs_eliminate.h; the planner: dags_vae_search_amd/eliminate.py).
Plain numpy, no GPU: tests/test_emu_eliminate.py (emulator build) and tests/test_gpu_eliminate.py (device) run the same checks
through the raw C ABI by argument name and differ only in the backend that moves buffers (tests/scoring_corpus.py);
tests/test_eliminate_ref.py checks the planner and the restatement themselves.

References
  execute_plan   the plan words executed in numpy in the kernel's order (per cell: the levels of x ascending, the inputs in plan
                 order, one fp64 multiplication each, acc + p from +0; z by the fixed tree): the kernels must give the same bytes.
  exact_cells    brute-force enumeration of the joint in exact rationals of the fp64 tables (infer_corpus.enumerate_states /
                 joint_factors); chain_exact: forward-backward in rationals on chain48, where enumeration is impossible.

The tolerance is derived, not chosen.  Every term is non-negative, so the relative error of a cell is at most
gamma_D = D u / (1 - D u), u = 2^-53, with D the plan's depth by recurrence: a table cell has 0, a step output the largest depth
of its inputs + (inputs - 1) + (levels summed - 1); z adds ceil(cells / 256) - 1 + 8; a quotient adds 1.  (EliminationPlan.depth
and .z_depth carry the recurrence.)  The checks use that bound with no extra factor.

dvs_bn_eliminate is declared in the companion header, which tests/abi_cases.py (dl.SIGNATURES only) does not read: call /
call_rc / entry below are the same functions over dl.signature.
"""
import ctypes
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd import eliminate as el
from tests import infer_corpus as ic
from tests import params_corpus as pm
from tests import scoring_corpus as sc
from tests.abi_cases import run

FN = "dvs_bn_eliminate"
SENTINEL = pm.SENTINEL
GUARD = 64                                    # sentinel cells on either side of every output
ROW_COUNTS = (1, 5, 64, 257)
ROWS_PER_GROUP = (0, 1, 3, 64)
NETWORKS = ("hand", "handfour", "six", "zeroone", "chain48", "asia", "band48")
ENUMERABLE = ("hand", "handfour", "six", "zeroone", "asia")


# ---------------------------------------------------------------------------------------------------------------------
# The C ABI by argument name, over both headers
# ---------------------------------------------------------------------------------------------------------------------
def _signature(fn, given, optional=()):
    sig = dl.signature(fn)[1]
    missing, unknown = {n for n, _ in sig} - set(given) - set(optional), set(given) - {n for n, _ in sig}
    if missing or unknown:
        raise TypeError(f"{fn}: arguments go by the names of its header: missing {sorted(missing)}, unknown {sorted(unknown)}")
    return sig


def call_rc(be, fn, **args):
    ptr = lambda v: v if v is None or isinstance(v, ctypes.c_void_p) else be.ptr(v)
    return getattr(be.lib, fn)(*[ptr(args.get(n, be.stream)) if ctype is ctypes.c_void_p else args[n]
                                 for n, ctype in _signature(fn, args, optional=("stream",))])


def call(be, fn, **args):
    assert call_rc(be, fn, **args) == 0, be.lib.dvs_last_error()


def entry(fn, into, **base):
    names = [name for name, _ in _signature(fn, base)]

    def case(code, text, **overrides):
        _signature(fn, overrides, optional=names)
        args = {**base, **overrides}
        into.append((fn, [args[name] for name in names], code, f"{fn}: {text}"))
    return case


# ---------------------------------------------------------------------------------------------------------------------
# Networks
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network(name):
    if name == "band48":                      # 48 variables, 2..4 levels, 1..3 parents within the 6 preceding indices
        rng = np.random.default_rng(4801)
        card = rng.integers(2, 5, 48).astype(np.uint8)
        dag = {}
        for v in range(1, 48):
            window = list(range(max(0, v - 6), v))
            dag[v] = sorted(int(u) for u in rng.choice(window, size=min(len(window), int(rng.integers(1, 4))), replace=False))
        masks = sc.masks_of(48, dag)[0]
        return pm.Network(name, card, masks, pm.random_tables(card, masks, 4802))
    if name == "isolated":                    # variables 1 and 3 touch nothing: their tables sum out to scalar factors
        card = np.asarray([2, 3, 4, 2], np.uint8)
        masks = sc.masks_of(4, {2: [0]})[0]
        return pm.Network(name, card, masks, pm.random_tables(card, masks, 4803))
    if name == "dense":                       # a seeded dense DAG whose elimination exceeds the cap
        rng = np.random.default_rng(4804)
        card = np.full(30, 4, np.uint8)
        dag = {v: sorted(int(u) for u in rng.choice(v, size=min(v, 3), replace=False)) for v in range(1, 30)}
        return pm.Network(name, card, sc.masks_of(30, dag)[0], None)
    if name in ("six", "handfour", "asia"):
        return ic.lw_network("six") if name == "six" else ic.stat_network(name)
    return pm.network(name)


def plan_of(name, keep=(), order=None):
    net = network(name)
    return el.plan_network(net.card, net.masks, keep, order)


def query_masks(name, Q, seed=11):
    """u16 [Q, n] level masks: rows drawn from the network itself, each variable observed with probability 1 / 2, and in every
    second row one more variable restricted to a seeded level set (an event; bits at or above card are set too and must be
    ignored).  Row 0 observes nothing, row 1 everything, row 2 has an empty allowed set (mask 0) and row 3 one that is empty once
    the bits at or above card are ignored."""
    net = network(name)
    n = len(net.card)
    rows = pm.sample_ref(net, Q, seed=seed)
    rng = np.random.default_rng(seed)
    seen = rng.random((Q, n)) < 0.5
    seen[0] = False
    if Q > 1:
        seen[1] = True
    masks = np.where(seen, np.uint16(1) << rows.astype(np.uint16), np.uint16(0xFFFF)).astype(np.uint16)
    for q in range(4, Q, 2):
        v = int(rng.integers(0, n))
        masks[q, v] = np.uint16(int(rng.integers(1, 1 << int(net.card[v]))) | (0xFFFF & ~((1 << int(net.card[v])) - 1)))
    if Q > 2:
        masks[2, n // 2] = 0
    if Q > 3:
        v = n - 1
        masks[3, v] = np.uint16(0xFFFF & ~((1 << int(net.card[v])) - 1))
    return masks


# ---------------------------------------------------------------------------------------------------------------------
# The restatement: plan words executed in the kernel's order
# ---------------------------------------------------------------------------------------------------------------------
def z_sum(cells):
    """f64 [..., C] -> [...]: slot t of 256 adds cells t, t + 256, ... ascending from +0, then x[i] += x[i + s], s = 128 .. 1"""
    cells = np.asarray(cells, np.float64)
    slots = np.zeros(cells.shape[:-1] + (256,))
    for c0 in range(0, cells.shape[-1], 256):
        part = cells[..., c0:c0 + 256]
        slots[..., :part.shape[-1]] = slots[..., :part.shape[-1]] + part
    return ic._tree(slots)


def execute_plan(words, card, tables, masks):
    """-> (out f64 [R, out_cells], z f64 [R]) as k_bn_eliminate computes them"""
    w = [int(x) for x in words]
    assert w[0] == dl.ELIM_TAG and w[1] == len(card)
    steps, arena_cells = w[2], w[3]
    cur = 6 + w[5]
    R = masks.shape[0]
    masks = masks.astype(np.int64)
    arena = np.zeros((R, arena_cells))
    flat = [np.asarray(t, np.float64).reshape(-1) for t in tables]
    out = None
    for _ in range(steps):
        x, off, cells, ns, ni = w[cur:cur + 5]
        scope = w[cur + 5:cur + 5 + ns]
        lv, rem = [], np.arange(cells)
        for v in scope:
            lv.append(rem % int(card[v]))
            rem = rem // int(card[v])
        allowed = np.ones((R, cells), bool)
        if x < 0:
            for i, v in enumerate(scope):
                allowed &= ((masks[:, v][:, None] >> lv[i][None, :]) & 1).astype(bool)
        acc = np.zeros((R, cells))
        for k in range(int(card[x]) if x >= 0 else 1):
            ok = allowed & (((masks[:, x] >> k) & 1).astype(bool)[:, None] if x >= 0 else True)
            p = None
            for j in range(ni):
                inw = w[cur + 5 + ns + j * (4 + ns):cur + 5 + ns + (j + 1) * (4 + ns)]
                at = k * inw[3] + sum(lv[i] * inw[4 + i] for i in range(ns)) + np.zeros(cells, np.int64)
                val = np.broadcast_to(flat[inw[0]][at], (R, cells)) if inw[0] >= 0 else arena[:, inw[1] + at]
                p = val if p is None else p * val
            acc = np.where(ok, acc + p, acc)
        if x >= 0:
            arena[:, off:off + cells] = acc
        else:
            out = acc
        cur += 5 + ns + ni * (4 + ns)
    assert cur == len(w) and out is not None
    return out, z_sum(out)


# ---------------------------------------------------------------------------------------------------------------------
# Exact rationals
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _joint(name):
    net = network(name)
    states = ic.enumerate_states(net.card)
    joint = []
    for f in ic.joint_factors(net, states):
        p = Fraction(1)
        for t in f:
            p *= Fraction(float(t))
        joint.append(p)
    return states, joint


def exact_cells(name, mask_row, keep):
    """[Fraction] over the cells of ``keep`` (lowest id fastest): P(kept levels and the row's masks), by enumeration"""
    net = network(name)
    states, joint = _joint(name)
    n = len(net.card)
    live = np.ones(len(states), bool)
    for v in range(n):
        live &= ((int(mask_row[v]) >> states[:, v].astype(np.int64)) & 1).astype(bool)
    idx, stride = np.zeros(len(states), np.int64), 1
    for v in sorted(keep):
        idx += states[:, v].astype(np.int64) * stride
        stride *= int(net.card[v])
    cells = [Fraction(0)] * stride
    for s in np.flatnonzero(live):
        cells[idx[s]] += joint[s]
    return cells


def chain_exact(mask_row, keep):
    """the same for chain48 (v's parent is v + 1) and ``keep`` empty or one variable: forward-backward in rationals"""
    net = network("chain48")
    n = 48
    ok = lambda v, l: (int(mask_row[v]) >> l) & 1
    theta = lambda v, pl, l: Fraction(float(net.tables[v][pl, l]))
    alpha = [None] * n                                            # alpha[v][l] = P(x_v = l, the masks of v .. 47)
    alpha[47] = [theta(47, 0, l) * ok(47, l) for l in range(int(net.card[47]))]
    for v in range(46, -1, -1):
        alpha[v] = [sum(alpha[v + 1][pl] * theta(v, pl, l) for pl in range(int(net.card[v + 1]))) * ok(v, l)
                    for l in range(int(net.card[v]))]
    if not keep:
        return [sum(alpha[0])]
    (t,) = keep
    beta = [Fraction(1)] * int(net.card[0])                       # beta[l] = P(the masks of 0 .. v - 1 | x_v = l)
    for v in range(1, t + 1):
        beta = [sum(theta(v - 1, l, c) * ok(v - 1, c) * beta[c] for c in range(int(net.card[v - 1]))) for l in range(int(net.card[v]))]
    return [a * b for a, b in zip(alpha[t], beta)]


def gamma(depth):
    """gamma_D = D u / (1 - D u) as an exact rational, u = 2^-53"""
    return Fraction(depth, 2 ** 53 - depth)


def assert_within(got, exact, depth, what):
    """every fp64 cell within gamma_depth (relative) of its exact rational; an exact zero must be zero"""
    g = gamma(depth)
    for i, (a, e) in enumerate(zip(np.asarray(got, np.float64).reshape(-1).tolist(), exact)):
        assert abs(Fraction(a) - e) <= g * e, (what, i, a, float(e), depth)


def check_against_exact(name, plan, masks, exact):
    """the restatement of ``plan`` against ``exact(mask_row, keep)``: cells, z and the quotients, each within its derived bound"""
    net = network(name)
    out, z = execute_plan(plan.words, net.card, net.tables, masks)
    with np.errstate(invalid="ignore", divide="ignore"):
        post = out / z[:, None]
    for q in range(masks.shape[0]):
        cells = exact(masks[q], plan.keep)
        total = sum(cells)
        assert_within(out[q], cells, plan.depth, (name, plan.keep, q, "cells"))
        assert_within(z[q:q + 1], [total], plan.z_depth, (name, plan.keep, q, "z"))
        if total == 0:
            assert z[q] == 0.0 and np.isnan(post[q]).all(), (name, plan.keep, q)
        else:
            assert_within(post[q], [c / total for c in cells], plan.z_depth + 1, (name, plan.keep, q, "posterior"))
    return out, z


# ---------------------------------------------------------------------------------------------------------------------
# The raw call
# ---------------------------------------------------------------------------------------------------------------------
ElimOut = namedtuple("ElimOut", "rc out z flags status guards_ok")


def _guarded(be, shape, dtype, fill):
    a = np.full(int(np.prod(shape)) + 2 * GUARD, fill, dtype)
    return be.put(a), a.itemsize * GUARD


def run_eliminate(be, net, words_list, masks, rows_per_group=0, out_stride=None, arena_cells=None, step_cells=None,
                  plan_words=None, offsets=None, cpt=None):
    """one dvs_bn_eliminate over the plans ``words_list`` (int32 arrays); out, z and plan_flags sit between GUARD sentinel
    cells, which must stay untouched (guards_ok)"""
    n, P, R = len(net.card), len(words_list), masks.shape[0]
    if offsets is None:
        offsets, cpt = pm.flat_network(net)
    header = lambda k: max(int(w[k]) for w in words_list if len(w) > k)
    stride = header(4) if out_stride is None else out_stride
    words = np.concatenate([np.asarray(w, np.int32) for w in words_list])
    starts = np.concatenate([[0], np.cumsum([len(w) for w in words_list])]).astype(np.int64)
    at = lambda h, skip: ctypes.c_void_p(be.ptr(h).value + skip)
    out, out_skip = _guarded(be, (P, R, stride), np.float64, SENTINEL)
    z, z_skip = _guarded(be, (P, R), np.float64, SENTINEL)
    flags, f_skip = _guarded(be, (P,), np.int32, 77)
    h = dict(card=be.put(net.card), parents=be.put(net.masks), offsets=be.put(offsets), cpt=be.put(cpt), plans=be.put(words),
             plan_offsets=be.put(starts), masks=be.put(np.ascontiguousarray(masks, np.uint16).view(np.int16)), status=be.put(np.zeros(1, np.int32)))
    rc = call_rc(be, FN, n_vars=n, n_plans=P, n_rows=R, n_cells=int(offsets[-1] - offsets[0]), plans_bytes=words.nbytes,
                 plan_words=max(len(w) for w in words_list) if plan_words is None else plan_words,
                 arena_cells=header(3) if arena_cells is None else arena_cells,
                 step_cells=max(_step_cells(w) for w in words_list) if step_cells is None else step_cells,
                 rows_per_group=rows_per_group, out_stride=stride, out=at(out, out_skip), out_bytes=P * R * stride * 8,
                 z=at(z, z_skip), plan_flags=at(flags, f_skip), **h)
    o, zz, ff = be.get(out).copy(), be.get(z).copy(), be.get(flags).copy()
    guards = all((a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all() for a, fill in ((o, SENTINEL), (zz, SENTINEL), (ff, 77)))
    return ElimOut(rc, o[GUARD:-GUARD].reshape(P, R, stride), zz[GUARD:-GUARD].reshape(P, R), ff[GUARD:-GUARD],
                   int(be.get(h["status"])[0]), guards)


def _step_cells(words):
    """the largest step output of well-formed plan words (a malformed plan states nothing the launch relies on)"""
    w = [int(x) for x in words]
    best, cur = 1, 6 + w[5]
    for _ in range(w[2]):
        if cur + 5 > len(w):
            break
        best = max(best, min(max(w[cur + 2], 1), dl.ELIM_MAX_CELLS))
        cur += 5 + w[cur + 3] + w[cur + 4] * (4 + w[cur + 3])
    return best


def _same(got, ref, what):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.tobytes() == ref.tobytes(), (what, np.argwhere(~((got == ref) | ((got != got) & (ref != ref))))[:4])


def reference(net, plans, masks, stride):
    """(out [P, R, stride], z [P, R]) of the restatement, padded with +0 as the kernel pads"""
    P, R = len(plans), masks.shape[0]
    out, z = np.zeros((P, R, stride)), np.zeros((P, R))
    for i, plan in enumerate(plans):
        o, z[i] = execute_plan(plan.words, net.card, net.tables, masks)
        out[i, :, :o.shape[1]] = o
    return out, z


KEEPS = {"hand": ((), (0,), (1, 2)), "handfour": ((), (2,), (0, 3)), "six": ((), (4,), (0, 2, 5)), "zeroone": ((), (4,), (1, 3)),
         "chain48": ((), (0,), (17,), (47,)), "asia": ((), (1,), (4, 7)), "band48": ((), (0,), (23,), (40, 47))}


@functools.lru_cache(maxsize=None)
def bytes_case(name, n_rows):
    """(plans, masks, reference out, reference z) of check_bytes: computed once, shared by the emulator and the device tests"""
    net = network(name)
    plans = [plan_of(name, keep) for keep in KEEPS[name]]
    masks = query_masks(name, n_rows)
    stride = max(p.out_cells for p in plans)
    return plans, masks, reference(net, plans, masks, stride)


def check_bytes(be, name, n_rows):
    """several plans in one call: out and z equal the restatement byte for byte; two calls give equal bytes"""
    net = network(name)
    plans, masks, (ref_out, ref_z) = bytes_case(name, n_rows)
    got = run_eliminate(be, net, [p.words for p in plans], masks)
    assert (got.rc, got.status, got.guards_ok) == (0, 0, True) and not got.flags.any(), (name, n_rows, got.rc, got.status)
    _same(got.out, ref_out, (name, n_rows, "out"))
    _same(got.z, ref_z, (name, n_rows, "z"))
    if n_rows > 2:
        assert (got.z[:, 2] == 0.0).all() and not np.signbit(got.out[:, 2]).any()      # an empty allowed set: plain zeros
    if n_rows == 5:
        again = run_eliminate(be, net, [p.words for p in plans], masks)
        _same(again.out, got.out, "two calls")
        _same(again.z, got.z, "two calls")


def check_rows_per_group(be, name):
    """the bytes do not depend on the rows per workgroup, row counts that are no multiple of it included"""
    net = network(name)
    for n_rows in (5, 257) if name != "chain48" else (5,):
        plans, masks, (ref_out, ref_z) = bytes_case(name, n_rows)
        for G in ROWS_PER_GROUP:
            got = run_eliminate(be, net, [p.words for p in plans], masks, rows_per_group=G)
            assert (got.rc, got.status, got.guards_ok) == (0, 0, True), (name, n_rows, G)
            _same(got.out, ref_out, (name, n_rows, G, "out"))
            _same(got.z, ref_z, (name, n_rows, G, "z"))


def loop_shape_plans():
    """[(network, plan)]: a step output above 256 cells (512 and 768), a final factor of 768 cells, a one-level variable kept,
    keep empty, scalar factors from isolated variables"""
    cases = [("six", plan_of("six", (1,), order=[4, 0, 2, 3, 5])), ("six", plan_of("six", (0, 2, 5))), ("six", plan_of("six", (4,))),
             ("six", plan_of("six", ())), ("isolated", plan_of("isolated", ())), ("isolated", plan_of("isolated", (0, 3)))]
    assert cases[0][1].max_step_cells == 512 and cases[1][1].out_cells == 768 and cases[1][1].max_step_cells == 768
    assert any(s["cells"] == 1 and s["x"] >= 0 for s in cases[4][1].steps)          # a scalar factor
    return cases


def check_loop_shapes(be):
    for n_rows in (5, 64):
        for name in ("six", "isolated"):
            net = network(name)
            plans = [p for nm, p in loop_shape_plans() if nm == name]
            masks = query_masks(name, n_rows, seed=13)
            stride = max(p.out_cells for p in plans)
            ref_out, ref_z = reference(net, plans, masks, stride)
            got = run_eliminate(be, net, [p.words for p in plans], masks)
            assert (got.rc, got.status, got.guards_ok) == (0, 0, True), (name, got.rc, got.status)
            _same(got.out, ref_out, (name, n_rows, "out"))
            _same(got.z, ref_z, (name, n_rows, "z"))


def malformed_plans():
    """{what: words}: asia's plan for keep (4, 7) with one thing wrong each"""
    good = plan_of("asia", (4, 7)).words
    w = [int(x) for x in good]
    first = 6 + w[5]                                             # the first step
    ns, ni = w[first + 3], w[first + 4]
    bad = {}
    b = good.copy()
    b[first + 1] = w[3] - w[first + 2] + 1                       # the first step's output ends one cell beyond arena_cells
    bad["an arena span beyond arena_cells"] = b
    b = good.copy()
    b[first + 5 + ns + 3] += 1 << 20                             # stride_x of the first input (a table) leaves the table
    bad["a stride that leaves its table"] = b
    arena_in = next((cur, j) for cur, s_ns, s_ni in _steps(w) for j in range(s_ni)
                    if w[cur + 5 + s_ns + j * (4 + s_ns)] == -1 and w[cur] >= 0)
    cur, j = arena_in
    b = good.copy()
    b[cur + 1] = w[cur + 5 + w[cur + 3] + j * (4 + w[cur + 3]) + 1]      # the output starts where one of its inputs lies
    bad["an output that overlaps an input"] = b
    assert ni >= 1
    return good, bad


def _steps(w):
    cur = 6 + w[5]
    for _ in range(w[2]):
        yield cur, w[cur + 3], w[cur + 4]
        cur += 5 + w[cur + 3] + w[cur + 4] * (4 + w[cur + 3])


def check_malformed(be):
    """a malformed plan sets bit 4 and is NaN; the other plans of the call are bytewise what they are without it; nothing is
    written outside the buffers"""
    net = network("asia")
    good, bad = malformed_plans()
    other = plan_of("asia", (1,)).words
    masks = query_masks("asia", 5)
    alone = run_eliminate(be, net, [good, other], masks, out_stride=4)
    assert (alone.rc, alone.status, alone.guards_ok) == (0, 0, True)
    cases = [(what, words, 4) for what, words in bad.items()] + [("out_cells > out_stride", good, 3)]
    for what, words, stride in cases:
        ref = alone if stride == 4 else run_eliminate(be, net, [other, other], masks, out_stride=stride)
        first = good if stride == 4 else other
        got = run_eliminate(be, net, [first, words, other], masks, out_stride=stride, arena_cells=max(int(good[3]), int(other[3])), step_cells=8)
        assert (got.rc, got.status, got.guards_ok) == (0, 16, True), (what, got.rc, got.status)
        assert got.flags.tolist() == [0, 1, 0], (what, got.flags)
        assert np.isnan(got.out[1]).all() and np.isnan(got.z[1]).all(), what
        _same(got.out[0], ref.out[0], (what, "the plan before"))
        _same(got.out[2], ref.out[1], (what, "the plan after"))
        _same(got.z[[0, 2]], ref.z, (what, "z of the others"))
    # a plan longer than the call says, a wrong tag, a truncated plan, offsets that leave the buffer
    for what, words, kw in (("plan_words too small", good, dict(plan_words=len(good) - 1)),
                            ("tag", np.concatenate([[7], good[1:]]).astype(np.int32), {}),
                            ("truncated", good[:-1], {}), ("arena_cells too small", good, dict(arena_cells=int(good[3]) - 1))):
        got = run_eliminate(be, net, [words], masks, out_stride=4, **kw)
        assert (got.rc, got.status, got.guards_ok) == (0, 16, True) and got.flags.tolist() == [1], (what, got.status)
        assert np.isnan(got.out).all() and np.isnan(got.z).all(), what
    # a table that does not match the structure refuses every plan
    offsets, cpt = pm.flat_network(net)
    wrong = offsets.copy()
    wrong[3:] += 2
    got = run_eliminate(be, net, [good, other], masks, out_stride=4, offsets=wrong, cpt=np.concatenate([cpt, [0.5, 0.5]]))
    assert (got.rc, got.status, got.guards_ok) == (0, 16, True) and got.flags.tolist() == [1, 1] and np.isnan(got.out).all()


def check_blanket_crosscheck(be, name, targets, n_rows=3):
    """every variable but the target observed: out / z of the target's plan equals dvs_bn_blanket_posterior within the sum of
    the two derived tolerances"""
    net = network(name)
    n = len(net.card)
    rows = pm.sample_ref(net, n_rows, seed=29)
    offsets, cpt = pm.flat_network(net)
    worst = 0.0
    for t in targets:
        plan = plan_of(name, (t,))
        masks = (np.uint16(1) << rows.astype(np.uint16)).astype(np.uint16)
        masks[:, t] = 0xFFFF
        got = run_eliminate(be, net, [plan.words], masks)
        ref = ic.run_blanket(be, rows, net.card, net.masks[None, :], offsets, cpt, t, 1)
        assert (got.rc, got.status, ref.rc, ref.status) == (0, 0, 0, 0)
        post = got.out[0] / got.z[0][:, None]
        tol = float(gamma(plan.z_depth + 1)) + ic.blanket_tolerance(net, t)
        rel = np.abs(post - ref.posterior[0]) / ref.posterior[0]
        assert (rel <= tol).all(), (name, t, rel.max(), tol)
        worst = max(worst, float(rel.max() / tol))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# Argument refusals (no device needed: everything is checked before anything is enqueued)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []
    c = entry(FN, cases, n_vars=8, n_plans=3, n_rows=100, card=D, parents=D, offsets=D, cpt=D, n_cells=36, plans=D,
              plans_bytes=84, plan_offsets=D, plan_words=200, arena_cells=17, step_cells=8, masks=D, rows_per_group=0,
              out_stride=16, out=D, out_bytes=38400, z=D, plan_flags=D, status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=7)
    c(2, "n_plans and n_rows must be in [1, 2^31 - 1] and n_plans * n_rows < 2^31", n_plans=0)
    c(2, "n_plans and n_rows must be in [1, 2^31 - 1] and n_plans * n_rows < 2^31", n_rows=0)
    c(2, "n_plans and n_rows must be in [1, 2^31 - 1] and n_plans * n_rows < 2^31", n_rows=1 << 31)
    c(2, "n_plans and n_rows must be in [1, 2^31 - 1] and n_plans * n_rows < 2^31", n_plans=1 << 16, n_rows=1 << 15,
      plans_bytes=1 << 40, out_bytes=1 << 60)
    c(12, "plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", plan_words=6)
    c(12, "plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", plan_words=4097)
    c(12, "arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", arena_cells=0)
    c(12, "arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", arena_cells=16385)
    c(12, "arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", step_cells=0)
    c(12, "out_stride must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", out_stride=0)
    c(12, "out_stride must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", out_stride=16385, out_bytes=1 << 40)
    c(12, "rows_per_group must be in [0, 64]", rows_per_group=-1)
    c(12, "rows_per_group must be in [0, 64]", rows_per_group=65)
    for name in ("card", "parents", "offsets", "cpt", "plans", "plan_offsets", "masks", "out", "z", "plan_flags", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "plans_bytes < n_plans * 28 = 84", plans_bytes=83)
    c(14, "out_bytes < n_plans * n_rows * out_stride * 8 = 38400", out_bytes=38399)
    c(3, "n_vars must be in [1, 48]", n_vars=49, n_cells=0)                            # n_vars before n_cells
    c(2, "n_cells must be in", n_cells=0, n_plans=0)                                   # n_cells before the counts
    c(2, "n_plans and n_rows", n_rows=0, plan_words=0)                                 # the counts before plan_words
    c(12, "plan_words must be in", plan_words=0, arena_cells=0)                        # plan_words before arena_cells
    c(12, "arena_cells and step_cells", step_cells=0, out_stride=0)                    # the cells before out_stride
    c(12, "out_stride must be in", out_stride=0, rows_per_group=65)                    # out_stride before rows_per_group
    c(12, "rows_per_group must be in", rows_per_group=65, card=None)                   # rows_per_group before null
    c(10, "null pointer", status=None, plans_bytes=0)                                  # null before plans_bytes
    c(14, "plans_bytes <", plans_bytes=0, out_bytes=0)                                 # plans_bytes before out_bytes
    return cases


def check_argument_refusals(lib, D=None):
    D = ctypes.c_void_p(4096) if D is None else D                                # never dereferenced
    cases = validation_cases(D)
    assert {fn for fn, *_ in cases} == {FN}
    run(lib, cases)
    for change in ({"n_rowz": 1}, {"n_rows": None}):
        args = {k: v for k, v in {**dict(zip([n for n, _ in dl.signature(FN)[1]], cases[0][1])), **change}.items() if v is not None}
        try:
            entry(FN, [], **args)
        except TypeError as e:
            assert FN in str(e)
        else:
            raise AssertionError("a missing or unknown name must be a TypeError")
