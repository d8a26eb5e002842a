"""TEST HELPER: cases, references and the checks themselves for learning from incomplete data (csrc/dvs_incomplete.h:
dvs_bn_expected_counts, dvs_bn_fit_counts, dvs_bn_impute; definitions in include/dvs_incomplete.h).  Plain numpy, no GPU:
tests/test_emu_incomplete.py (emulator build) and tests/test_gpu_incomplete.py (device) run the same checks through the raw C
ABI by argument name and differ only in the backend; tests/test_incomplete_ref.py checks the restatement itself.

References
  restate_counts / restate_impute / fit_counts_ref   the header's definitions in numpy on eliminate_corpus.execute_plan, in the
                 kernels' order: the kernels must give the same bytes (the log-likelihood: within the bound of dvs_bn_loglik,
                 since log() is the platform's).
  exact_counts / exact_argmax                         brute-force enumeration of the joint in exact rationals.

Tolerances are derived.  A quotient out / z of a family plan is within gamma_(z_depth + 1); adding a chunk's A active rows in
turn adds A - 1 roundings, the tree over the chunks ceil(chunks / 256) - 1 + 8, and I + F one more:
D = z_depth + 1 + (A - 1) + ceil(chunks / 256) - 1 + 8 + 1, with no extra factor.
"""
import ctypes
import functools
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests import infer_corpus as ic
from tests import params_corpus as pm
from tests import scoring_corpus as sc
from dags_vae_search_amd import eliminate as el
from tests import eliminate_corpus as ec
from tests.eliminate_corpus import _same, _step_cells, _steps, call_rc, entry, exact_cells, execute_plan, gamma, z_sum
from tests.abi_cases import run

SENTINEL = pm.SENTINEL
GUARD = 64
ROW_COUNTS = (1, 255, 257, 600)
ROWS_PER_GROUP = (0, 1, 3, 64)
BYTES_NETWORKS = ("hand", "six", "zeroone", "asia")
MISSING = 0.3
MANY_CHUNKS_ROWS = 256 * 256 + 1        # 257 chunks: slot 0 of the chunk tree and of the log-likelihood adds two of them
U64 = np.uint64


# ---------------------------------------------------------------------------------------------------------------------
# Plans and data
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network(name):
    """eliminate_corpus.network, and two of this corpus: "wide3", whose last family has 16 * 16 * 5 = 1280 cells (more than the
    1024 a workgroup of k_bn_inc_counts accumulates in registers), and "full4", whose last family fills the cap of 16 384 cells
    so that arena + last step exceed it (structure only)"""
    if name == "wide3":
        card = np.asarray([16, 16, 5], np.uint8)
        masks = sc.masks_of(3, {2: [0, 1]})[0]
        return pm.Network(name, card, masks, pm.random_tables(card, masks, 4805))
    if name == "full4":
        card = np.asarray([16, 16, 16, 4], np.uint8)
        return pm.Network(name, card, sc.masks_of(4, {3: [0, 1, 2]})[0], None)
    return ec.network(name)


def plan_of(name, keep=(), order=None):
    net = network(name)
    return el.plan_network(net.card, net.masks, keep, order)


def family(net, v):
    return tuple(sorted(set(pm.parents_of(net.masks[v], v)) | {v}))


@functools.lru_cache(maxsize=None)
def family_plans(name):
    """the n + 1 plans of dvs_bn_expected_counts: plan v keeps the family of v, the last nothing"""
    net = network(name)
    return [plan_of(name, family(net, v)) for v in range(len(net.card))] + [plan_of(name, ())]


@functools.lru_cache(maxsize=None)
def target_plans(name):
    """the n plans of dvs_bn_impute: plan v keeps {v}"""
    return [plan_of(name, (v,)) for v in range(len(network(name).card))]


def observed_bits(seen):
    """bool [R, n] -> u64 [R]"""
    return (seen.astype(U64) << np.arange(seen.shape[1], dtype=U64)).sum(1, dtype=U64)


def seen_of(observed, n):
    return ((observed[:, None] >> np.arange(n, dtype=U64)) & U64(1)).astype(bool)


@functools.lru_cache(maxsize=None)
def incomplete_case(name, n_rows, rate=MISSING, seed=41, special=True):
    """(levels u8 [R, n], observed u64 [R]): rows drawn from the network, each value missing with probability ``rate``; the
    nibble of a missing value is 15 (it must be ignored).  With ``special``: row 0 is wholly observed, row 1 wholly unobserved,
    row 2 (zeroone) observes a level of probability zero under its observed parent, row 3 an observed level at or above its
    variable's level count."""
    net = network(name)
    n = len(net.card)
    levels = pm.sample_ref(net, n_rows, seed=seed)
    seen = np.random.default_rng(seed + 1).random((n_rows, n)) >= rate
    if special:
        seen[0] = True
        if n_rows > 1:
            seen[1] = False
        if n_rows > 2 and name == "zeroone":
            j = next(j for j in range(net.tables[3].shape[0]) if (net.tables[3][j] == 0.0).any())
            seen[2] = False
            seen[2, 2] = seen[2, 3] = True
            levels[2, 2], levels[2, 3] = j, int(np.argmin(net.tables[3][j]))
        if n_rows > 3:
            v = next(v for v in range(n) if net.card[v] < 16)
            seen[3, v] = True
            levels[3, v] = net.card[v]
    levels = np.where(seen, levels, 15).astype(np.uint8)
    return levels, observed_bits(seen)


def row_masks(levels, observed):
    """u16 [R, n]: the level masks the kernels build on the fly"""
    seen = seen_of(observed, levels.shape[1])
    return np.where(seen, np.uint16(1) << levels.astype(np.uint16), np.uint16(0xFFFF)).astype(np.uint16)


def sound_rows(net, levels, observed):
    n = len(net.card)
    seen = seen_of(observed, n)
    return ((observed >> U64(n)) == 0) & ~(seen & (levels >= net.card[None, :])).any(1)


def _positive(z):
    return np.isfinite(z) & (z > 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# The restatement
# ---------------------------------------------------------------------------------------------------------------------
def plan_cell_of(net, v):
    """int [q * r]: the cell of the family plan (lowest id fastest) that holds the table cell j = key * r + k"""
    fam = family(net, v)
    ps, q, r = pm.family_shape(net.card, net.masks[v], v)
    j = np.arange(q * r)
    lv = {v: j % r}
    key = j // r
    for p in ps:
        lv[p] = key % int(net.card[p])
        key = key // int(net.card[p])
    cell, stride = np.zeros(q * r, np.int64), 1
    for u in fam:
        cell += lv[u] * stride
        stride *= int(net.card[u])
    return cell


def chunk_tree(parts):
    """f64 [chunks, cells] -> [cells]: the library's tree over the chunk values"""
    return z_sum(np.ascontiguousarray(parts.T))


def loglik_tree(terms):
    """f64 [R] -> the sum in the order of dvs_bn_loglik"""
    R = len(terms)
    chunks = (R + 255) // 256
    padded = np.zeros(chunks * 256)
    padded[:R] = terms
    return float(z_sum(ic._tree(padded.reshape(chunks, 256))[None, :])[0])


Counts = namedtuple("Counts", "counts row_z loglik loglik_tol skipped status ok active")


def restate_counts(net, plans, levels, observed, tables=None):
    """dvs_bn_expected_counts as include/dvs_incomplete.h defines it -> Counts (loglik: the fsum reference and its tolerance
    term sum |log z|; active: the most active rows of a chunk per family)"""
    n, R = len(net.card), levels.shape[0]
    tables = net.tables if tables is None else tables
    masks, sound = row_masks(levels, observed), sound_rows(net, levels, observed)
    row_z = np.full(R, math.nan)
    if sound.any():
        row_z[sound] = execute_plan(plans[n].words, net.card, tables, masks[sound])[1]
    ok = sound & _positive(row_z)
    status = (16 if (~sound).any() else 0) | (128 if (sound & ~ok).any() else 0)
    seen = seen_of(observed, n)
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    counts = np.zeros(int(offsets[-1]))
    chunks = (R + 255) // 256
    most = []
    for v in range(n):
        fam = list(family(net, v))
        ps, q, r = pm.family_shape(net.card, net.masks[v], v)
        whole = ok & seen[:, fam].all(1)
        act = ok & ~seen[:, fam].all(1)
        idx = pm.config_keys(levels[whole], net.card, ps) * r + levels[whole, v].astype(np.int64)
        I = np.bincount(idx, minlength=q * r)
        F = np.zeros((chunks, q * r))
        cell = plan_cell_of(net, v)
        rows = np.flatnonzero(act)
        most.append(max([int(((rows // 256) == c).sum()) for c in range(chunks)], default=0))
        if len(rows):
            out, z = execute_plan(plans[v].words, net.card, tables, masks[rows])
            for i, row in enumerate(rows):
                if _positive(z[i]):
                    F[row // 256] = F[row // 256] + out[i, cell] / z[i]
                else:
                    status |= 128
        counts[int(offsets[v]):int(offsets[v + 1])] = I.astype(np.float64) + chunk_tree(F)
    logs = np.log(row_z[ok])
    return Counts(counts, row_z, math.fsum(logs), math.fsum(np.abs(logs)), int((~ok).sum()), status, ok, most)


def restated_loglik(c):
    """the log-likelihood of a Counts in the kernel's order, with numpy's log"""
    return loglik_tree(np.where(c.ok, np.log(np.where(c.ok, c.row_z, 1.0)), 0.0))


def counts_depth(plan, active, n_rows):
    chunks = (n_rows + 255) // 256
    return plan.z_depth + 1 + max(active - 1, 0) + (chunks + 255) // 256 - 1 + 8 + 1


def fit_counts_ref(net, counts, method, iss, unobserved):
    """dvs_bn_fit_counts in numpy: cpt f64 [n_cells]"""
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    out = np.empty(int(offsets[-1]))
    for v in range(len(net.card)):
        _, q, r = pm.family_shape(net.card, net.masks[v], v)
        c = counts[int(offsets[v]):int(offsets[v + 1])].reshape(q, r)
        if not (np.isfinite(c) & (c >= 0)).all():
            out[int(offsets[v]):int(offsets[v + 1])] = math.nan
            continue
        N = np.zeros(q)
        for k in range(r):
            N = N + c[:, k]
        if method == 1:
            a = float(iss) / (float(r) * float(q))
            th = (c + a) / (N + float(r) * a)[:, None]
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                th = np.where(N[:, None] != 0.0, c / N[:, None], 1.0 / float(r) if unobserved else math.nan)
        out[int(offsets[v]):int(offsets[v + 1])] = th.reshape(-1)
    return out


def tables_from(net, cpt):
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    return [np.ascontiguousarray(t) for t in pm.tables_of(cpt, net.card, net.masks[None, :], offsets)[0]]


def uniform_tables(net):
    return [np.full(t.shape, 1.0 / t.shape[1]) for t in net.tables]


def em_ref(net, plans, levels, observed, iterations, tables=None, method=0, iss=1.0):
    """soft EM in the restatement: ``iterations`` of (expected counts, tables from counts with unobserved = uniform) ->
    (tables, [(loglik in the kernel's order, its tolerance term)] of the tables each E-step saw)"""
    tables = uniform_tables(net) if tables is None else tables
    trace = []
    for _ in range(iterations):
        c = restate_counts(net, plans, levels, observed, tables)
        trace.append((restated_loglik(c), c.loglik_tol))
        tables = tables_from(net, fit_counts_ref(net, c.counts, method, iss, 1))
    return tables, trace


def restate_impute(net, plans, levels, observed):
    """dvs_bn_impute -> (levels_out u8 [R, n] with the nibbles it writes, observed_out u64 [R], status)"""
    n, R = len(net.card), levels.shape[0]
    masks, sound, seen = row_masks(levels, observed), sound_rows(net, levels, observed), seen_of(observed, n)
    out_levels = np.where(seen, levels & 15, 0).astype(np.uint8)
    seen_out = observed.copy()
    status = 16 if (~sound).any() else 0
    for v in range(n):
        rows = np.flatnonzero(sound & ~seen[:, v])
        if not len(rows):
            continue
        out, z = execute_plan(plans[v].words, net.card, net.tables, masks[rows])
        good = _positive(z)
        if (~good).any():
            status |= 128
        out_levels[rows[good], v] = np.argmax(out[good], axis=1)              # the first of equal maxima: the lowest level
        seen_out[rows[good]] |= U64(1) << U64(v)
    return out_levels, seen_out, status


# ---------------------------------------------------------------------------------------------------------------------
# Exact rationals
# ---------------------------------------------------------------------------------------------------------------------
def exact_counts(name, levels, observed):
    """[Fraction] in the CPT layout: the sum over rows of P(family cell | the row's observed values), by enumeration; every row
    must be ok"""
    net = network(name)
    n = len(net.card)
    masks, seen = row_masks(levels, observed), seen_of(observed, n)
    out = []
    for v in range(n):
        fam = list(family(net, v))
        ps, q, r = pm.family_shape(net.card, net.masks[v], v)
        cell = plan_cell_of(net, v)
        total = [Fraction(0)] * (q * r)
        for row in range(levels.shape[0]):
            if seen[row, fam].all():
                j = int(pm.config_keys(levels[row:row + 1], net.card, ps)[0]) * r + int(levels[row, v])
                total[j] += 1
                continue
            cells = exact_cells(name, masks[row], fam)
            z = sum(cells)
            assert z > 0
            for j in range(q * r):
                total[j] += cells[cell[j]] / z
        out += total
    return out


def exact_argmax(name, levels, observed, depth_of):
    """[(row, v, level)] the lowest level of the largest exact posterior for every missing value, and the number of (row, v)
    whose top two are within 2 gamma_D of the top, D = depth_of(v) (those are not decided by the exact answer)"""
    net = network(name)
    n = len(net.card)
    masks, seen = row_masks(levels, observed), seen_of(observed, n)
    picks, close = [], 0
    for row in range(levels.shape[0]):
        for v in range(n):
            if seen[row, v]:
                continue
            cells = exact_cells(name, masks[row], (v,))
            order = sorted(range(len(cells)), key=lambda k: (-cells[k], k))
            if len(cells) > 1 and cells[order[0]] - cells[order[1]] <= 2 * gamma(depth_of(v)) * cells[order[0]]:
                close += 1
            picks.append((row, v, order[0]))
    return picks, close


# ---------------------------------------------------------------------------------------------------------------------
# The raw calls
# ---------------------------------------------------------------------------------------------------------------------
def _guarded(be, shape, dtype, fill):
    a = np.full(int(np.prod(shape)) + 2 * GUARD, fill, dtype)
    return be.put(a), a.itemsize * GUARD


def _inner(be, h, fill):
    a = be.get(h).copy()
    return a[GUARD:-GUARD], bool((a[:GUARD] == fill).all() and (a[-GUARD:] == fill).all())


def _plans_args(be, words_list):
    words = np.concatenate([np.asarray(w, np.int32) for w in words_list])
    starts = np.concatenate([[0], np.cumsum([len(w) for w in words_list])]).astype(np.int64)
    header = lambda k: max(int(w[k]) for w in words_list if len(w) > k)
    return dict(plans=be.put(words), plan_offsets=be.put(starts), plans_bytes=words.nbytes,
                plan_words=max(len(w) for w in words_list), arena_cells=header(3), step_cells=max(_step_cells(w) for w in words_list)), header(4)


def _network_args(be, net, offsets=None, cpt=None):
    if offsets is None:
        offsets, cpt = pm.flat_network(net)
    return dict(n_vars=len(net.card), card=be.put(net.card), parents=be.put(net.masks), offsets=be.put(offsets), cpt=be.put(cpt),
                n_cells=int(offsets[-1] - offsets[0]))


def _data_args(be, levels, observed):
    return dict(n_rows=levels.shape[0], data=be.put(sc.pack(levels)), observed=be.put(observed.astype(U64)))


CountsOut = namedtuple("CountsOut", "rc counts row_z loglik skipped flags status guards_ok")


def run_expected_counts(be, net, words_list, levels, observed, rows_per_group=0, tables=None, offsets=None, cpt=None, **over):
    """one dvs_bn_expected_counts; every output sits between GUARD sentinel cells"""
    n = len(net.card)
    if offsets is None:
        offsets, cpt = pm.flat_network(net if tables is None else net._replace(tables=tables))
    at = lambda h, skip: ctypes.c_void_p(be.ptr(h).value + skip)
    plans, out_cells = _plans_args(be, words_list)
    net_args = _network_args(be, net, offsets, cpt)
    R, cells = levels.shape[0], net_args["n_cells"]
    ws_bytes = int(be.lib.dvs_bn_expected_counts_workspace_bytes(cells, n, R))
    assert ws_bytes > 0
    outs = dict(counts=_guarded(be, (cells,), np.float64, SENTINEL), row_z=_guarded(be, (R,), np.float64, SENTINEL),
                loglik=_guarded(be, (1,), np.float64, SENTINEL), skipped=_guarded(be, (1,), np.int64, -7),
                plan_flags=_guarded(be, (n + 1,), np.int32, 77))
    status = be.put(np.zeros(1, np.int32))
    outs["workspace"] = _guarded(be, (ws_bytes // 8,), np.int64, -1)               # the workspace between guards as well
    args = dict(**net_args, **plans, **_data_args(be, levels, observed), out_cells=out_cells, rows_per_group=rows_per_group,
                workspace_bytes=ws_bytes, status=status, **{k: at(h, skip) for k, (h, skip) in outs.items()})
    args.update(over)
    rc = call_rc(be, "dvs_bn_expected_counts", **args)
    fills = {"plan_flags": 77, "skipped": -7, "workspace": -1}
    got = {k: _inner(be, h, fills.get(k, SENTINEL)) for k, (h, _) in outs.items()}
    return CountsOut(rc, got["counts"][0], got["row_z"][0], float(got["loglik"][0][0]), int(got["skipped"][0][0]), got["plan_flags"][0],
                     int(be.get(status)[0]), all(g for _, g in got.values()))


def run_fit_counts(be, net, counts, method, iss, unobserved, offsets=None):
    """one dvs_bn_fit_counts -> (rc, cpt f64 [n_cells], status, guards_ok)"""
    net_args = _network_args(be, net, offsets, None if offsets is None else np.zeros(1))
    net_args.pop("cpt")
    out, skip = _guarded(be, (len(counts),), np.float64, SENTINEL)
    status = be.put(np.zeros(1, np.int32))
    rc = call_rc(be, "dvs_bn_fit_counts", **net_args, counts=be.put(np.asarray(counts, np.float64)), method=method, iss=float(iss),
                 unobserved=unobserved, cpt_out=ctypes.c_void_p(be.ptr(out).value + skip), status=status)
    cpt, guards = _inner(be, out, SENTINEL)
    return rc, cpt, int(be.get(status)[0]), guards


ImputeOut = namedtuple("ImputeOut", "rc data observed flags status guards_ok")


def run_impute(be, net, words_list, levels, observed, rows_per_group=0, **over):
    n, R = len(net.card), levels.shape[0]
    words = (n + 15) // 16
    at = lambda h, skip: ctypes.c_void_p(be.ptr(h).value + skip)
    plans, _ = _plans_args(be, words_list)
    ws_bytes = int(be.lib.dvs_bn_impute_workspace_bytes(n, R))
    assert ws_bytes > 0
    fill = 0xAAAAAAAAAAAAAAAA
    outs = dict(data_out=_guarded(be, (R, words), U64, fill), observed_out=_guarded(be, (R,), U64, fill),
                plan_flags=_guarded(be, (n,), np.int32, 77))
    status = be.put(np.zeros(1, np.int32))
    args = dict(**_network_args(be, net), **plans, **_data_args(be, levels, observed), rows_per_group=rows_per_group,
                workspace=be.put(np.full(ws_bytes // 8 + 1, -1, np.int64)), workspace_bytes=ws_bytes, status=status,
                **{k: at(h, skip) for k, (h, skip) in outs.items()})
    args.update(over)
    rc = call_rc(be, "dvs_bn_impute", **args)
    got = {k: _inner(be, h, 77 if k == "plan_flags" else fill) for k, (h, _) in outs.items()}
    return ImputeOut(rc, got["data_out"][0].reshape(R, words), got["observed_out"][0], got["plan_flags"][0], int(be.get(status)[0]),
                     all(g for _, g in got.values()))


# ---------------------------------------------------------------------------------------------------------------------
# Checks (emulator and device)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counts_case(name, n_rows):
    net = network(name)
    levels, observed = incomplete_case(name, n_rows)
    return levels, observed, restate_counts(net, family_plans(name), levels, observed)


@functools.lru_cache(maxsize=None)
def impute_case(name, n_rows):
    net = network(name)
    levels, observed = incomplete_case(name, n_rows)
    return levels, observed, restate_impute(net, target_plans(name), levels, observed)


def assert_counts(got, ref, what):
    assert (got.rc, got.guards_ok) == (0, True) and not got.flags.any(), (what, got.rc, got.guards_ok, got.flags)
    assert got.status == ref.status and got.skipped == ref.skipped, (what, got.status, ref.status, got.skipped, ref.skipped)
    _same(got.row_z, ref.row_z, (what, "row_z"))
    _same(got.counts, ref.counts, (what, "counts"))
    err = abs(got.loglik - ref.loglik)
    print(f"{what}: loglik {got.loglik!r}, error {err:.3g} of the bound {pm.LOG_RTOL * ref.loglik_tol:.3g}")
    assert err <= pm.LOG_RTOL * ref.loglik_tol, (what, got.loglik, ref.loglik)


def check_counts_bytes(be, name, n_rows, rows_per_group=(0,)):
    net = network(name)
    levels, observed, ref = counts_case(name, n_rows)
    words = [p.words for p in family_plans(name)]
    for G in rows_per_group:
        assert_counts(run_expected_counts(be, net, words, levels, observed, rows_per_group=G), ref, (name, n_rows, G))
    if n_rows > 3:
        assert ref.status & 16 and ref.skipped >= 1 and np.isnan(ref.row_z[3])           # the level at or above card
        if name == "zeroone":
            assert ref.status & 128 and ref.row_z[2] == 0.0                              # the impossible row


def assert_impute(got, ref, n, what):
    ref_levels, ref_seen, ref_status = ref
    assert (got.rc, got.guards_ok, got.status) == (0, True, ref_status) and not got.flags.any(), (what, got.rc, got.status, ref_status)
    _same(got.data, sc.pack(ref_levels), (what, "data_out"))
    _same(got.observed, ref_seen, (what, "observed_out"))


def check_impute_bytes(be, name, n_rows, rows_per_group=(0,)):
    net = network(name)
    levels, observed, ref = impute_case(name, n_rows)
    for G in rows_per_group:
        got = run_impute(be, net, [p.words for p in target_plans(name)], levels, observed, rows_per_group=G)
        assert_impute(got, ref, len(net.card), (name, n_rows, G))


def check_fully_observed(be, name, n_rows=300):
    """complete data: the counts are the integer family counts, and dvs_bn_fit_counts on them gives the bytes of dvs_bn_fit"""
    net = network(name)
    n = len(net.card)
    levels = pm.sample_ref(net, n_rows, seed=43)
    observed = np.full(n_rows, (1 << n) - 1, U64)
    got = run_expected_counts(be, net, [p.words for p in family_plans(name)], levels, observed)
    assert (got.rc, got.status, got.skipped, got.guards_ok) == (0, 0, 0, True)
    ints = np.concatenate([pm.family_counts(levels, net.card, net.masks[v], v).reshape(-1) for v in range(n)])
    _same(got.counts, ints.astype(np.float64), (name, "integer counts"))
    for method, iss, unobserved in ((0, 1.0, 0), (0, 1.0, 1), (1, 1.0, 0), (1, 10.0, 1)):
        rc, cpt, status, guards = run_fit_counts(be, net, got.counts, method, iss, unobserved)
        rc2, ref, status2 = pm.run_fit(be, levels, net.card, net.masks[None, :], method, iss, unobserved)
        assert (rc, status, guards, rc2, status2) == (0, 0, True, 0, 0), (name, method)
        _same(cpt, ref[:len(cpt)], (name, method, iss, unobserved, "fit_counts against dvs_bn_fit"))
        _same(cpt, fit_counts_ref(net, got.counts, method, iss, unobserved), (name, method, "fit_counts against the restatement"))


def check_fit_counts_fractional(be, name="asia"):
    """fractional counts, an empty configuration, and a family with a negative and one with a NaN count (NaN alone, bit 4)"""
    net = network(name)
    levels, observed, ref = counts_case(name, 257)
    counts = ref.counts.copy()
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    counts[int(offsets[7]):int(offsets[7]) + int(net.card[7])] = 0.0                   # a configuration never seen
    for method, iss, unobserved in ((0, 1.0, 0), (0, 1.0, 1), (1, 2.5, 0)):
        rc, cpt, status, guards = run_fit_counts(be, net, counts, method, iss, unobserved)
        assert (rc, status, guards) == (0, 0, True)
        _same(cpt, fit_counts_ref(net, counts, method, iss, unobserved), (name, method, unobserved))
    bad = counts.copy()
    bad[int(offsets[2])] = -1.0
    bad[int(offsets[5]) + 1] = math.nan
    rc, cpt, status, guards = run_fit_counts(be, net, bad, 0, 1.0, 1)
    assert (rc, status, guards) == (0, 16, True)
    want = fit_counts_ref(net, bad, 0, 1.0, 1)
    assert np.isnan(want[int(offsets[2]):int(offsets[3])]).all() and np.isnan(want[int(offsets[5]):int(offsets[6])]).all()
    _same(cpt, want, "bad counts")


def check_em_step(be, name="asia", n_rows=257, iterations=3):
    """a few EM iterations through the C ABI equal the restatement's byte for byte"""
    net = network(name)
    levels, observed = incomplete_case(name, n_rows, special=False)
    plans = family_plans(name)
    tables = uniform_tables(net)
    for it in range(iterations):
        ref = restate_counts(net, plans, levels, observed, tables)
        got = run_expected_counts(be, net, [p.words for p in plans], levels, observed, tables=tables)
        assert_counts(got, ref, (name, "EM iteration", it))
        rc, cpt, status, guards = run_fit_counts(be, net, got.counts, 0, 1.0, 1)
        assert (rc, status, guards) == (0, 0, True)
        _same(cpt, fit_counts_ref(net, ref.counts, 0, 1.0, 1), (name, "M-step", it))
        tables = tables_from(net, cpt)


def check_impute_equals_blanket(be, name, targets, n_rows=5):
    """every other variable observed: dvs_bn_impute gives the prediction of dvs_bn_blanket_posterior"""
    net = network(name)
    n = len(net.card)
    levels = pm.sample_ref(net, n_rows, seed=29)
    offsets, cpt = pm.flat_network(net)
    for t in targets:
        observed = np.full(n_rows, ((1 << n) - 1) & ~(1 << t), U64)
        got = run_impute(be, net, [p.words for p in target_plans(name)], levels, observed)
        ref = ic.run_blanket(be, levels, net.card, net.masks[None, :], offsets, cpt, t, 1)
        assert (got.rc, got.status, got.guards_ok, ref.rc, ref.status) == (0, 0, True, 0, 0)
        assert (got.observed == U64((1 << n) - 1)).all()
        assert np.array_equal(pm.unpack(got.data, n)[:, t], ref.pred[0]), (name, t)


def wrong_keep_plans(name="asia"):
    """{what: (slot, words)}: well-formed plans that keep the wrong variables for their slot"""
    return {"a family slot that keeps one variable": (4, plan_of(name, (4,)).words),
            "a family slot that keeps another family": (1, plan_of(name, family(network(name), 3)).words),
            "the evidence slot keeps a variable": (len(network(name).card), plan_of(name, (0,)).words)}


def malformed_words(good):
    """{what: words}: the cases of eliminate_corpus.malformed_plans on the plan ``good``, one thing wrong each"""
    w = [int(x) for x in good]
    first = 6 + w[5]
    ns = w[first + 3]
    bad = {}
    b = good.copy()
    b[first + 1] = w[3] - w[first + 2] + 1                       # the first step's output ends one cell beyond arena_cells
    bad["an arena span beyond arena_cells"] = b
    b = good.copy()
    b[first + 5 + ns + 3] += 1 << 20                             # stride_x of the first input (a table) leaves the table
    bad["a stride that leaves its table"] = b
    cur, j = next((cur, j) for cur, s_ns, s_ni in _steps(w) for j in range(s_ni)
                  if w[cur + 5 + s_ns + j * (4 + s_ns)] == -1 and w[cur] >= 0)
    b = good.copy()
    b[cur + 1] = w[cur + 5 + w[cur + 3] + j * (4 + w[cur + 3]) + 1]      # the output starts where one of its inputs lies
    bad["an output that overlaps an input"] = b
    return bad


def wider_last_step(good, card, extra):
    """``good`` with the variable ``extra`` added to the scope of its last step (stride 0 in every input) and the header's
    out_cells multiplied by its level count: every word is well formed and the kept list is untouched, but the last step has
    more cells than the slot's table"""
    w = [int(x) for x in good]
    cur = [c for c, _, _ in _steps(w)][-1]
    ns, ni = w[cur + 3], w[cur + 4]
    scope = w[cur + 5:cur + 5 + ns]
    assert w[cur] == -1 and extra not in scope
    at = sum(1 for u in scope if u < extra)
    cells = w[cur + 2] * int(card[extra])
    last = [-1, -1, cells, ns + 1, ni, *scope[:at], extra, *scope[at:]]
    for j in range(ni):
        inw = w[cur + 5 + ns + j * (4 + ns):cur + 5 + ns + (j + 1) * (4 + ns)]
        last += [*inw[:4 + at], 0, *inw[4 + at:]]
    out = w[:cur] + last
    out[4] = cells
    return np.asarray(out, np.int32)


def check_malformed(be, name="asia", n_rows=70):
    """a malformed family plan: bit 4, its flag, NaN counts for that family alone; a malformed evidence plan: nothing is ok"""
    net = network(name)
    n = len(net.card)
    levels, observed = incomplete_case(name, n_rows, special=False)
    good = [p.words for p in family_plans(name)]
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    ref = run_expected_counts(be, net, good, levels, observed)
    assert (ref.rc, ref.status, ref.guards_ok) == (0, 0, True)
    sized = dict(arena_cells=32, out_cells=64, step_cells=8, plan_words=400)
    same_sizes = run_expected_counts(be, net, good, levels, observed, **sized)
    _same(same_sizes.counts, ref.counts, "the call's size statements do not change the bytes")
    cases = dict(wrong_keep_plans(name))
    cases.update({what: (7, words) for what, words in malformed_words(good[7]).items()})
    # the right kept list over a larger last step, in the last family's slot: its cells would leave the table, the chunk's
    # partials and, in the last chunk, the workspace
    extra = next(u for u in range(n) if u not in family(net, n - 1))
    cases["a last step wider than the family's table"] = (n - 1, wider_last_step(good[n - 1], net.card, extra))
    cases["an evidence slot whose last step has cells"] = (n, wider_last_step(good[n], net.card, 0))
    cases["a wrong tag"] = (2, np.concatenate([[7], good[2][1:]]).astype(np.int32))
    cases["a truncated plan"] = (5, good[5][:-1])
    for what, (slot, words) in cases.items():
        plans = list(good)
        plans[slot] = words
        got = run_expected_counts(be, net, plans, levels, observed, **sized)
        assert (got.rc, got.status & 16, got.guards_ok) == (0, 16, True), (what, got.rc, got.status)
        want = [1 if v == slot else 0 for v in range(n + 1)]
        assert got.flags.tolist() == want, (what, got.flags)
        if slot == n:
            assert np.isnan(got.counts).all() and np.isnan(got.row_z).all() and math.isnan(got.loglik) and got.skipped == n_rows, what
            continue
        lo, hi = int(offsets[slot]), int(offsets[slot + 1])
        assert np.isnan(got.counts[lo:hi]).all(), what
        _same(np.delete(got.counts, np.s_[lo:hi]), np.delete(ref.counts, np.s_[lo:hi]), (what, "the other families"))
        _same(got.row_z, ref.row_z, (what, "row_z"))
        assert got.loglik == ref.loglik and got.skipped == ref.skipped, what
    # a table that does not match the structure refuses every plan
    off2, cpt = pm.flat_network(net)
    wrong = off2.copy()
    wrong[3:] += 2
    got = run_expected_counts(be, net, good, levels, observed, offsets=wrong, cpt=np.concatenate([cpt, [0.5, 0.5]]))
    assert (got.rc, got.status & 16, got.guards_ok) == (0, 16, True) and got.flags.all() and np.isnan(got.counts).all()
    # impute: plan v must keep exactly {v}
    tgt = [p.words for p in target_plans(name)]
    base = run_impute(be, net, tgt, levels, observed)
    assert (base.rc, base.status, base.guards_ok) == (0, 0, True)
    for what, (slot, words) in {"a pair kept": (4, plan_of(name, (4, 7)).words), "another variable kept": (2, tgt[3]),
                                "nothing kept": (6, plan_of(name, ()).words), "truncated": (0, tgt[0][:-1]),
                                "a last step with more cells than levels": (n - 1, wider_last_step(tgt[n - 1], net.card, 0))}.items():
        plans = list(tgt)
        plans[slot] = words
        got = run_impute(be, net, plans, levels, observed, arena_cells=32, step_cells=8, plan_words=400)
        assert (got.rc, got.status, got.guards_ok) == (0, 16, True) and got.flags.tolist() == [int(v == slot) for v in range(n)], (what, got.status)
        lv, ref_lv = pm.unpack(got.data, n), pm.unpack(base.data, n)
        seen = seen_of(observed, n)
        assert np.array_equal(np.delete(lv, slot, 1), np.delete(ref_lv, slot, 1)), what
        assert (lv[~seen[:, slot], slot] == 0).all() and np.array_equal(got.observed, base.observed & ~((~observed) & (U64(1) << U64(slot)))), what


# ---------------------------------------------------------------------------------------------------------------------
# Argument refusals (no device needed)
# ---------------------------------------------------------------------------------------------------------------------
def validation_cases(D):
    cases = []
    fn = "dvs_bn_expected_counts"
    ws = 1 << 20
    c = entry(fn, cases, n_vars=8, n_rows=100, card=D, parents=D, offsets=D, cpt=D, n_cells=36, plans=D, plans_bytes=252,
              plan_offsets=D, plan_words=200, arena_cells=17, out_cells=8, step_cells=8, data=D, observed=D, rows_per_group=0,
              counts=D, row_z=D, loglik=D, skipped=D, plan_flags=D, workspace=D, workspace_bytes=ws, status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=7)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=1 << 31)
    c(2, "ceil(n_rows / 256) * n_cells must be < 2^40", n_rows=(1 << 31) - 1, n_cells=(1 << 31) - 1)
    c(12, "plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", plan_words=6)
    c(12, "plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", plan_words=4097)
    for name in ("arena_cells", "out_cells", "step_cells"):
        c(12, "arena_cells, out_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", **{name: 0})
        c(12, "arena_cells, out_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", **{name: 16385})
    c(12, "arena_cells + out_cells = 16385 exceeds DVS_BN_ELIM_MAX_CELLS = 16384", arena_cells=16000, out_cells=385)
    c(12, "rows_per_group must be in [0, 64]", rows_per_group=-1)
    c(12, "rows_per_group must be in [0, 64]", rows_per_group=65)
    for name in ("card", "parents", "offsets", "cpt", "plans", "plan_offsets", "data", "observed", "counts", "row_z", "loglik",
                 "skipped", "plan_flags", "workspace", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "plans_bytes < (n_vars + 1) * 28 = 252", plans_bytes=251)
    c(14, "workspace_bytes < dvs_bn_expected_counts_workspace_bytes = ", workspace_bytes=100)
    c(3, "n_vars must be in", n_vars=49, n_cells=0)                                    # the order of the header
    c(2, "n_cells must be in", n_cells=0, n_rows=0)
    c(2, "n_rows must be in", n_rows=0, plan_words=0)
    c(12, "plan_words must be in", plan_words=0, arena_cells=0)
    c(12, "arena_cells, out_cells and step_cells", step_cells=0, arena_cells=16384, out_cells=16384)
    c(12, "arena_cells + out_cells", arena_cells=16384, out_cells=1, rows_per_group=65)
    c(12, "rows_per_group must be in", rows_per_group=65, card=None)
    c(10, "null pointer", status=None, plans_bytes=0)
    c(14, "plans_bytes <", plans_bytes=0, workspace_bytes=0)
    fn = "dvs_bn_fit_counts"
    c = entry(fn, cases, n_vars=8, card=D, parents=D, offsets=D, counts=D, n_cells=36, method=0, iss=1.0, unobserved=0, cpt_out=D,
              status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=49)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=7)
    c(12, "method is not a dvs_fit_method", method=2)
    c(13, "iss must be finite and > 0", method=1, iss=0.0)
    c(13, "iss must be finite and > 0", method=1, iss=math.inf)
    c(12, "unobserved must be 0 (NaN) or 1 (uniform)", unobserved=2)
    for name in ("card", "parents", "offsets", "counts", "cpt_out", "status"):
        c(10, "null pointer", **{name: None})
    c(3, "n_vars must be in", n_vars=0, n_cells=0)
    c(2, "n_cells must be in", n_cells=0, method=2)
    c(12, "method is not", method=2, unobserved=2, iss=-1.0)
    c(13, "iss must be", method=1, iss=-1.0, unobserved=2)
    c(12, "unobserved must be", unobserved=2, card=None)
    fn = "dvs_bn_impute"
    c = entry(fn, cases, n_vars=8, n_rows=100, card=D, parents=D, offsets=D, cpt=D, n_cells=36, plans=D, plans_bytes=224,
              plan_offsets=D, plan_words=200, arena_cells=17, step_cells=8, data=D, observed=D, rows_per_group=0, data_out=D,
              observed_out=D, plan_flags=D, workspace=D, workspace_bytes=1024, status=D, stream=None)
    c(3, "n_vars must be in [1, 48]", n_vars=0)
    c(2, "n_cells must be in [n_vars, 2^31 - 1]", n_cells=7)
    c(2, "n_rows must be in [1, 2^31 - 1]", n_rows=0)
    c(12, "plan_words must be in [7, DVS_BN_ELIM_MAX_WORDS = 4096]", plan_words=4097)
    c(12, "arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", arena_cells=0)
    c(12, "arena_cells and step_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = 16384]", step_cells=16385)
    c(12, "arena_cells + 16 = 16385 exceeds DVS_BN_ELIM_MAX_CELLS = 16384", arena_cells=16369)
    c(12, "rows_per_group must be in [0, 64]", rows_per_group=65)
    for name in ("card", "parents", "offsets", "cpt", "plans", "plan_offsets", "data", "observed", "data_out", "observed_out",
                 "plan_flags", "workspace", "status"):
        c(10, "null pointer", **{name: None})
    c(14, "plans_bytes < n_vars * 28 = 224", plans_bytes=223)
    c(14, "workspace_bytes < dvs_bn_impute_workspace_bytes = 1024", workspace_bytes=1023)
    c(2, "n_rows must be in", n_rows=0, plan_words=0)
    c(12, "plan_words must be in", plan_words=0, arena_cells=0)
    c(12, "arena_cells + 16", arena_cells=16384, rows_per_group=65)
    c(12, "rows_per_group must be in", rows_per_group=65, card=None)
    c(10, "null pointer", status=None, plans_bytes=0)
    c(14, "plans_bytes <", plans_bytes=0, workspace_bytes=0)
    return cases


def check_argument_refusals(lib, D=None):
    D = ctypes.c_void_p(4096) if D is None else D                                # never dereferenced
    run(lib, validation_cases(D))
    assert lib.dvs_bn_expected_counts_workspace_bytes(36, 8, 0) == 0 and b"n_rows" in lib.dvs_last_error()
    assert lib.dvs_bn_expected_counts_workspace_bytes(36, 49, 10) == 0 and lib.dvs_bn_impute_workspace_bytes(0, 10) == 0
    up = lambda x: (x + 255) & ~255
    assert lib.dvs_bn_expected_counts_workspace_bytes(36, 8, 600) == up(3 * 36 * 8) + up(36 * 4) + up(3 * 8) + up(3 * 4) + up(600)
    assert lib.dvs_bn_impute_workspace_bytes(8, 100) == 1024
