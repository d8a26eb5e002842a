"""TEST HELPER: cases, float64 reference, derived tolerance and the checks that pin the NUMBERS of dvs_decode
(csrc/k_decode.hip: k_decode_memory, the decoder stack on partial graphs with padding tokens, decode_hidden's final
LayerNorm out of fragment-ordered tiles, k_decode_step's __expf softmax / sigmoid and double-precision inverse CDF) on
both backends.  tests/test_emu_decode_margins.py (emulator build, -m "not gpu") and tests/test_gpu_decode_margins.py (C ABI
on the device) import the same cases AND the same check functions; they differ only in the backend that moves buffers
(scoring_corpus.EmuBackend / GpuBackend) and in the batch.

Why the sampled graphs alone pin little.  A random uniform lands within 1e-4 of a decision threshold once in 10^4 draws,
so a decode whose probabilities are off by 1e-3 still returns the oracle's graphs under random uniforms.  Here the test
steers the uniforms instead (oracle.decode.tight_uniforms): every uniform lies a chosen distance tau from the threshold
the FLOAT64 reference computes at that point of ITS OWN growing graph, on a side drawn in advance.  A device probability
that is off by more than tau towards the uniform flips that decision, the grown graph differs, and the case fails naming
row, step and candidate.  Sides are drawn independently per decision and a batch has many rows, so a systematic error is
met from both sides.

Reference.  oracle.decode.decode_trace in torch.float64 (parameters, z and features cast; the same loop oracle.decode
runs in float32 for the older graph-for-graph tests).

Tolerance: derived from the reference alone, never from the code under test.
    tau(case) = max(32 * d32, 1e-6)
    d32       = largest |float32 oracle - float64 oracle| over the node-type probabilities and edge scores of the rows
                that still grow, along the float64 path of that case (the float32 oracle is evaluated on the float64
                run's partial graphs, step by step)
    32        covers the device's different rounding of the same fp32 chain: fixed-order lane sums, three-way split-bf16
              products, __expf
    1e-6      keeps tau above a few float32 ulps of a uniform near 1
The path depends on tau only through forced sides and class eligibility, so tau is found by iteration: start at the
floor, regenerate while the path's own 32 * d32 exceeds the tau it was drawn with (random-init cases: the path does not
move, the second run confirms the first).  On random-init cases tau may not exceed TAU_CAP = 2e-5 — one tenth of the
2e-4 the suite allows on the decoder output.

Measured (the reference alone, device batches: 8 rows, n45c45 4): d32 of the node probabilities 1.1e-8 .. 7.0e-8 and of
the edge scores 4.8e-8 .. 1.0e-7 on the random-init cases, so tau = 1.5e-6 .. 3.3e-6 there (the same at 1 029 rows of
n12c12); asia d32 = 5.3e-8 (edge scores; nearly all of them sit at 0 or 1 to within 1e-8 along this path), tau = 1.7e-6,
and 42 % of its decisions are forced to a side (152 of 360: the pin there is one-sided, tau from 0 or 1).  The emulator
build and an MI355X pass every case at these tau with the factor 32 as it stands: it was never raised.  The last-step
ladder (report only: earlier steps at 1e-4, the last step at each tau of {1e-7 .. 1e-4}; the smallest at which every
last-step decision agrees) gives 1e-7, its lowest rung, on both backends for n12c12, n14c14 and asia.  That the checks
bite was shown on scratch emulator builds with the edge sigmoid of k_decode_step times (1 + 1e-4) and with
decode_hidden's rstd times (1 + 1e-4): the two older decode-vs-oracle tests pass on both, all nine random-init cases
here fail naming row, step and candidate, and the ladder reads 1e-4 and 1e-5 (asia passes on both, a
relative 1e-4 moves no saturated score across a threshold).

Counter draws.  With uniforms = NULL the library draws for itself (site 200 of its counter-based generator);
oracle.rng.decode_uniforms restates that stream, and the float64 reference under it must give the library's graphs, at
dag_offset 0 and continued at dag_offset k.  These uniforms cannot be steered, so a row in which some deciding draw lies
within TAU_CAP (the largest tau any random-init case may have) of its reference threshold is left out; COUNTER_SEED is
chosen so that no row is (smallest margin of its 8 rows: 2.5e-4 on n12c12, 1.5e-4 on n14c14), which the not-gpu run
asserts.

Cases: the smallest shapes at which each mechanism can go wrong (CASES below).  Row roles are fixed by row index so
that every path runs on purpose: rows b % 4 != 3 grow to full size, rows b % 4 == 3 sample `output` at a seeded step
and stop (loose ends hooked), and at the last step even rows take `output`, odd rows another class — both arms of the
reference's last-vertex quirk.
"""
import ctypes
import functools
from collections import namedtuple

import numpy as np
import torch

from dags_vae_search_amd import _lib as dl
from oracle import decode as odec
from oracle import pace_oracle as po
from oracle import rng as orng
from tests.abi_cases import call
from tests.helpers import load_golden

TAU_FACTOR = 32.0
TAU_FLOOR = 1e-6
TAU_CAP = 2e-5             # random-init cases; also the exclusion distance of the counter-draw rows
LADDER = (1e-7, 3e-7, 1e-6, 3e-6, 1e-5, 3e-5, 1e-4)

# name: (golden or None, n, card, emulator batch, device batch, why)
CASES = {
    "n1c1": (None, 1, 1, 4, 8, "N = 4, C = 4: two steps, the smallest legal shape"),
    "n12c12": ("n12c12", 12, 12, 4, 8, "N = 15, C = 15: the benchmark shape, a padding row in the tile"),
    "n13c13": (None, 13, 13, 4, 8, "N = 16, C = 16: full tile, C at the one-tile limit"),
    "n12c14": (None, 12, 14, 4, 8, "N = 15, C = 17: C alone sends a short graph to the wide path"),
    "n13c5": ("n13c5", 13, 5, 4, 8, "N = 16, C = 8: full tile, no padding row"),
    "n14c14": ("n14c14", 14, 14, 4, 8, "N = 17, C = 17: one valid row in the second tile"),
    "n29c7": ("n29c7", 29, 7, 4, 8, "N = 32, C = 10: two full tiles"),
    "n30c3": (None, 30, 3, 4, 8, "N = 33, C = 6: the first three-tile shape"),
    "n45c45": ("n45c45", 45, 45, 2, 4, "N = 48, C = 48: both maxima, bit 47 of the parent rows"),
    "asia": ("asia", 8, 8, 4, 8, "N = 11, C = 11, shipped checkpoint: saturated probabilities, one-sided pin"),
}
CASE_NAMES = list(CASES)
GRID_CASE = "n12c12"       # device only: batch 4 * CUs + 5, tight draws past one pass of the persistent grid
LADDER_CASES = ["n12c12", "n14c14", "asia"]
COUNTER_CASES = ["n12c12", "n14c14"]
COUNTER_SEED = 3           # every one of COUNTER_ROWS rows clears TAU_CAP on both cases (asserted, not-gpu run)
COUNTER_ROWS = 8

Case = namedtuple("Case", "name cfg params z tau d32_node d32_edge U graphs forced decisions trace")


def case_inputs(name, B):
    """(cfg, float32 parameters, z float32 [B, 32]): the committed golden where there is one (z = its eval/mu rows, repeated
    when the batch is larger), else fresh-seed parameters (po.init_params(seed=5), as test_emu_edge_sizes_forward_and_gradients)
    and seeded normal z."""
    golden, n, card = CASES[name][:3]
    if golden is not None:
        cfg, params, _, z = load_golden(golden)
        mu = z["eval/mu"]
        zz = np.ascontiguousarray(mu[np.arange(B) % len(mu)], np.float32)
    else:
        cfg = po.PaceConfig(n=n, card=card)
        params = po.init_params(cfg, seed=5)
        zz = np.random.default_rng(100 + n * 64 + card).standard_normal((B, 32)).astype(np.float32)
    assert (cfg.n, cfg.card) == (n, card)
    return cfg, params, zz


class _D32:
    """observe hook of tight_uniforms: the float32 oracle on the float64 run's partial graphs."""

    def __init__(self, cfg, params, z):
        self.cfg = cfg
        self.P, z32 = odec._cast(params, torch.from_numpy(z), torch.float32)
        with torch.no_grad():
            self.memory = odec.decode_memory(self.P, cfg, z32)
        self.node = self.edge = 0.0

    def __call__(self, idx, graphs, probs, score):
        alive = np.array([not g.finished for g in graphs])
        if not alive.any():
            return
        with torch.no_grad():
            p32, s32 = odec.step_probabilities(self.P, self.cfg, self.memory, graphs, idx)
        self.node = max(self.node, float(np.abs(p32.astype(np.float64) - probs)[alive].max()))
        self.edge = max(self.edge, float(np.abs(s32.astype(np.float64) - score)[alive].max()))


def _draws(cfg, params, z, seed, tau, **kw):
    d = _D32(cfg, params, z)
    U, graphs, forced, td = odec.tight_uniforms(params, cfg, torch.from_numpy(z), np.random.default_rng(seed), tau,
                                                observe=d, **kw)
    return U, graphs, forced, td, d


@functools.lru_cache(maxsize=None)
def case(name, B):
    """The case at batch B: inputs, tau by the iteration of the module docstring, bracketing uniforms and the float64
    reference's graphs.  Built once per process and shared; nothing in it is written again."""
    cfg, params, z = case_inputs(name, B)
    seed = 7000 + CASE_NAMES.index(name)
    tau = TAU_FLOOR
    for _ in range(6):
        U, graphs, forced, td, d = _draws(cfg, params, z, seed, tau)
        need = max(TAU_FACTOR * max(d.node, d.edge), TAU_FLOOR)
        if need <= tau:
            break
        tau = need
    else:
        raise AssertionError(f"{name}: tau did not settle ({tau:g})")
    U.setflags(write=False)
    return Case(name, cfg, params, z, tau, d.node, d.edge, U, graphs, forced, td.decisions, td)


# ---------------------------------------------------------------------------------------------------------------------
# the library under test
# ---------------------------------------------------------------------------------------------------------------------
def run_decode(be, cfg, params, z, U=None, seed=0, dag_offset=0, calls=1):
    """dvs_decode through the C ABI on backend `be`: `calls` raw state arrays uint8 [B, DECODE_STATE_BYTES].  Workspace and
    records are reused between the calls (the second call meets what the first left there); every state buffer is pre-filled
    with 0xA5, so the zero tails are the library's."""
    lib = be.lib
    B = len(z)
    shape = dl.make_shape(B, cfg.N, cfg.C, False, 0.15, dag_offset=dag_offset, seed=seed)
    table, P = dl.param_table(lib, shape)
    flat = np.zeros(P, np.float32)
    for nm, off, shp in table:
        v = np.asarray(params[nm], np.float32).reshape(-1)
        flat[off:off + v.size] = v
    ws_words = lib.dvs_workspace_bytes(ctypes.byref(shape)) // 4 + 64
    hf, hw = be.put(flat), be.put(np.zeros(ws_words, np.float32))
    hr = be.put(np.zeros(B * dl.record_bytes(lib, shape), np.uint8))
    hz = be.put(np.ascontiguousarray(z, np.float32))
    hu = None if U is None else be.put(np.ascontiguousarray(U, np.float32))
    assert U is None or U.shape == (B, cfg.N, cfg.N)
    out = []
    for _ in range(calls):
        hs = be.put(np.full(B * dl.DECODE_STATE_BYTES, 0xA5, np.uint8))
        call(be, "dvs_decode", s=ctypes.byref(shape), params=hf, n_params=P, workspace=hw, workspace_bytes=ws_words * 4, records=hr,
             records_bytes=B * dl.record_bytes(lib, shape), z=hz, uniforms=hu, state_out=hs, state_bytes=B * dl.DECODE_STATE_BYTES)
        out.append(np.array(be.get(hs)).reshape(B, dl.DECODE_STATE_BYTES))
    return out


def expected_states(graphs):
    """The whole dvs_decode_state of every reference graph: parents words, labels, nv, finished, and zeros beyond nv as
    k_decode_init leaves them."""
    raw = np.zeros((len(graphs), dl.DECODE_STATE_BYTES), np.uint8)
    for b, g in enumerate(graphs):
        par = np.zeros(48, np.uint64)
        for u, v in g.edges:
            assert u < v < g.nv
            par[v] |= np.uint64(1) << np.uint64(u)
        raw[b, :384] = par.view(np.uint8)
        raw[b, 384:384 + g.nv] = g.labels
        raw[b, 432:440] = np.array([g.nv, int(g.finished)], np.int32).view(np.uint8)
    return raw


def _fields(row):
    return row[:384].copy().view(np.uint64), row[384:432], row[432:440].copy().view(np.int32)


def describe_differences(c, got, want, U=None):
    """One line per differing row: the first step whose decision differs, which candidate, and what the reference had
    there (probability / score, the uniform, the distance between them)."""
    U = c.U if U is None else U
    N, lines = c.cfg.N, []
    for b in range(len(want)):
        if np.array_equal(got[b], want[b]):
            continue
        gp, gl, gm = _fields(got[b])
        wp, wl, wm = _fields(want[b])
        step = next((v for v in range(2, 48) if gl[v] != wl[v] or gp[v] != wp[v]), None)
        head = f"row {b}: nv {gm[0]} / finished {gm[1]} (reference {wm[0]} / {wm[1]})"
        if step is None or step >= N or step not in c.trace.probs:
            lines.append(head + "; differs outside the sampled vertices")
            continue
        u0 = float(U[b, step, 0])
        cdf = odec.node_cdf(c.trace.probs[step][b])
        if gl[step] != wl[step] or (step == N - 1 and gm[1] != wm[1]):     # last step: finished iff the type was `output`
            lines.append(head + f"; step {step}, candidate node type: label {gl[step]} (reference {wl[step]}), u = {u0!r}, "
                         f"nearest reference cdf edge at distance {float(np.abs(cdf - u0).min()):.3g}")
            continue
        for j in range(48):
            if (int(gp[step]) ^ int(wp[step])) >> j & 1:
                vi = j - 1
                if 0 <= vi < c.trace.score[step].shape[1]:
                    s, u = float(c.trace.score[step][b, vi]), float(U[b, step, 1 + vi])
                    lines.append(head + f"; step {step}, candidate edge vi = {vi} (vertex {j} -> {step}): got "
                                 f"{int(gp[step]) >> j & 1}, reference score {s!r}, u = {u!r}, margin {abs(s - u):.3g}")
                else:
                    lines.append(head + f"; step {step}: parent bit {j} differs (no such candidate)")
    return lines


def check_states(c, got, want=None, U=None):
    want = expected_states(c.graphs) if want is None else want
    if not np.array_equal(got, want):
        lines = describe_differences(c, got, want, U)
        rows = int((got != want).any(axis=1).sum())
        raise AssertionError(f"{c.name} (tau {c.tau:.3g}): {rows} of {len(want)} rows differ from the float64 reference\n" +
                             "\n".join(lines[:12]))


def check_reference_conditions(c):
    """Conditions on the reference alone (not-gpu run): tau within its cap, no forced side on a random-init case, every
    grower row at full size, an early finisher where the batch has one, both last-step arms present."""
    if c.name == "asia":
        return
    assert TAU_FLOOR <= c.tau <= TAU_CAP, (c.name, c.tau)
    assert c.forced == 0, (c.name, c.forced)
    N = c.cfg.N
    for b, g in enumerate(c.graphs):
        if b % 4 != 3:
            assert g.nv == N and g.finished == (b % 2 == 0), (c.name, b, g.nv, g.finished)
        else:
            assert g.finished and g.nv == c.trace.early[b] + 1 < N, (c.name, b, g.nv)


def check_case(be, c, twice=True):
    """The whole dvs_decode_state of every row equals the float64 reference under the bracketing uniforms; a second call
    leaves the same bytes."""
    out = run_decode(be, c.cfg, c.params, c.z, c.U, calls=2 if twice else 1)
    check_states(c, out[0])
    assert np.array_equal(out[0], out[-1]), f"{c.name}: a second call gave other bytes"


def report_line(c):
    return (f"decode {c.name} B={len(c.z)}: d32 node {c.d32_node:.3g} edge {c.d32_edge:.3g}, tau {c.tau:.3g}, "
            f"forced {c.forced} of {c.decisions} decisions ({100.0 * c.forced / max(c.decisions, 1):.1f} %)")


# ---------------------------------------------------------------------------------------------------------------------
# last-step ladder (report only)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder_case(name, B):
    """The case drawn again for the ladder: every step BEFORE the last keeps the ladder's top distance (so that a backend
    whose error lies anywhere on the ladder still grows the reference's graphs up to the last step), and forcing and class
    eligibility are judged at that distance too, so that every rung has the same sides and the same reference graphs; only
    the distance of the LAST step's draws changes between rungs."""
    c = case(name, B)
    top = max(LADDER[-1], c.tau)
    U, graphs, forced, td, _ = _draws(c.cfg, c.params, c.z, 9000 + CASE_NAMES.index(name), top, floor_tau=top)
    return c._replace(U=U, graphs=graphs, forced=forced, decisions=td.decisions, trace=td)


def last_step_ladder(be, name, B):
    """[(tau, all last-step decisions agree)] over LADDER and the smallest agreeing tau (None: none).  Asserts only that
    agreement is monotone in tau (same sides on every rung: a decision that holds at tau holds at every larger one)."""
    c = ladder_case(name, B)
    want = expected_states(c.graphs)
    # one call decodes every rung: the rows of rung r are rows [r * B, (r + 1) * B) of the batch
    U = np.concatenate([c.trace.with_last_step_at(tau) for tau in LADDER])
    got, = run_decode(be, c.cfg, c.params, np.tile(c.z, (len(LADDER), 1)), U)
    agree = [bool(np.array_equal(got[r * B:(r + 1) * B], want)) for r in range(len(LADDER))]
    assert agree == sorted(agree), (name, list(zip(LADDER, agree)))
    return list(zip(LADDER, agree)), next((t for t, a in zip(LADDER, agree) if a), None)


# ---------------------------------------------------------------------------------------------------------------------
# the library's own counter-based draws (uniforms == NULL)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def counter_reference(name):
    """(cfg, params, z [COUNTER_ROWS, 32], expected states, per-row margin) under oracle.rng.decode_uniforms(COUNTER_SEED)
    at dag_offset 0, float64 reference.  margin[b]: the smallest distance of a deciding draw of row b from its threshold."""
    cfg, params, z = case_inputs(name, COUNTER_ROWS)
    mt = odec.MarginTrace(orng.decode_uniforms(COUNTER_SEED, COUNTER_ROWS, cfg.N, 0))
    graphs = odec.decode_trace(params, cfg, torch.from_numpy(z), mt, torch.float64)
    return cfg, params, z, expected_states(graphs), mt.margin


def check_counter_draws(be, name, B, k):
    """uniforms = NULL: rows [0, B) at dag_offset 0 equal the reference under decode_uniforms; rows [k, B) decoded alone at
    dag_offset k equal the same rows of the offset-0 call (an ignored dag_offset would give them the draws of rows
    [0, B - k)).  Rows with a draw within TAU_CAP of a reference threshold are left out of the first equality (the not-gpu
    run asserts that COUNTER_SEED leaves out none)."""
    cfg, params, z, want, margin = counter_reference(name)
    assert 0 < k < B <= COUNTER_ROWS
    got, = run_decode(be, cfg, params, z[:B], None, seed=COUNTER_SEED, dag_offset=0)
    keep = margin[:B] > TAU_CAP
    assert keep.any()
    bad = [b for b in range(B) if keep[b] and not np.array_equal(got[b], want[b])]
    assert not bad, f"{name}: rows {bad} differ from the reference under the restated counter draws"
    tail, = run_decode(be, cfg, params, z[k:B], None, seed=COUNTER_SEED, dag_offset=k)
    assert np.array_equal(tail, got[k:]), f"{name}: dag_offset {k} does not continue the offset-0 stream"
