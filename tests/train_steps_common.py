"""TEST HELPER: one train step checked as a TRANSITION against the float64 oracle.  Plain numpy / torch on the CPU, no GPU.
tests/test_gpu_train_steps.py (PaceVaeV3 + optim.Adam + train_batch on the device) and tests/test_emu_train_steps.py (the
C ABI on the host emulator) share the reference and the checks, as the scoring tests share tests/scoring_corpus.py.

Method.  A free-running float32 run and a float64 run drift apart: Adam normalises entries whose gradient is rounding noise
to +-lr (test_gpu_module.py: check_step).  So every step k of a multi-step run is compared on its own, teacher-forced: the
reference starts from the state the DEVICE had before the step (parameters, moments, step counts, lr, mask seed), takes one
step in float64, and is compared with the state the device has after it.  Single-step tolerances then hold at every k.

Reference of step k: oracle.pace_oracle.loss_direct in float64, training=True, masks and eps from
DeviceMasks((seed << 32) | (model step before + 1), 0.15, dag_offset); backward; global norm; clip coefficient; Adam at
step (optimiser steps before + 1) from the before-moments.

Checks (check_transition)
  1. loss: total and kld within 1e-4 relative, recon within 1e-4 * max(1, |recon|) (the bounds of
     test_gpu_module.test_loss_direct_and_autograd_match_reference_golden).
  2. gradient: after the fused step the gradient buffer holds the CLIPPED gradient (k_adam clips in place); per tensor it is
     within GRAD_BOUND of (oracle gradient on the device's linear piece) x (the device's own coefficient, clip_scratch[1]);
     relu_flips <= max(4, 2e-5 * relu_units); units within float32 resolution of their kink get both sides tried where the
     bound is missed (as test_gpu_mapping_parity.mapping_parity).
  3. norm and coefficient: sqrt(clip_scratch[0]) and clip_scratch[1] within 1e-4 relative of the oracle's
     (test_train_mode_dropout0_injected_eps_and_one_step's bound).  Also clip_scratch[0] against the sum of squares of the
     device's OWN gradient (the clipped buffer divided by the coefficient): SS_SELF_RTOL, derived below.
  4. state carry, EVERY entry: exp_avg, exp_avg_sq and the parameters after the step against torch.optim.Adam in float64
     (scoring_corpus.adam_ref) from the device's own before-state, its own clipped gradient, lr and step k.  The gradient is
     the device's, so entries whose gradient is noise are pinned like all others.
  5. counters: optimiser step, model step (mask counter) and the host notification's sequence number each moved by one.

Tolerance of check 4.  scoring_corpus.check_clip_adam derives, for float32 results of k_adam, 8 * 2^-24 of the absolute
terms each quantity is made of (at most 8 roundings, no cancellation beyond those terms):
      exp_avg      8 * 2^-24 * (b1 |m| + (1 - b1) |g|)
      exp_avg_sq   8 * 2^-24 * (b2 v + (1 - b2) g^2)
      parameters   8 * 2^-24 * (|p| + |update|)
That test gives exp_avg the gradient's sign, so nothing cancels and |update| is its own absolute term.  In a real run b1 m and
(1 - b1) g do cancel (measured: to 1 / 4000 of their size in one fc2.weight entry at step 3 of the n = 14 case, which missed
the line above by a factor 2 on the device and 1.5 on the emulator), and the update, a ratio exp_avg / denominator, inherits
exp_avg's absolute terms:
      parameters   8 * 2^-24 * (|p| + lr / (1 - b1^k) * (b1 |m| + (1 - b1) |g|) / (sqrt(v') / sqrt(1 - b2^k) + eps))
There is no clip-coefficient term here: g is the clipped gradient the device itself stored, bit for bit.  That derivation
leaves the bias corrections out because they fit at its step 7.  At small k they do not: the library computes
1 - powf(b, k) in float32, powf is within one ulp (2 * 2^-24 relative) of b^k, and the subtraction turns that into
b^k / (1 - b^k) ulps of the difference: 999 for b2 = 0.999 at k = 1, 9 for b1 = 0.9.  The update is proportional to
sqrt(1 - b2^k) / (1 - b1^k), so the parameters get the extra relative term
      2 * 2^-24 * (b1^k / (1 - b1^k) + b2^k / (2 (1 - b2^k))) * |update|                (scoring_corpus.bias_correction_rounding)
which is 6.1e-5 |update| at k = 1 and falls like 1 / k.  lr, the betas and eps are the float32 values the ABI carries.  A
result below 2^-126 rounds absolutely (2^-150 per rounding): the floor 8 * 2^-150 covers exp_avg_sq of entries whose
gradient is ~1e-20.

SS_SELF_RTOL.  clip_scratch[0] is a float32 sum of P non-negative squares: at most 256 additions inside one partial (one per
256 entries, whatever their order), ceil(parts / 256) per lane of k_adam and 8 tree levels, plus 2 roundings for the square
itself and 2 for each clipped entry being g * coef rounded: (256 + 16 + 8 + 4) * 2^-24 = 1.7e-5.  A stale set of partials
differs by the change of the gradient between two steps with different masks, percents.

Free run.  FreeRun steps a float64 OracleTrainer freely from the initial parameters with the same masks; its loss is
recorded next to the device's at every step (free_gap).  Nothing is asserted on it: drift is a measurement.
"""
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import pace_oracle as po
from oracle.rng import DeviceMasks
from tests import relu_trace as rt
from tests.scoring_corpus import F32_EPS, adam_ref, adam_tolerances, bias_correction_rounding
from tests.test_gpu_module import GRAD_BOUND

F64 = torch.float64
DROPOUT = 0.15
BETA = 0.005
BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8
MAX_NORM = 1.0
UNDERFLOW = 8 * 2.0 ** -150
SS_SELF_RTOL = (256 + 16 + 8 + 4) * F32_EPS


class State(NamedTuple):
    """What lives from one step to the next, read from the device (copies)."""
    flat: np.ndarray                # parameters, float32 [P], in the C layout (`table` slices it by name)
    exp_avg: np.ndarray
    exp_avg_sq: np.ndarray
    opt_steps: int                  # Adam steps taken
    lr: float                       # the param group's lr
    seed: int                       # high word of the mask seed
    model_step: int                 # low word: PaceVaeV3._step
    host_seq: Optional[int] = None  # sequence number in the host notification packet (None: no packet on this path)


class DeviceStep(NamedTuple):
    """What one step on the device reported."""
    total: float
    recon: float
    kld: float
    grads: np.ndarray               # gradient buffer after the step: clipped in place, float32 [P]
    ss: float                       # clip_scratch[0]: sum of squares of the unclipped gradient
    coef: float                     # clip_scratch[1]


def named(table, flat):
    """{state-dict name: tensor view} of a flat numpy buffer in the C layout."""
    return {name: torch.from_numpy(flat[off:off + int(np.prod(shp))].reshape(shp)) for name, off, shp in table}


def step_masks(state, dag_offset=0):
    """the masks of the step that FOLLOWS `state`: PaceVaeV3._next_seed increments the step, then (seed << 32) | step"""
    return DeviceMasks((state.seed << 32) | ((state.model_step + 1) & 0xFFFFFFFF), DROPOUT, dag_offset=dag_offset)


class EmuActivations:
    """What relu_trace.device_relu_masks asks of a model (model._engine.activation(B, slot)), over a tests.emu EmuModel."""

    def __init__(self, emu_model):
        self._m, self._engine = emu_model, self

    def activation(self, B, slot):
        return torch.from_numpy(self._m.activation(slot))


class FreeRun:
    """The float64 OracleTrainer run freely from the initial parameters (recorded, never asserted)."""

    def __init__(self, cfg, params, lr):
        self.tr = po.OracleTrainer(cfg, params, lr=lr, max_grad_norm=MAX_NORM, dtype=F64)

    def step(self, feats, masks, lr):
        self.tr.opt.param_groups[0]["lr"] = lr
        B = feats["vertex_label_features"].shape[0]
        _, f64, eps = rt.as_dtype({}, feats, torch.from_numpy(masks.eps(B)), F64)
        return self.tr.step(f64, training=True, eps=eps, masks=masks)[0]


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-12)


def check_transition(tag, cfg, table, before, after, dev, feats, acts, free=None, dag_offset=0):
    """One step on the device, `before` -> `after`, against the float64 reference from `before` (module docstring).  `feats`:
    the batch as CPU tensors; `acts`: the model whose saved activations belong to this step's forward
    (relu_trace.device_relu_masks).  Records every figure through relu_trace.record under `tag`, then asserts."""
    B = feats["vertex_label_features"].shape[0]
    k = before.opt_steps + 1
    masks = step_masks(before, dag_offset)
    eps = torch.from_numpy(masks.eps(B))
    params = named(table, before.flat)
    # ---- 1, 2: loss and gradient on the device's linear piece ------------------------------------------------------
    t, kl, g_piece, _, info = rt.oracle_on_device_piece(acts, params, cfg, feats, B, True, eps=eps, masks=masks, dtype=F64)
    t, kl = float(t), float(kl)
    recon = t - BETA * kl
    got = named(table, dev.grads)
    ref = {n: g * dev.coef for n, g in g_piece.items()}
    grad_err, worst, _ = rt.grad_errors(got, ref)
    if grad_err >= GRAD_BOUND:
        P, f64, e64 = rt.as_dtype(params, feats, eps, F64)
        trace = rt.ReluTrace()
        rt.run_oracle(P, cfg, f64, True, e64, masks, trace)
        side0 = rt.device_relu_masks(acts, params, cfg, B, trace.aux["pairs"])
        units, flipped = rt.sub_resolution_units(trace), []
        for _, name, i in units:
            side = {n: m.clone() for n, m in side0.items()}
            side[name][i] = ~side[name][i]
            g = rt.run_oracle(P, cfg, f64, True, e64, masks, rt.ReluTrace(override=side))[2]
            flipped.append({n: x * dev.coef for n, x in g.items()})
        grad_err, worst, n_sides = rt.best_tie_sides(got, ref, flipped)
        info["relu_flips"] += n_sides
    # ---- 3: norm and coefficient ---------------------------------------------------------------------------------------
    norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in g_piece.values()))
    coef = min(1.0, MAX_NORM / (norm + 1e-6))
    ss_own = float((dev.grads.astype(np.float64) ** 2).sum()) / dev.coef ** 2
    # ---- 4: state carry ---------------------------------------------------------------------------------------------
    hyper = tuple(float(np.float32(x)) for x in (before.lr, *BETAS, ADAM_EPS))
    _, _, m_ref, v_ref, p_ref = adam_ref(before.flat, dev.grads, before.exp_avg, before.exp_avg_sq, k, hyper)
    upd = np.abs(p_ref - before.flat.astype(np.float64))
    lr, b1, b2, adam_eps = hyper
    m_terms = b1 * np.abs(before.exp_avg.astype(np.float64)) + (1 - b1) * np.abs(dev.grads.astype(np.float64))
    upd_terms = lr / (1 - b1 ** k) * m_terms / (np.sqrt(v_ref) / math.sqrt(1 - b2 ** k) + adam_eps)
    tols = adam_tolerances(before.flat, dev.grads, before.exp_avg, before.exp_avg_sq, upd, b1, b2,
                           rbias=bias_correction_rounding(b1, b2, k), floor=UNDERFLOW, upd_terms=upd_terms)
    carry = {}
    for name, got_a, ref_a, tol in (("exp_avg", after.exp_avg, m_ref, tols[0]), ("exp_avg_sq", after.exp_avg_sq, v_ref, tols[1]),
                                    ("params", after.flat, p_ref, tols[2])):
        ratio = np.abs(got_a.astype(np.float64) - ref_a) / tol
        ratio[np.isnan(ratio)] = np.inf                     # a NaN on the device is a miss, not a pass
        carry[name] = (float(ratio.max()), int(ratio.argmax()))
    figs = dict(step=k, mask_step=before.model_step + 1, lr=float(before.lr),
                total_rel=_rel(dev.total, t), kld_rel=_rel(dev.kld, kl), recon_err=abs(dev.recon - recon) / max(1.0, abs(recon)),
                grad_err=grad_err, worst=worst, **info,
                norm_rel=_rel(math.sqrt(dev.ss), norm), coef_rel=_rel(dev.coef, coef), coef=dev.coef, ss_own_rel=_rel(dev.ss, ss_own),
                exp_avg_tol=carry["exp_avg"][0], exp_avg_sq_tol=carry["exp_avg_sq"][0], params_tol=carry["params"][0],
                moved=float(np.abs(after.flat - before.flat).max()))
    if free is not None:
        figs["free_loss"] = free.step(feats, masks, before.lr)
        figs["free_gap"] = _rel(dev.total, figs["free_loss"])
    rt.record(tag, **figs)
    assert figs["total_rel"] < 1e-4 and figs["kld_rel"] < 1e-4 and figs["recon_err"] < 1e-4, (tag, "loss", figs)
    assert info["relu_flips"] <= max(4, 2e-5 * info["relu_units"]), (tag, info)
    assert grad_err < GRAD_BOUND, (tag, "gradient", worst, grad_err, info)
    assert figs["norm_rel"] < 1e-4 and figs["coef_rel"] < 1e-4, (tag, "norm / coefficient", figs)
    assert figs["ss_own_rel"] <= SS_SELF_RTOL, (tag, "sum of squares is not this gradient's", figs["ss_own_rel"])
    for name, (worst_ratio, at) in carry.items():
        assert worst_ratio <= 1.0, (tag, name, "entry", at, "|got - ref| / tolerance", worst_ratio)
    assert figs["moved"] > 0.1 * before.lr, (tag, "the step did not move the parameters", figs["moved"])
    assert after.opt_steps == before.opt_steps + 1 and after.model_step == before.model_step + 1 and after.seed == before.seed, \
        (tag, "counters", before[3:], after[3:])
    if before.host_seq is not None:
        assert after.host_seq == ((before.host_seq + 1) & 0xFFFFFF or 1), (tag, "host sequence", before.host_seq, after.host_seq)
    return figs


def check_skipped(tag, before, after):
    """A guard-skipped step (invalid batch, non-finite loss): parameters and moments bit for bit, Adam's step count unchanged."""
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        a, b = getattr(before, name), getattr(after, name)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, name, "moved in a skipped step")
    assert after.opt_steps == before.opt_steps and after.lr == before.lr and after.seed == before.seed, (tag, before[3:], after[3:])
