"""TEST INFRASTRUCTURE: gradient parity on the same linear piece of the network.

PACE-VAE is piecewise linear in its hidden layers (6 FFN ReLUs, the add_node / add_edge heads).  Device and CPU oracle
agree on every hidden pre-activation to ~1e-6, so a unit whose pre-activation is within that distance of zero can land on
different sides of the ReLU — and one such unit moves a weight gradient by a whole token's contribution (1e-3..1e-2 of the
tensor maximum on a 24-DAG batch), although both evaluations are correct to rounding.  A max-norm bound loose enough to
survive that (round 1: 3e-3, exceeded once at 3.013e-3) cannot see real regressions.  So:

  1. the oracle runs with a hook that records every hidden pre-activation (oracle/pace_oracle.py `_relu`);
  2. the device's side of each ReLU is re-derived in float64 from the device's OWN saved input of that layer
     (dvs_debug_activation: the pre-LayerNorm sum the FFN / loss head consumed);
  3. units where the two disagree are counted, and each must be a genuine tie (|pre| <= `tie` of the layer's scale) —
     a disagreement at a large pre-activation is a bug, not rounding;
  4. if there are any, the oracle is re-evaluated ON THE DEVICE'S PIECE (pre * device mask instead of relu) and the
     gradient bound (2e-4 of the tensor maximum) is asserted against that; with no disagreement it is asserted directly;
  5. large batches (test_gpu_mapping_parity.py) run the oracle in float64 and, where the bound is missed, also try both
     sides of the few units within float32 resolution of their kink (sub_resolution_units / best_tie_sides): step 2
     cannot see which side the device's own rounding chose there.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import pace_oracle as po

REPORT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "parity_report.json")
_report = {}


def record(test, **vals):
    """Measured parity figures of a GPU test (printed, and kept in gpurun_out/parity_report.json for profiles/)."""
    _report[test] = vals
    print(f"[parity] {test}: " + ", ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in vals.items()))
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        old = {}
        if os.path.exists(REPORT):
            with open(REPORT) as fh:
                old = json.load(fh)
        old.update(_report)
        with open(REPORT, "w") as fh:
            json.dump(old, fh, indent=1, sort_keys=True)
    except OSError:
        pass


class ReluTrace:
    def __init__(self, override=None):
        self.pre, self.aux, self.override = {}, {}, override or {}

    def __call__(self, name, pre):
        self.pre[name] = pre.detach()
        m = self.override.get(name)
        return torch.relu(pre) if m is None else pre * m.to(pre.dtype)


def device_relu_masks(model, params, cfg, B, pairs):
    """{hidden layer: bool mask} as the device sees each ReLU, from its saved activations (valid after a forward)."""
    eng = model._engine
    N = cfg.N
    P = {k: v.detach().double().cpu() for k, v in params.items()}

    def layer_input(slot, norm):
        pre = eng.activation(B, slot)[:, :N].double().cpu()                       # [B, N, 64] pre-LayerNorm sum
        return F.layer_norm(pre, (64,), P[norm + ".weight"], P[norm + ".bias"], 1e-5)
    out = {}
    for l in range(cfg.layers):
        x = layer_input(1 + 2 * l, f"encoder.layers.{l}.norm1")
        out[f"encoder.layers.{l}.linear1"] = (F.linear(x, P[f"encoder.layers.{l}.linear1.weight"],
                                                       P[f"encoder.layers.{l}.linear1.bias"]) > 0).transpose(0, 1)
        x = layer_input(8 + 3 * l + 1, f"decoder.layers.{l}.norm2")
        out[f"decoder.layers.{l}.linear1"] = (F.linear(x, P[f"decoder.layers.{l}.linear1.weight"],
                                                       P[f"decoder.layers.{l}.linear1.bias"]) > 0).transpose(0, 1)
    dec = layer_input(8 + 3 * (cfg.layers - 1) + 2, f"decoder.layers.{cfg.layers - 1}.norm3")
    out["add_node.0"] = F.linear(dec, P["add_node.0.weight"], P["add_node.0.bias"]) > 0
    b, i, j = pairs
    pair = torch.cat([dec[b, i], dec[b, j]], dim=1)
    out["add_edge.0"] = F.linear(pair, P["add_edge.0.weight"], P["add_edge.0.bias"]) > 0
    return out


def grad_errors(got, ref):
    """per-tensor |got - ref|_max / max(|ref|_max, 1e-4 * global scale); returns (worst, its name, dict)."""
    scale = max(float(v.abs().max()) for v in ref.values())
    errs = {}
    for k, r in ref.items():
        g = got[k].detach().cpu().double()
        errs[k] = float((g - r.double()).abs().max()) / max(float(r.abs().max()), 1e-4 * scale)
    worst = max(errs, key=errs.get)
    return errs[worst], worst, errs


def as_dtype(params, feats, eps=None, dtype=None):
    """params, the floating-point feature tensors and eps cast to `dtype` (None: unchanged) — the oracle runs in float64 when
    given float64 inputs (a float32 oracle is too coarse for batches of thousands of DAGs: its sums round at ~1e-4)."""
    if dtype is None:
        return params, feats, eps
    P = {k: v.to(dtype) for k, v in params.items()}
    F_ = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in feats.items()}
    return P, F_, None if eps is None else eps.to(dtype)


def run_oracle(params, cfg, feats_cpu, training, eps=None, masks=None, hook=None):
    """oracle forward + backward -> (total, kld, {name: grad})."""
    P = {k: v.detach().clone().requires_grad_(True) for k, v in params.items()}
    t, r, k = po.loss_direct(P, cfg, feats_cpu, training=training, eps=eps, masks=masks, relu=hook)
    t.backward()
    return t.detach(), k.detach(), {n: p.grad for n, p in P.items()}


def relu_flips(trace, dev, tie=1e-4):
    """count the units where the device's ReLU side (`dev`, device_relu_masks) differs from the oracle's (`trace`); each
    must be a genuine tie (|pre| <= `tie` of the layer's scale)."""
    flips, units, worst_tie = 0, 0, 0.0
    for name, pre in trace.pre.items():
        d = dev[name] != (pre > 0)
        units += pre.numel()
        n = int(d.sum())
        if n:
            flips += n
            rel = float(pre.abs()[d].max()) / float(pre.abs().max())
            worst_tie = max(worst_tie, rel)
            assert rel <= tie, f"{name}: device and oracle disagree on a ReLU at |pre| = {rel:.2e} of the layer scale"
    return {"relu_units": units, "relu_flips": flips, "worst_tie": worst_tie}


def oracle_on_device_piece(model, params, cfg, feats_cpu, B, training, eps=None, masks=None, tie=1e-4, dtype=None):
    """Run the oracle; count ReLU disagreements with the device (model must have just run its forward on the same batch);
    if any, re-run the oracle on the device's piece.  `dtype` (e.g. torch.float64) casts params, the floating-point
    features and eps (and, through ReluTrace, the override masks); None keeps the inputs' own.  Returns (total, kld, grads
    on the device's piece, grads of the plain oracle, info dict)."""
    P, feats, eps = as_dtype(params, feats_cpu, eps, dtype)
    tr = ReluTrace()
    t0, k0, g0 = run_oracle(P, cfg, feats, training, eps, masks, tr)
    dev = device_relu_masks(model, params, cfg, B, tr.aux["pairs"])
    info = relu_flips(tr, dev, tie)
    if info["relu_flips"] == 0:
        return t0, k0, g0, g0, info
    t1, k1, g1 = run_oracle(P, cfg, feats, training, eps, masks, ReluTrace(override=dev))
    return t1, k1, g1, g0, info


def sub_resolution_units(trace, floor=1e-7, cap=8):
    """The `cap` hidden units closest to their ReLU's kink, among those within `floor` of the layer scale.  There, float32
    rounding of the device's own evaluation decides the side, and device_relu_masks (a float64 re-derivation from the
    device's saved layer input) cannot tell which side it took: at batches of thousands of DAGs a few such units exist in
    every run (e.g. |pre| = 6e-9 of the scale), and one of them moves a linear1 gradient by up to ~5e-4 of its maximum."""
    units = []
    for name, pre in trace.pre.items():
        r = pre.abs() / pre.abs().max()
        units += [(float(r[tuple(i)]), name, tuple(i)) for i in (r < floor).nonzero().tolist()]
    return sorted(units)[:cap]


def best_tie_sides(got, ref, flipped):
    """Gradient error of `got` against the oracle `ref` on the best choice of sides for sub-resolution units: `flipped` holds
    one oracle gradient dict per unit, evaluated with only that unit's side flipped.  The forward pass does not move
    (those pre-activations are ~0), so flips add up; every subset is tried.  Returns (error, worst tensor, subset size)."""
    deltas = [{k: g[k] - ref[k] for k in ref} for g in flipped]
    best = None
    for mask in range(1 << len(deltas)):
        cand = {k: v.clone() for k, v in ref.items()}
        for u, d in enumerate(deltas):
            if mask >> u & 1:
                for k in cand:
                    cand[k] += d[k]
        err, worst, _ = grad_errors(got, cand)
        if best is None or err < best[0]:
            best = (err, worst, bin(mask).count("1"))
    return best
