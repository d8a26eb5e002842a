"""Consecutive train steps on the device — PaceVaeV3 + optim.Adam(...).attach(model) + train_batch, where the state between
steps lives — with EVERY step checked as a transition against the float64 oracle, teacher-forced from the device's own
state before the step (tests/train_steps_common.py holds the reference, the checks and the tolerance derivations).

What is carried from one step to the next and pinned here: the per-step mask seed (seed << 32) | step of
PaceVaeV3._next_seed, the 1-based Adam step and its bias corrections, the flat moments, the lr handed down from the param
group, the weight images and saved activations rebuilt from parameters the previous step moved, the clip partials the
backward leaves in scratch[2..] for dvs_clip_adam_from_partials, the host notification's sequence number, and all of these
after a guard-skipped step and across a state_dict() resume.  No test resets model._seed / model._step inside its loop: the
mask stream moves only through what train_batch does itself.  The float64 OracleTrainer also runs freely from the start
with the same masks; its loss is recorded next to the device's (free_gap) and nothing is asserted on it.

Faults these checks were shown to catch.  Each was injected into a scratch copy, never committed, and this file
("device") and tests/test_emu_train_steps.py ("emulator") were run against it: on the device the fault sat in the Python
layer (PaceVaeV3, PaceEngine) unless marked "kernels", on the emulator always in the kernels / the C ABI, which is all an
emulator run goes through.  Every failure is at the first step the fault can touch; figures are that step's.

  fault                                          build     first failing check (figure against its bound)
  _next_seed returns the same step twice         device    2, the ReLU-side rule inside it: device and oracle disagree on
   (emulator: the kernels ignore the step word             a ReLU at 0.67 of the layer scale (bound 1e-4), every case, step 2.
   of the seed)                                  emulator  The same; with that rule switched off check 1 fails next:
                                                           total 7.8e-3 ... 2.4e-2, kld 0.11 ... 0.22 (bound 1e-4), gradient
                                                           0.77 ... 1.02 of the tensor maximum (bound 2e-4)
  optimiser passes step stuck at 1               both      4 parameters: 29 000 tolerances, every case, step 2
  moments zeroed before every step               both      4 exp_avg: 2.1e6 tolerances, every case, step 2
  backward without clip_scratch from the         both      3 norm and coefficient: norm off by 0.8 ... 3.0 relative (bound
   second step on (from_partials reads the                 1e-4), every case, step 2; checks 1 and 2 stay green (the gradient
   previous step's partials)                               is compared under the device's own coefficient)
  lr ignored after the first step                device    4 parameters: 4.4e5 tolerances at call 3 of the lr-cut case; the
                                                           other cases never change lr and pass, as does the emulator file
  wide path skips its weight-image rebuild on    device    2, the ReLU-side rule: 2.4e-2 of the layer scale at step 2 of
   the second forward (kernels)                  emulator  n14-B5 and n45-B3 (emulator n = 14: 1.6e-2); one-tile cases pass;
                                                           with that rule switched off check 1 fails next: total 5.0e-2,
                                                           kld 0.55, gradient 1.3
Without any fault the worst |got - ref| / tolerance of check 4 was 0.35 (exp_avg_sq), 0.24 (exp_avg), 0.21 (parameters) on the
device, the worst gradient error 5.9e-5, and the free-run loss gap at most 2.4e-7.
"""
import numpy as np
import pytest
import torch

from oracle import pace_oracle as po
from tests import train_steps_common as ts
from tests.gpu_common import default_waves, device_cus
from tests.test_gpu_module import build_model

pytestmark = pytest.mark.gpu
SEED = 7
LR = 1e-3


def _setup(n, B, monkeypatch, loss_once=True):
    from dags_vae_search_amd import optim as dopt
    from dags_vae_search_amd.synthetic import synthetic_dags
    monkeypatch.delenv("DVS_WAVES_PER_WG", raising=False)
    cfg = po.PaceConfig(n=n, card=n)
    params = po.init_params(cfg, seed=3)
    graphs = synthetic_dags(n, n, B, seed=42, density_limit=0.2 if n > 20 else 0.4)
    model = build_model(cfg, params, dropout=ts.DROPOUT).train()
    model._loss_once = loss_once
    model.seed(SEED)
    opt = dopt.Adam(model.parameters(), lr=LR).attach(model)
    f = model.prepare_features(graphs)
    f_cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}
    return cfg, params, model, opt, f, f_cpu


def _state(model, opt):
    """the device's state between two steps (train_steps_common.State)"""
    torch.cuda.synchronize()
    st = opt.state[opt.param_groups[0]["params"][0]]
    flat = model.flat_params.detach().cpu().numpy().copy()
    m, v = (st[k].detach().cpu().numpy().reshape(-1).copy() if k in st else np.zeros_like(flat) for k in ("exp_avg", "exp_avg_sq"))
    tail = getattr(model, "_host_tail", None)              # allocated with the gradient buffer, by the first step
    seq = 0 if tail is None else int(tail.numpy().view("uint32")[3]) >> 8
    return ts.State(flat, m, v, opt._steps, opt.param_groups[0]["lr"], model._seed, model._step, seq)


def _step(tag, cfg, model, opt, f, f_cpu, free):
    """one train_batch, checked as a transition"""
    from dags_vae_search_amd.train import train_batch
    before = _state(model, opt)
    loss, recon, kld = train_batch(f, model, opt, max_grad_norm=ts.MAX_NORM)
    after = _state(model, opt)
    dev = ts.DeviceStep(loss, float(recon), float(kld), model.flat_grads.detach().cpu().numpy().copy(),
                        float(opt._scratch[0]), float(opt._scratch[1]))
    return ts.check_transition(tag, cfg, model._engine.table, before, after, dev, f_cpu, model, free)


CASES = [  # n, B (C = compute units), steps, loss head run once, wide path, waves per workgroup
    pytest.param(12, lambda C: 9, 4, True, False, 4, id="n12-B9"),               # narrow mapping, loss-once pair, from_partials
    pytest.param(12, lambda C: 4 * C + 1, 3, True, False, 8, id="n12-B4C+1"),    # 8-wave mapping, ragged second pass
    pytest.param(12, lambda C: 9, 3, False, False, 4, id="n12-B9-two-kernel"),   # two-kernel loss head + notify
    pytest.param(14, lambda C: 5, 3, True, True, 8, id="n14-B5"),                # N = 17: smallest wide shape
    pytest.param(45, lambda C: 3, 2, True, True, 8, id="n45-B3"),                # N = C = 48: both maxima
]


@pytest.mark.parametrize("n,batch,steps,loss_once,wide,nw", CASES)
def test_consecutive_steps_match_oracle_transitions(n, batch, steps, loss_once, wide, nw, request, monkeypatch):
    B = batch(device_cus())
    cfg, params, model, opt, f, f_cpu = _setup(n, B, monkeypatch, loss_once)
    free = ts.FreeRun(cfg, params, LR)
    for k in range(1, steps + 1):
        _step(f"train_steps[{request.node.callspec.id}] step {k}", cfg, model, opt, f, f_cpu, free)
    assert model._engine.wide == wide and (wide or default_waves(B) == nw)       # the case ran on the path it names
    assert opt._steps == steps and model._step == steps and model._seed == SEED


def test_lr_cut_and_invalid_batch_in_the_middle_of_a_run(monkeypatch):
    """Five calls at n = 12, B = 9: the lr drops to a tenth after step 2 (what ReduceLROnPlateau does to the param group);
    call 4 is an invalid batch (label rows that are not one-hot): ValueError, parameters and moments bit for bit, Adam's step
    count unchanged; call 5 is a normal transition again, with the mask step read from the model and Adam step 4."""
    from dags_vae_search_amd.train import train_batch
    cfg, params, model, opt, f, f_cpu = _setup(12, 9, monkeypatch)
    free = ts.FreeRun(cfg, params, LR)
    tag = "train_steps[n12-B9-lr-cut-invalid]"
    for k in (1, 2):
        _step(f"{tag} call {k}", cfg, model, opt, f, f_cpu, free)
    opt.param_groups[0]["lr"] = LR / 10
    figs = _step(f"{tag} call 3", cfg, model, opt, f, f_cpu, free)
    assert figs["lr"] == LR / 10 and figs["moved"] < 0.5 * LR                     # the cut reached the kernel
    before = _state(model, opt)
    bad = dict(f)
    bad["vertex_label_features"] = f["vertex_label_features"] * 0.5
    with pytest.raises(ValueError, match="feature invariants"):
        train_batch(bad, model, opt, max_grad_norm=ts.MAX_NORM)
    after = _state(model, opt)
    ts.check_skipped(f"{tag} call 4", before, after)
    assert opt._steps == 3
    figs = _step(f"{tag} call 5", cfg, model, opt, f, f_cpu, free)
    assert figs["step"] == 4 and figs["mask_step"] == after.model_step + 1 and opt._steps == 4


def test_resume_from_state_dicts_continues_the_transitions(monkeypatch):
    """Two steps, then state_dict() of model and optimiser into a fresh pair: steps 3 and 4 on the fresh pair are transitions
    against the oracle like any other (moments, Adam step 3 and the lr come from the loaded state), and end bit for bit where
    the uninterrupted run ends.  The mask counter is not part of a state dict: the fresh model is handed it once, before its
    first step."""
    from dags_vae_search_amd import optim as dopt
    from dags_vae_search_amd.train import train_batch
    cfg, params, a, oa, f, f_cpu = _setup(12, 9, monkeypatch)
    free = ts.FreeRun(cfg, params, LR)
    tag = "train_steps[n12-B9-resume]"
    for k in (1, 2):
        _step(f"{tag} step {k}", cfg, a, oa, f, f_cpu, free)
    sd_model = {k: v.detach().cpu().clone() for k, v in a.state_dict().items()}
    sd_opt = oa.state_dict()
    sd_opt = {"state": {k: {kk: (vv.cpu().clone() if torch.is_tensor(vv) else vv) for kk, vv in v.items()}
                        for k, v in sd_opt["state"].items()}, "param_groups": sd_opt["param_groups"]}     # as torch.save / load
    b = build_model(cfg, sd_model, dropout=ts.DROPOUT).train()
    ob = dopt.Adam(b.parameters(), lr=123.0).attach(b)          # the lr must come from the loaded state
    ob.load_state_dict(sd_opt)
    b._seed, b._step = a._seed, a._step
    for k in (3, 4):
        figs = _step(f"{tag} step {k} (fresh pair)", cfg, b, ob, f, f_cpu, free)
        assert figs["step"] == k and figs["mask_step"] == k and figs["lr"] == LR
        train_batch(f, a, oa, max_grad_norm=ts.MAX_NORM)
    torch.cuda.synchronize()
    assert ob._steps == oa._steps == 4 and torch.equal(a.flat_params, b.flat_params)
