"""Per-tensor parity of the persistent mappings past their first pass.

Every persistent grid is capped at dvs_device_cus() = C workgroups (dvs_api.hip: grid_for, active_slabs), so a batch above
C x (DAGs per workgroup and pass) makes each workgroup loop over a second, third, ... group of DAGs.  The one-tile stack
kernels own 4 DAGs per workgroup and pass below 4C DAGs (narrow mapping) and 8 above (dvs_api.hip: waves_per_wg); the wide
path's workgroup-per-DAG kernels own one.  The batch sizes below are chosen by the pass boundary they hit, with C taken from
the loaded library.  Sums (ELBO, gradient norms, shard additivity) cannot see a fault confined to one small tensor or to a
few DAGs, so here: all 108 gradients against a float64 oracle on the device's linear piece (tests/relu_trace.py), per-DAG
latents row by row, bitwise position invariance of a DAG's latents, and decode past one pass."""
import numpy as np
import pytest
import torch

from oracle import pace_oracle as po
from oracle.rng import DeviceMasks
from tests.gpu_common import default_waves, device_cus
from tests.helpers import load_golden, rel
from tests.relu_trace import (ReluTrace, as_dtype, best_tie_sides, device_relu_masks, grad_errors, record, relu_flips,
                              run_oracle, sub_resolution_units)
from tests.test_gpu_module import GRAD_BOUND, build_model, feats_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def _synthetic(n, card, B, seed):
    from dags_vae_search_amd.synthetic import synthetic_dags
    return synthetic_dags(n, card, B, seed=seed, density_limit=0.2 if n > 20 else 0.4)


def _bench_model_and_graphs(B):
    """bench.py's own weights (torch.manual_seed(42) + the PaceVaeV3 constructor) and inputs (seed 42, density 0.4)."""
    from dags_vae_search_amd import PaceVaeV3
    from dags_vae_search_amd.synthetic import synthetic_dags
    torch.manual_seed(42)
    model = PaceVaeV3(max_num_vertices=12, vertex_label_cardinality=12, vertices_embedding_size=32, num_heads=8,
                      num_layers=3, ff_hidden_size=64, latent_layer_size=32, fc_hidden=32, dropout=0.15)
    params = {k: v.detach().clone() for k, v in model.state_dict().items()}
    return model.to(DEV), params, synthetic_dags(12, 12, B, seed=42, density_limit=0.4)


def _device_step(model, params, cfg, f, seed, B, pairs):
    """one train-mode forward + backward on the device (dropout 0.15, step 1 of `seed`) -> losses, gradients, and the
    device's side of every hidden ReLU (read from its saved activations right after this forward)."""
    model.train()
    model.zero_grad(set_to_none=True)
    model.seed(seed)
    model.dag_offset = 0
    total, recon, kld = model.loss_direct(f)
    total.backward()
    grads = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
    masks = device_relu_masks(model, params, cfg, B, pairs)
    model.zero_grad(set_to_none=True)
    return total.item(), kld.item(), grads, masks


def mapping_parity(tag, monkeypatch, model, params, cfg, graphs, seed, widths=(None,)):
    """Train mode, dropout 0.15 with the device's own masks, at each workgroup width in `widths` (None: the batch's own):
    ELBO and KLD within 1e-4 relative of a FLOAT64 oracle, all 108 gradients within GRAD_BOUND of each tensor's maximum on
    the device's linear piece, and the ReLU-flip rule of test_gpu_module.dropout_on_parity.  One oracle run serves every
    width whose ReLU piece agrees with it (or with an earlier width's piece).  Where the gradients miss the bound, units
    within float32 resolution of their kink get both sides tried (relu_trace.sub_resolution_units); the bound then holds
    for the best choice, and the units flipped count as ReLU flips."""
    B = len(graphs)
    f = feats_for(model, graphs)
    f_cpu = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}
    masks = DeviceMasks((seed << 32) | 1, 0.15)                 # PaceVaeV3._next_seed: (seed << 32) | step
    P, feats, eps = as_dtype(params, f_cpu, torch.from_numpy(masks.eps(B)), F64)
    trace = ReluTrace()
    plain = run_oracle(P, cfg, feats, True, eps, masks, trace)
    pieces = []                                                  # [(device ReLU masks, oracle result on that piece)]
    for nw in widths:
        if nw is None:
            monkeypatch.delenv("DVS_WAVES_PER_WG", raising=False)
            nw = 8 if cfg.N > 16 or cfg.C > 16 else default_waves(B)
        else:
            monkeypatch.setenv("DVS_WAVES_PER_WG", str(nw))
        total, kld, got, dev = _device_step(model, params, cfg, f, seed, B, trace.aux["pairs"])
        info = relu_flips(trace, dev)
        ref, on_piece = plain, False
        if info["relu_flips"]:
            on_piece = True
            ref = next((r for d, r in pieces if all(torch.equal(d[k], dev[k]) for k in dev)), None)
            if ref is None:
                ref = run_oracle(P, cfg, feats, True, eps, masks, ReluTrace(override=dev))
                pieces.append((dev, ref))
        t, k, g_ref = ref
        err, worst, _ = grad_errors(got, g_ref)
        err_plain, worst_plain, _ = grad_errors(got, plain[2])
        extra = {}
        if err >= GRAD_BOUND:
            # units within float32 resolution of their kink: which side the device took is not observable, so the
            # oracle is evaluated with each one flipped and the best choice of sides is bounded instead
            units = sub_resolution_units(trace)
            flipped = []
            for _, name, i in units:
                side = {n: m.clone() for n, m in dev.items()}
                side[name][i] = ~side[name][i]
                flipped.append(run_oracle(P, cfg, feats, True, eps, masks, ReluTrace(override=side))[2])
            err_direct = err
            err, worst, n_sides = best_tie_sides(got, g_ref, flipped)
            info["relu_flips"] += n_sides
            extra = dict(grad_err_before_tie_sides=err_direct, tie_sides_flipped=n_sides,
                         tie_sides_tried=len(units), smallest_tie=units[0][0] if units else None)
        record(f"{tag},B={B},nw={nw}", elbo_rel=rel(total, t), kld_rel=rel(kld, k), grad_err=err, worst=worst,
               grad_err_plain_oracle=err_plain, worst_plain=worst_plain, device_piece=on_piece, **info, **extra)
        assert rel(total, t) < 1e-4 and rel(kld, k) < 1e-4, (nw, total, float(t), kld, float(k))
        assert info["relu_flips"] <= max(4, 2e-5 * info["relu_units"]), (nw, info)
        assert err < GRAD_BOUND, (nw, worst, err, info, extra)
    monkeypatch.delenv("DVS_WAVES_PER_WG", raising=False)


@pytest.mark.parametrize("mult,extra", [(4, 0), (4, 1), (8, 1)], ids=["B=4C", "B=4C+1", "B=8C+1"])
def test_one_tile_pass_boundaries(mult, extra, monkeypatch):
    """4C: the largest narrow batch, one full pass; 4C + 1: the switch to 8 waves with a ragged last group; 8C + 1: the
    8-wave mapping's second pass holds a single DAG."""
    B = mult * device_cus() + extra
    cfg = po.PaceConfig(n=12, card=12)
    params = po.init_params(cfg, seed=3)
    model = build_model(cfg, params)
    mapping_parity(f"mapping[n12,{mult}C+{extra}]", monkeypatch, model, params, cfg, _synthetic(12, 12, B, 42), 1)


def test_benchmark_batch_both_widths(monkeypatch):
    """The benchmark's own shape, weights and inputs (16C = 4 096 DAGs on an MI355X): the 8-wave mapping it runs (two
    passes) and the forced narrow one (four passes)."""
    B = 16 * device_cus()
    model, params, graphs = _bench_model_and_graphs(B)
    cfg = po.PaceConfig(n=12, card=12)
    mapping_parity("mapping[bench n12,16C]", monkeypatch, model, params, cfg, graphs, 42, widths=(None, 4))


def test_batch_8192_n11_gradients(monkeypatch):
    """BASELINE config 4's per-GPU shape (sachs n = 11, 8 192 DAGs): four passes of the 8-wave mapping on an MI355X; all
    gradients (test_gpu_module.test_batch_8192_per_gpu_shapes checks its loss only)."""
    cfg = po.PaceConfig(n=11, card=11)
    params = po.init_params(cfg, seed=11)
    model = build_model(cfg, params)
    mapping_parity("mapping[n11]", monkeypatch, model, params, cfg, _synthetic(11, 11, 8192, 111), 4)


@pytest.mark.parametrize("n,mult,extra", [(37, 1, 1), (37, 2, 3), (45, 1, 1)], ids=["n37-B=C+1", "n37-B=2C+3", "n45-B=C+1"])
def test_wide_path_second_and_third_dag_per_workgroup(n, mult, extra, monkeypatch):
    """Wide path (N > 16 tokens): its workgroup-per-DAG kernels run a second DAG at C + 1 and a third at 2C + 3; n = 45
    (N = 48 tokens, C = 48 classes) is the maximum of both."""
    B = mult * device_cus() + extra
    cfg = po.PaceConfig(n=n, card=n)
    params = po.init_params(cfg, seed=8)
    model = build_model(cfg, params)
    mapping_parity(f"mapping[n{n},{mult}C+{extra}]", monkeypatch, model, params, cfg, _synthetic(n, n, B, 31), 9)


def test_per_dag_latents_at_benchmark_batch(monkeypatch):
    """Eval encode_direct of the benchmark batch (16C DAGs) at both widths against the float64 oracle ROW BY ROW: a fault
    that swaps or drops a few DAGs of a later pass moves the summed ELBO by ~1/B, far inside its bound, but not here."""
    B = 16 * device_cus()
    model, params, graphs = _bench_model_and_graphs(B)
    model.eval()
    cfg = po.PaceConfig(n=12, card=12)
    f = feats_for(model, graphs)
    P, feats, _ = as_dtype(params, {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in f.items()}, None, F64)
    with torch.no_grad():
        ref = po.encode_direct(P, cfg, feats)
    for nw in (8, 4):
        monkeypatch.setenv("DVS_WAVES_PER_WG", str(nw))
        got = [t.cpu().double() for t in model.encode_direct(f)]
        errs = {}
        for name, g, r in zip(("mu", "logvar"), got, ref):
            row = (g - r).abs().amax(dim=1) / float(r.abs().max())
            errs[name] = float(row.max())
            errs[name + "_worst_row"] = int(row.argmax())
        record(f"per_dag_latents[bench n12,B={B},nw={nw}]", **errs)
        assert errs["mu"] < 2e-4 and errs["logvar"] < 2e-4, (nw, errs)


@pytest.mark.parametrize("nw", [4, 8])
def test_latents_do_not_depend_on_batch_position(nw, monkeypatch):
    """The 48 golden n12c12 DAGs at the start of a 16C + 5 batch, at index 8C (first DAG of the 8-wave mapping's second
    pass, of the narrow mapping's third) and at the tail: their eval mu / logvar are BITWISE those of a 48-DAG call at the
    same width (per-DAG values do not depend on the mapping: test_gpu_stack.py)."""
    monkeypatch.setenv("DVS_WAVES_PER_WG", str(nw))
    cfg, params, golden, z = load_golden("n12c12")
    model = build_model(cfg, params).eval()
    C = device_cus()
    B = 16 * C + 5
    G = len(golden)
    filler = _synthetic(12, 12, B - 3 * G, 5)
    starts = [0, 8 * C, B - G]
    graphs = golden + filler[:8 * C - G] + golden + filler[8 * C - G:] + golden
    assert len(graphs) == B and all(graphs[s:s + G] == golden for s in starts)
    mu0, lv0 = model.encode_direct(feats_for(model, golden))
    mu, lv = model.encode_direct(feats_for(model, graphs))
    for s in starts:
        assert torch.equal(mu[s:s + G], mu0) and torch.equal(lv[s:s + G], lv0), (nw, s)
    record(f"position_invariance[n12c12,B={B},nw={nw}]", starts=str(starts), bitwise=True)


def test_decode_past_one_pass_equals_48_row_call():
    """k_decode runs 4 DAGs per workgroup and pass: the 48 golden eval/mu rows and their injected uniforms tiled to 4C + 5
    rows decode to exactly the graphs of the 48-row call (pinned to oracle/decode.py by
    test_gpu_decode.test_decode_with_injected_uniforms_equals_oracle) in every row."""
    cfg, params, graphs, z = load_golden("n12c12")
    model = build_model(cfg, params).eval()
    mu = torch.from_numpy(z["eval/mu"].copy())
    G = mu.shape[0]
    U = torch.from_numpy(np.random.default_rng(11).random((G, cfg.N, cfg.N)).astype(np.float32))
    base = model.decode(mu, uniforms=U, strict=False)
    B = 4 * device_cus() + 5
    idx = torch.arange(B) % G
    out = model.decode(mu[idx], uniforms=U[idx], strict=False)
    assert len(out) == B
    for row, g in enumerate(out):
        r = base[row % G]
        if r is None:
            assert g is None, row
        else:
            assert g is not None and g.labels == r.labels and sorted(g.edges) == sorted(r.edges), row
    record(f"decode_tiled[n12c12,B={B}]", rows=B, full_graphs=sum(g is not None for g in out))
