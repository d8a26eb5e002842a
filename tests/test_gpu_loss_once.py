"""The fused train step runs the loss head once (dvs_loss_forward_defer + dvs_loss_backward_emit) — on the device, against the
two-kernel sequence (PaceVaeV3._loss_once = False) from the same parameters, batch and seeds: one train_batch each."""
import numpy as np
import pytest
import torch

from oracle.rng import DeviceMasks
from tests.gpu_common import default_waves
from tests.helpers import load_golden
from tests.loss_once_common import check_dag_losses, n_terms, oracle_abs_terms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 3


def _one_step(cfg, params, graphs, loss_once):
    from dags_vae_search_amd import PaceVaeV3, optim as dopt
    from dags_vae_search_amd.train import train_batch
    model = PaceVaeV3(max_num_vertices=cfg.n, vertex_label_cardinality=cfg.card, vertices_embedding_size=32, num_heads=8,
                      num_layers=3, ff_hidden_size=64, latent_layer_size=32, fc_hidden=32, dropout=0.15)
    model.load_state_dict(params)
    model = model.to(DEV).train()
    model._loss_once = loss_once
    model.seed(SEED)
    opt = dopt.Adam(model.parameters(), lr=1e-4).attach(model)
    f = model.prepare_features(graphs)
    params0 = model.flat_params.detach().cpu().numpy().copy()
    loss_value, recon, kld = train_batch(f, model, opt)
    torch.cuda.synchronize()
    host = model._host_tail[:3].clone()
    assert loss_value == float(host[0]) and float(recon) == float(host[1]) and float(kld) == float(host[2])
    return dict(params0=params0, scalars=np.asarray([loss_value, float(recon), float(kld)], np.float64),
                params=model.flat_params.detach().cpu().numpy().copy(), grads=model.flat_grads.detach().cpu().numpy().copy(),
                dag=model._eng().dag_losses(len(graphs)).cpu().numpy(), f_cpu={k: (v.cpu() if torch.is_tensor(v) else v)
                                                                             for k, v in f.items()})


@pytest.mark.parametrize("B,waves", [(9, 4), (1030, 8)], ids=["B9-nw4", "B1030-nw8"])
def test_loss_once_train_step_equals_the_two_kernel_sequence(B, waves):
    """n = 12: B = 9 on the narrow 4-wave mapping; B = 1030 (> 4 x #CU) on the 8-wave mapping with a last partial round of
    the loss-head backward.  Parameters after one fused Adam step and the (clipped) gradient: bit for bit.  Per-DAG
    reconstruction loss within n_terms * 2^-24 * sum|terms| of k_loss_fwd's (sum|terms| from the oracle under the device's
    masks), KL bit for bit; train_batch's (loss, recon, kld): kld equal, loss / recon within the per-DAG bounds summed plus
    one rounding per addend of k_finalize's fixed-order sum."""
    from dags_vae_search_amd.synthetic import synthetic_dags
    cfg, params, _, _ = load_golden("n12c12")
    assert default_waves(B) == waves
    graphs = synthetic_dags(12, 12, B, seed=17, density_limit=0.4)
    old = _one_step(cfg, params, graphs, False)
    new = _one_step(cfg, params, graphs, True)
    assert np.isfinite(old["grads"]).all() and np.abs(old["grads"]).max() > 0
    assert np.array_equal(old["grads"].view(np.uint32), new["grads"].view(np.uint32))
    assert np.array_equal(old["params"].view(np.uint32), new["params"].view(np.uint32))
    assert np.array_equal(old["params0"], new["params0"]) and not np.array_equal(old["params"], old["params0"])     # it moved them
    masks = DeviceMasks((SEED << 32) | 1, 0.15)                      # PaceVaeV3._next_seed: (seed << 32) | step
    abs_terms, counts = oracle_abs_terms(cfg, params, old["f_cpu"], True, eps=torch.from_numpy(masks.eps(B)), masks=masks)
    assert np.abs(abs_terms - old["dag"][:, 0]).max() <= 1e-4 * abs_terms.max()
    bound = check_dag_losses(cfg, old["dag"], new["dag"], abs_terms, counts, f"gpu n=12 B={B}")
    assert counts[0] == n_terms(cfg.N)
    slack = float(bound.sum()) + B * 2.0 ** -24 * float(abs_terms.sum())
    d = np.abs(new["scalars"] - old["scalars"])
    print(f"loss_once gpu B={B}: train_batch |new - old| = loss {d[0]:.3e}, recon {d[1]:.3e}, kld {d[2]:.3e}; bound {slack:.3e}")
    assert d[2] == 0.0
    assert d[1] <= slack and d[0] <= slack + 2.0 ** -24 * abs(old["scalars"][0])

