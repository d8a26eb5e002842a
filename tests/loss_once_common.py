"""Shared by tests/test_emu_loss_once.py and tests/test_gpu_loss_once.py: the oracle's per-term reconstruction losses and the
bound they give for a per-DAG loss whose fp32 sum is associated differently.

The fused train step lets the loss-head backward write the per-DAG reconstruction loss (include/dvs.h:
dvs_loss_forward_defer / dvs_loss_backward_emit).  That value is a sum of n_terms = (N-1) node terms + (N-1)(N-2)/2 pair
terms, all non-negative; the worst-case difference between two fp32 evaluations of such a sum in different orders is
n_terms * 2^-24 * sum|terms| (every one of at most n_terms roundings is relative 2^-24 of a partial sum that never exceeds
sum|terms|)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import features as ofeat
from oracle import pace_oracle as po

U = 2.0 ** -24


def n_terms(N: int) -> int:
    return (N - 1) + (N - 1) * (N - 2) // 2


def oracle_abs_terms(cfg, params, f_np, training, eps=None, masks=None):
    """sum|terms| of the reconstruction loss per DAG, float64 [B], from the oracle's decoder output: the node terms
    -log_softmax(add_node(h))[i, label_{i+1}] for i < N-1 and the BCE-with-logits terms of the pairs j < i <= N-2
    (oracle/pace_oracle.py: log_likelihood, term by term instead of summed).  Also returns the term count per DAG."""
    ft = ofeat.to_torch(f_np)
    with torch.no_grad():
        _, recon, _, aux = po.loss_direct(params, cfg, ft, training=training, eps=eps, masks=masks, return_aux=True)
        dec = aux["decoder_output"]
        B, N = dec.shape[0], cfg.N
        h = torch.relu(F.linear(dec, params["add_node.0.weight"], params["add_node.0.bias"]))
        logp = torch.log_softmax(F.linear(h, params["add_node.2.weight"], params["add_node.2.bias"]), dim=2)
        tgt = torch.zeros(B, N, dtype=torch.long)
        vl = torch.tensor([list(v)[:N] for v in ft["vertex_labels"]], dtype=torch.long)
        tgt[:, :vl.shape[1]] = vl
        sizes = torch.tensor(ft["num_vertices"])
        valid = torch.arange(N).expand(B, N) < (sizes - 1).unsqueeze(1)
        node = -torch.gather(logp, 2, tgt.unsqueeze(2)).squeeze(2) * valid
        total = node.abs().double().sum(1)
        count = valid.sum(1)
        adj = ft["adjacency_matrices"]
        w1, b1 = params["add_edge.0.weight"], params["add_edge.0.bias"]
        w2, b2 = params["add_edge.2.weight"], params["add_edge.2.bias"]
        for b in range(B):
            m = int(sizes[b]) - 1
            ii, jj = torch.meshgrid(torch.arange(m), torch.arange(m), indexing="ij")
            keep = ii > jj
            i_idx, j_idx = ii[keep], jj[keep]
            pair = torch.cat([dec[b, i_idx], dec[b, j_idx]], dim=1)
            logit = F.linear(torch.relu(F.linear(pair, w1, b1)), w2, b2)
            truth = adj[b, j_idx + 1, i_idx + 1].view(-1, 1)
            bce = F.binary_cross_entropy_with_logits(logit, truth, reduction="none")
            total[b] += bce.abs().double().sum()
            count[b] += bce.numel()
        # the term-by-term evaluation is the oracle's own loss
        assert abs(float(total.sum()) - float(recon)) <= 1e-4 * abs(float(recon))
    return total.numpy(), count.numpy()


def per_dag_bound(cfg, abs_terms, counts):
    """n_terms * 2^-24 * sum|terms| per DAG; every DAG of these batches has all N tokens."""
    nt = n_terms(cfg.N)
    assert (np.asarray(counts) == nt).all(), (counts, nt)
    return nt * U * np.asarray(abs_terms, np.float64)


def check_dag_losses(cfg, old, new, abs_terms, counts, label=""):
    """old / new: [B][2] per-DAG {reconstruction loss, KL term} of the two-kernel sequence (k_loss_fwd's value: the reference
    of this comparison) and of the run-once sequence.  Reconstruction within the reordering bound, KL bit for bit."""
    old = np.asarray(old, np.float32)
    new = np.asarray(new, np.float32)
    bound = per_dag_bound(cfg, abs_terms, counts)
    diff = np.abs(new[:, 0].astype(np.float64) - old[:, 0].astype(np.float64))
    worst = int(np.argmax(diff / bound))
    print(f"loss_once {label}: per-DAG recon |new - old| max {diff.max():.3e}, worst ratio to bound "
          f"{diff[worst] / bound[worst]:.3f} (DAG {worst}: {diff[worst]:.3e} vs {bound[worst]:.3e})")
    assert np.isfinite(new).all()
    assert (diff <= bound).all(), (label, worst, diff[worst], bound[worst])
    assert np.array_equal(old[:, 1].view(np.uint32), new[:, 1].view(np.uint32)), label
    return bound
