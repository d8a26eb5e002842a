"""The fused train step runs the loss head once (dvs_loss_forward_defer + dvs_loss_backward_emit) — on the host emulator,
against the two-kernel sequence (dvs_loss_forward + dvs_loss_backward_sq) from the same parameters, records and seeds."""
import ctypes

import numpy as np
import pytest
import torch

from dags_vae_search_amd import _lib as dl
from oracle import features as ofeat
from oracle import pace_oracle as po
from oracle.rng import DeviceMasks
from tests.emu.harness import EmuModel, ptr
from tests.loss_once_common import check_dag_losses, oracle_abs_terms

BETA = 0.005
SEED = 4242
DAG_OFFSET = 3


def _dag_losses(m):
    out = np.zeros((m.batch, 2), np.float32)
    dl.check(m.lib, m.lib.dvs_debug_dag_losses(ctypes.byref(m.shape), ptr(m.ws), ptr(out), None), "dag_losses")
    return out


def _aligned_words(n=4):
    buf = np.zeros(n + 4, np.float32)
    off = (-buf.ctypes.data % 16) // 4
    return buf[off:off + n]


def _old_sequence(m, eps):
    losses, mu, lv = m.forward(eps)
    dag = _dag_losses(m)
    scratch = np.zeros(dl.CLIP_SCRATCH_FLOATS, np.float32)
    _, flat = m.backward(1.0, BETA, clip_scratch=scratch)
    return dict(losses=losses, mu=mu, lv=lv, dag=dag, grads=flat, scratch=scratch)


def _new_sequence(m, eps, host_seq=77):
    mu = np.zeros((m.batch, 32), np.float32)
    lv = np.zeros((m.batch, 32), np.float32)
    e = None if eps is None else np.ascontiguousarray(eps, np.float32)
    args = (ctypes.byref(m.shape), ptr(m.records), m.records.nbytes, ptr(m.flat), m.flat.size, ptr(m.ws), m.ws.nbytes)
    dl.check(m.lib, m.lib.dvs_loss_forward_defer(*args, ptr(e), ptr(mu), ptr(lv), None), "forward_defer")
    kld_after_forward = _dag_losses(m)[:, 1].copy()
    losses = np.full(dl.LOSS_FLOATS, np.nan, np.float32)
    gcoef = np.asarray([1.0, BETA], np.float32)
    grads = np.full(m.P, np.nan, np.float32)
    scratch = np.zeros(dl.CLIP_SCRATCH_FLOATS, np.float32)
    tail = _aligned_words()
    m.status[0] = 0
    dl.check(m.lib, m.lib.dvs_loss_backward_emit(*args, ptr(gcoef), ptr(grads), ptr(scratch), ptr(m.status), ptr(losses),
                                                 ptr(tail), host_seq, None), "backward_emit")
    dag = _dag_losses(m)
    assert np.array_equal(dag[:, 1], kld_after_forward)               # the backward leaves the KL slots alone
    # the host packet: the same scalars, the sequence number in the upper 24 bits, no flag
    word = int(tail.view(np.uint32)[3])
    assert word >> 8 == host_seq and word & 0xFF == 0
    assert np.array_equal(tail[:3], losses[:3])
    return dict(losses=losses, mu=mu, lv=lv, dag=dag, grads=grads, scratch=scratch)


CASES = [  # n, card, B, dropout
    (2, 2, 1, 0.15),       # the smallest pair walk; three dead waves in the workgroup
    (12, 12, 5, 0.15),     # B no multiple of the 4 waves: the dead-wave branch next to live waves
    (13, 13, 4, 0.15),     # N = 16: a full tile, no padded token
    (12, 12, 9, 0.15),     # 2 workgroups x 4 waves on the emulator: a second round with one live wave
    (12, 12, 9, 0.0),
]


@pytest.mark.parametrize("n,card,B,dropout", CASES, ids=[f"n{n}c{c}-B{B}-p{p}" for n, c, B, p in CASES])
def test_emu_loss_once_equals_the_two_kernel_sequence(n, card, B, dropout):
    """Gradients (all 108 tensors), KL slots, mu, logvar: bit for bit.  Per-DAG reconstruction loss: within
    n_terms * 2^-24 * sum|terms| of k_loss_fwd's value (tests/loss_once_common.py), sum|terms| from the oracle's per-term
    losses: the pair logits come from the backward's recompute, whose inner sum is associated differently."""
    cfg = po.PaceConfig(n=n, card=card, dropout=dropout)
    params = po.init_params(cfg, seed=5)
    graphs = ofeat.synthetic_dags(n, card, B, seed=3, density_limit=0.4)
    f_np = ofeat.dense_features(graphs, card)
    pn = {k: v.numpy() for k, v in params.items()}
    if dropout > 0:
        masks = DeviceMasks(SEED, dropout, dag_offset=DAG_OFFSET)
        eps_dev, eps_ref = None, torch.from_numpy(masks.eps(B))          # counter-based noise on both sides
    else:
        masks = None
        eps_dev = (np.random.default_rng(11).standard_normal((B, 32)) * 0.01).astype(np.float32)
        eps_ref = torch.from_numpy(eps_dev)
    runs = []
    for seq in (_old_sequence, _new_sequence):
        m = EmuModel(cfg, pn, B, training=True, dropout=dropout, seed=SEED, dag_offset=DAG_OFFSET, beta=BETA)
        assert m.pack(f_np) == 0
        runs.append((m, seq(m, eps_dev)))
    (m, old), (_, new) = runs
    assert not np.isnan(old["grads"]).any()
    assert np.array_equal(old["grads"].view(np.uint32), new["grads"].view(np.uint32))
    for name, off, shp in m.table:                                      # all 108 tensors, by name
        k = int(np.prod(shp))
        assert np.array_equal(old["grads"][off:off + k].view(np.uint32), new["grads"][off:off + k].view(np.uint32)), name
    assert len(m.table) == 108
    assert np.array_equal(old["scratch"].view(np.uint32), new["scratch"].view(np.uint32))
    assert np.array_equal(old["mu"].view(np.uint32), new["mu"].view(np.uint32))
    assert np.array_equal(old["lv"].view(np.uint32), new["lv"].view(np.uint32))
    abs_terms, counts = oracle_abs_terms(cfg, params, f_np, True, eps=eps_ref, masks=masks)
    # the oracle evaluates the same model: its per-DAG loss is the device's to 1e-4
    assert np.abs(abs_terms - old["dag"][:, 0]).max() <= 1e-4 * abs_terms.max()
    bound = check_dag_losses(cfg, old["dag"], new["dag"], abs_terms, counts, f"emu n={n} B={B} p={dropout}")
    # the scalars: KL bit for bit; the reconstruction sum is k_finalize's fixed-order sum of the per-DAG values, so it moves by
    # at most the per-DAG differences plus one rounding per addend
    assert old["losses"][2] == new["losses"][2] and new["losses"][3] == 0.0 and new["losses"][4] == 0.0
    slack = float(bound.sum()) + B * 2.0 ** -24 * float(abs_terms.sum())
    assert abs(float(new["losses"][1]) - float(old["losses"][1])) <= slack
    assert abs(float(new["losses"][0]) - float(old["losses"][0])) <= slack + 2.0 ** -24 * abs(float(old["losses"][0]))


def test_emu_loss_once_refuses_the_wide_path_and_keeps_the_plain_backward():
    """Shapes of the wide path are refused by both new entry points before anything is enqueued; dvs_loss_backward_emit
    without `losses` is dvs_loss_backward_sq (the two-kernel sequence runs through it)."""
    gcoef = np.asarray([1.0, BETA], np.float32)
    losses = np.zeros(dl.LOSS_FLOATS, np.float32)

    def model(n, B):
        cfg = po.PaceConfig(n=n, card=n)
        params = po.init_params(cfg, seed=5)
        m = EmuModel(cfg, {k: v.numpy() for k, v in params.items()}, B, training=False)
        assert m.pack(ofeat.dense_features(ofeat.synthetic_dags(n, n, B, seed=3, density_limit=0.4), n)) == 0
        return m, (ctypes.byref(m.shape), ptr(m.records), m.records.nbytes, ptr(m.flat), m.flat.size, ptr(m.ws), m.ws.nbytes)

    m, args = model(14, 1)                                             # N = 17 tokens: two tiles
    grads = np.full(m.P, np.nan, np.float32)
    assert m.lib.dvs_loss_forward_defer(*args, None, None, None, None) == 13
    assert m.lib.dvs_loss_backward_emit(*args, ptr(gcoef), ptr(grads), None, None, ptr(losses), None, 0, None) == 13
    assert np.isnan(grads).all() and not losses.any()
    m, args = model(2, 2)
    grads = np.full(m.P, np.nan, np.float32)
    m.forward()
    assert m.lib.dvs_loss_backward_emit(*args, ptr(gcoef), ptr(grads), None, None, None, None, 0, None) == 0
    _, ref = m.backward(1.0, BETA)
    assert not np.isnan(ref).any() and np.array_equal(grads.view(np.uint32), ref.view(np.uint32))
