"""Consecutive train steps through the C ABI on the host emulator, every step checked as a transition against the float64
oracle (tests/train_steps_common.py).  The emulator pins the kernels' half of what lives between steps: the weight images
and saved activations rebuilt from parameters the previous step moved, `step` in the bias corrections, the moments, and the
freshness of the clip partials in scratch[2..].  The Python half (PaceVaeV3._next_seed, optim.Adam) is pinned by
tests/test_gpu_train_steps.py, which also lists the faults these checks were shown to catch, on this build as well."""
import numpy as np
import pytest

from oracle import features as ofeat
from oracle import pace_oracle as po
from tests import train_steps_common as ts
from tests.emu.harness import EmuModel

SEED = 7
DAG_OFFSET = 3
LR = 1e-3


def _state(m, opt_steps, host_seq):
    return ts.State(m.flat.copy(), m.exp_avg.copy(), m.exp_avg_sq.copy(), opt_steps, LR, int(m.shape.seed) >> 32,
                    int(m.shape.seed) & 0xFFFFFFFF, host_seq)


CASES = [  # n, card, B, waves per workgroup, steps, loss head run once (dvs_loss_forward_defer + dvs_loss_backward_emit)
    pytest.param(12, 12, 5, 4, 3, True, id="n12-B5-nw4-once"),
    pytest.param(12, 12, 5, 8, 3, True, id="n12-B5-nw8-once"),
    pytest.param(12, 12, 17, 8, 2, False, id="n12-B17-nw8-second-pass"),       # 2 'CUs' x 8 DAGs, then one more
    pytest.param(14, 14, 2, None, 2, False, id="n14-B2-wide"),                 # N = 17: the smallest wide shape
]


@pytest.mark.parametrize("n,card,B,nw,steps,once", CASES)
def test_emu_consecutive_steps_match_oracle_transitions(n, card, B, nw, steps, once, monkeypatch):
    if nw is None:
        monkeypatch.delenv("DVS_WAVES_PER_WG", raising=False)
    else:
        monkeypatch.setenv("DVS_WAVES_PER_WG", str(nw))
    cfg = po.PaceConfig(n=n, card=card)
    params = po.init_params(cfg, seed=5)
    f_np = ofeat.dense_features(ofeat.synthetic_dags(n, card, B, seed=3, density_limit=0.4), card)
    feats = ofeat.to_torch(f_np)
    m = EmuModel(cfg, {k: v.numpy() for k, v in params.items()}, B, training=True, dropout=ts.DROPOUT, seed=SEED << 32,
                 dag_offset=DAG_OFFSET, beta=ts.BETA)
    assert m.pack(f_np) == 0
    free = ts.FreeRun(cfg, params, LR)
    acts = ts.EmuActivations(m)
    host_seq = 40 if once else None
    for k in range(1, steps + 1):
        before = _state(m, k - 1, host_seq)
        m.advance_seed()
        if once:
            host_seq += 1
            m.forward_defer()
            _, losses, packet = m.backward_emit(host_seq, 1.0, ts.BETA, clip_scratch=m.clip_scratch)
            assert np.array_equal(packet[:3], losses[:3].view(np.uint32)) and packet[3] & 0xFF == 0
            host_seq = int(packet[3]) >> 8                    # what the device wrote, not what was asked for
        else:
            losses, _, _ = m.forward()
            m.backward(1.0, ts.BETA, clip_scratch=m.clip_scratch)
        assert losses[3] == 0.0 and losses[4] == 0.0
        m.clip_adam(k, LR, ts.MAX_NORM, from_partials=True, guard=losses[3:5])
        after = _state(m, k, host_seq)
        dev = ts.DeviceStep(float(losses[0]), float(losses[1]), float(losses[2]), m.grads.copy(), float(m.clip_scratch[0]),
                            float(m.clip_scratch[1]))
        ts.check_transition(f"train_steps[emu n={n},B={B},nw={nw},once={once}] step {k}", cfg, m.table, before, after, dev,
                            feats, acts, free, DAG_OFFSET)
