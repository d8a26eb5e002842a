"""GPU: device-side reconstruction judging (dvs_match_decoded via recon.match_decoded / evaluate_reconstruction) against
the host judge on the same decoded graphs.  The host judge here is tests/iso_ref.py (no networkx on the GPU machines)."""
import math

import numpy as np
import pytest
import torch

from oracle import pace_oracle as po
from tests import iso_ref
from tests import recon_corpus as rc
from tests.helpers import graphs_from, load_golden, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _toolkit(n, card):
    from dags_vae_search_amd import LabeledDag

    class Judge(LabeledDag):
        def graph_equals(self, g1, g2, attributes_match=True):
            return iso_ref.graph_equals(g1, g2, attributes_match)

    return Judge(n, card)


def build_model(cfg, params):
    from dags_vae_search_amd import PaceVaeV3
    m = PaceVaeV3(cfg.n, cfg.card, 32, 8, 3, 64, 32, 32, 0.15)
    m.load_state_dict(params)
    return m.to(DEV).eval()


def host_flags(toolkit, targets, decoded, repeats):
    out = []
    for k, g in enumerate(decoded):
        t = targets[k // repeats]
        s = toolkit.graph_equals(t, g, attributes_match=False)
        out.append(int(toolkit.is_valid_graph(g)) | 2 * int(s) | 4 * int(s and toolkit.graph_equals(t, g)))
    return np.asarray(out, np.uint8)


@pytest.mark.parametrize("name", ["asia", "n12c1", "n12c12", "n13c5", "n29c7", "n37c37", "n45c45"])
def test_flags_equal_host_judge_on_decoded_rows(name):
    from dags_vae_search_amd.recon import match_decoded, topological_targets
    cfg, params, graphs, z = load_golden(name)
    B, R = min(16, len(graphs)), 4
    model = build_model(cfg, params)
    mu = torch.from_numpy(z["eval/mu"][:B].copy()).to(DEV)
    zz = mu.repeat_interleave(R, dim=0)
    U = torch.from_numpy(np.random.default_rng(17).random((B * R, cfg.N, cfg.N)).astype(np.float32)).to(DEV)
    targets = graphs[:B]
    flags = match_decoded(topological_targets(targets, cfg.n), model.decode_states(zz, U), R, cfg.card).cpu().numpy()
    decoded = model.decode(zz, uniforms=U, strict=False)
    want = host_flags(_toolkit(cfg.n, cfg.card), targets, decoded, R)
    assert not (flags & 8).any()
    bad = [(k, int(flags[k]), int(want[k])) for k in range(B * R) if flags[k] != want[k]]
    assert not bad, bad[:8]


def test_synthetic_corpus_on_the_device():
    from dags_vae_search_amd.recon import match_decoded
    from dags_vae_search_amd.records import encode_graphs
    for (n, card), pairs in rc.corpus(lambda a, b, attr=True: iso_ref.graph_equals(a, b, attr)).items():
        targets = [t for t, _ in pairs]
        raw = rc.states_of([g for _, g in pairs], n)
        flags = match_decoded(encode_graphs(targets, n), torch.from_numpy(raw).to(DEV), 1, card).cpu().numpy()
        want = host_flags(_toolkit(n, card), targets, [g for _, g in pairs], 1)
        assert list(flags) == list(want), (n, card)


def _asia():
    ck = load_npz("asia_ckpt110.npz")
    model = build_model(po.PaceConfig(n=8, card=8), {k: torch.from_numpy(ck[k]) for k in ck.files})
    from dags_vae_search_amd import LabeledGraph
    graphs = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_known_answer.npz"), 8)][:77]
    return model, graphs


def test_evaluate_reconstruction_asia():
    from dags_vae_search_amd import evaluate_reconstruction
    model, graphs = _asia()
    tk = _toolkit(8, 8)
    lines = []
    out = evaluate_reconstruction(model, graphs, tk, batch_size=32, encode_times=2, decode_times=2, seed=5, log=lines.append)
    assert out["graphs"] == 77 and len(lines) == 3 and out["undecided"] == 0
    assert out["valid_ratio"] == 1.0 and out["recon_accuracy"] >= 0.7 and out["recon_loss"] < 0.5
    assert out["structure_accuracy"] >= out["recon_accuracy"]
    again = evaluate_reconstruction(model, graphs, tk, batch_size=32, encode_times=2, decode_times=2, seed=5)
    assert again == out


def test_rates_agree_with_model_test_n12c1():
    from dags_vae_search_amd import evaluate_reconstruction, model_test
    cfg, params, graphs, _ = load_golden("n12c1")
    model = build_model(cfg, params)
    tk = _toolkit(12, 1)
    dev = evaluate_reconstruction(model, graphs, tk, batch_size=32, encode_times=4, decode_times=4, seed=3)
    host = model_test(model, graphs, tk, batch_size=32, encode_times=2, decode_times=2, seed=3)
    n1, n2 = len(graphs) * 16, len(graphs) * 4
    assert dev["undecided"] == 0
    for key in ("valid_ratio", "recon_accuracy"):
        p = (dev[key] * n1 + host[key] * n2) / (n1 + n2)
        sigma = math.sqrt(max(p * (1 - p), 1e-4) * (1 / n1 + 1 / n2))
        assert abs(dev[key] - host[key]) <= 4 * sigma, (key, dev[key], host[key])
    assert abs(dev["recon_loss"] - host["recon_loss"]) <= 1e-4 * max(1.0, abs(host["recon_loss"]))


def test_split_calls_give_the_same_flags():
    from dags_vae_search_amd.recon import match_decoded, topological_targets
    cfg, params, graphs, z = load_golden("n12c1")
    model = build_model(cfg, params)
    B, R = 24, 10
    model.seed(1)
    states = model.decode_states(torch.from_numpy(z["eval/mu"][:B].copy()).to(DEV).repeat_interleave(R, dim=0))
    targets = topological_targets(graphs[:B], cfg.n)
    whole = match_decoded(targets, states, R, cfg.card)
    parts = torch.cat([match_decoded(targets[s:s + 5], states[s * R:(s + 5) * R], R, cfg.card) for s in range(0, B, 5)])
    assert torch.equal(whole, parts)
    assert (whole & 6).any()
