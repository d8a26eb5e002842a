"""GPU: the search's candidate stage on the device (search.decoded_structures / StructureSet / candidates="device",
csrc/dvs_structs.h) against the host stage it replaces, on real decode_states output, and the search pin: the same
search with candidates="host" and "device" gives the same result, exactly."""
import numpy as np
import pytest
import torch

from tests import structs_corpus as sc
from tests.helpers import graphs_from, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _asia_model():
    from dags_vae_search_amd import PaceVaeV3
    ck = load_npz("asia_ckpt110.npz")
    m = PaceVaeV3(8, 8, 32, 8, 3, 64, 32, 32, 0.15)
    m.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    return m.to(DEV).eval()


def _random_model(n):
    from dags_vae_search_amd import PaceVaeV3
    torch.manual_seed(0)
    return PaceVaeV3(n, n, 32, 8, 3, 64, 32, 32, 0.15).to(DEV).eval()


def _asia_latents(rows, seed):
    """Half posterior means of known asia graphs (mostly valid draws), half N(0, I)."""
    x = torch.from_numpy(load_npz("asia_predictor.npz")["x"]).float()
    g = torch.Generator().manual_seed(seed)
    near = x[torch.randint(0, len(x), (rows // 2,), generator=g)]
    return torch.cat([near, torch.randn(rows - rows // 2, x.shape[1], generator=g)]).to(DEV)


def _numpy(flags, compact, keys, hashes):
    preds = compact.preds.cpu().numpy()
    return (flags.cpu().numpy(), compact.labels.cpu().numpy(), preds.view(np.uint64 if preds.dtype == np.int64 else np.uint16),
            keys.cpu().numpy().view(np.uint64), hashes.cpu().numpy().view(np.uint64))


@pytest.mark.parametrize("name", ["asia", "n37"])
def test_decoded_rows_equal_the_host_stage(name):
    from dags_vae_search_amd.search import decoded_structures, hash_keys
    rows = 4096
    if name == "asia":
        model, n = _asia_model(), 8
        z = _asia_latents(rows, 5)
    else:
        model, n = _random_model(37), 37
        z = torch.randn(rows, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    model.seed(3)
    states = model.decode_states(z)
    out = decoded_structures(model, states)
    flags, labels, preds, keys, hashes = _numpy(*out)
    raw = states.cpu().numpy()
    assert raw.shape[0] >= 4096
    graphs, valid = sc.check_rows(raw, n, flags, labels, preds, keys)
    print(f"{name}: {int(valid.sum())} of {rows} rows valid; flags histogram {np.bincount(flags, minlength=9).tolist()}")
    if name == "asia":
        assert valid.sum() >= rows // 20 and (~valid).any()
    assert np.array_equal(hash_keys(out[2]).cpu().numpy().view(np.uint64)[valid], hashes[valid])
    assert (hashes[~valid] == sc.HASH_INVALID).all()
    again = decoded_structures(model, states)
    for a, b in zip(_numpy(*again), (flags, labels, preds, keys, hashes)):
        assert a.tobytes() == b.tobytes()
    # the synthetic corpus of the emulator test, on the device
    craw, _, _ = sc.corpus(n)
    cout = _numpy(*decoded_structures(model, torch.from_numpy(craw).to(DEV)))
    sc.check_rows(craw, n, *cout[:4])


def test_structure_set_equals_new_structures_on_decoded_rows():
    from dags_vae_search_amd import LabeledGraph, StructureSet
    from dags_vae_search_amd.search import decoded_structures, structure_key
    model, n = _asia_model(), 8
    initial = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_predictor_graphs.npz"), 8)][:256]
    results = []
    for mask in (sc.ALL_ONES, 0xF):
        seen = {structure_key(g) for g in initial}
        sset = StructureSet(n, DEV, hash_mask=mask)
        assert sset.add_graphs(initial) == len(seen) == len(sset)
        model.seed(9)
        verdicts = []
        for batch in range(3):
            states = model.decode_states(_asia_latents(4096, 20 + batch))
            flags, compact, keys, hashes = decoded_structures(model, states, hash_mask=mask)
            graphs, valid = sc.host_view(states.cpu().numpy(), n)
            want = sc.host_new_mask(graphs, n, seen)
            v1 = sset._verdicts(keys, hashes, flags)
            assert torch.equal(v1, sset._verdicts(keys, hashes, flags))              # two calls: equal bytes
            got = sset.filter(keys, hashes, flags)
            assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)
            assert np.array_equal((v1 == 1).cpu().numpy(), want)
            assert len(sset) == len(seen)
            assert sset.contains(keys).cpu().numpy()[valid].all()                    # every valid row is in the set now
            assert not sset.filter(keys, hashes, flags, insert=False).any()
            verdicts.append(v1.cpu().numpy())
            print(f"mask {mask:#x} batch {batch}: valid {int(valid.sum())}, new {int(want.sum())}, set {len(sset)}")
        results.append(np.concatenate(verdicts))
        assert (results[-1] == 1).sum() >= 10 and (results[-1] == 2).any() and (results[-1] == 4).any()
    assert results[0].tobytes() == results[1].tobytes()
    # empty batch and a key that is not in the set
    empty = sset.filter(keys[:0], hashes[:0], flags[:0])
    assert empty.shape == (0,)
    other = torch.full((1, n), 1 << 40, dtype=torch.int64, device=DEV)
    assert not sset.contains(other).any()


def _same_search(a, b):
    strip = lambda r: [(h.iteration, h.n_candidates, h.n_valid, h.n_new, h.best_score, h.ei_max) for h in r.history]
    assert strip(a) == strip(b)
    assert len(a.evaluated) == len(b.evaluated) and a.n_initial == b.n_initial
    for (g1, s1), (g2, s2) in zip(a.evaluated, b.evaluated):
        assert [int(x) for x in g1.labels] == [int(x) for x in g2.labels]
        assert [(int(u), int(v)) for u, v in g1.edges] == [(int(u), int(v)) for u, v in g2.edges]
        assert np.float64(s1).tobytes() == np.float64(s2).tobytes()
    assert list(a.best_graph.labels) == list(b.best_graph.labels) and list(a.best_graph.edges) == list(b.best_graph.edges)
    assert a.best_score == b.best_score


@pytest.mark.parametrize("cfg", [{}, {"batch_size": 128, "decode_tries": 8, "iterations": 2}], ids=["32x4", "128x8"])
def test_search_pin_host_and_device_candidates_agree_exactly(cfg):
    from tests.test_gpu_search import _run_search
    _, host, _ = _run_search(1234, candidates="host", **cfg)
    _, dev, _ = _run_search(1234, candidates="device", **cfg)
    _same_search(host, dev)
    assert sum(h.n_new for h in dev.history) >= 1
    assert all("candidates" in h.timings_ms for h in dev.history)
    _, default, _ = _run_search(1234, **cfg)                 # the default is the host path
    _same_search(host, default)
    assert all("candidates" not in h.timings_ms for h in default.history)


@pytest.mark.parametrize("source", ["prior", "near_data"])
def test_generation_metrics_equal_host_counts(source):
    """Draws from N(0, I) (the definition; measured on the asia checkpoint: 0 of 4 096 valid, its posteriors lie far from
    the prior) and from latents around the data (valid, repeated and novel structures all occur)."""
    from dags_vae_search_amd import LabeledDag, LabeledGraph, generation_metrics
    from dags_vae_search_amd.search import generation_latents, is_search_valid, structure_key
    model, n = _asia_model(), 8
    train = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_predictor_graphs.npz"), 8)][:512]
    rows, seed = 4096, 17
    if source == "prior":
        got = generation_metrics(model, train, rows, seed)
        z = generation_latents(model, rows, seed)
    else:
        x = torch.from_numpy(load_npz("asia_predictor.npz")["x"]).float()
        g = torch.Generator().manual_seed(seed)
        # posterior means of known graphs (most of them outside `train`), half of them with a little noise: the decoder
        # of this checkpoint is sharp (measured: N(0, 0.3^2) noise leaves 12 valid draws of 4 096, N(0, 0.5^2) none)
        noise = 0.05 * (torch.arange(rows) % 2).float()[:, None]
        z = x[torch.randint(0, len(x), (rows,), generator=g)] + noise * torch.randn(rows, x.shape[1], generator=g)
        got = generation_metrics(model, train, seed=seed, latents=z)
    model.seed(seed)
    draws = model.decode(z.to(DEV), strict=False)
    dag = LabeledDag(n, n)
    valid = [g for g in draws if is_search_valid(g, dag)]
    unique = {structure_key(g) for g in valid}
    novel = unique - {structure_key(g) for g in train}
    print(got)
    assert (got["n_samples"], got["n_valid"], got["n_unique"], got["n_novel"]) == (rows, len(valid), len(unique), len(novel))
    assert got["validity"] == len(valid) / rows and got["uniqueness"] == len(unique) / max(len(valid), 1)
    assert got["novelty"] == len(novel) / max(len(unique), 1)
    if source == "near_data":
        assert 1 <= len(novel) < len(unique) < len(valid)


def test_device_candidates_need_a_permutation_data_set():
    from dags_vae_search_amd import PaceVaeV3
    from dags_vae_search_amd.search import decoded_structures
    m = PaceVaeV3(12, 1, 32, 8, 3, 64, 32, 32, 0.15).to(DEV).eval()
    states = m.decode_states(torch.zeros(4, 32, device=DEV))
    with pytest.raises(ValueError):
        decoded_structures(m, states)
