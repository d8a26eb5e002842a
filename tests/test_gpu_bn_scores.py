"""GPU: dvs_bn_scores (csrc/k_bic.hip: loglik, aic, bic, bde, bds, k2, bdj) through the raw C ABI with the cases, references,
tolerances and checks of tests/bn_score_corpus.py — shared with the emulator twin tests/test_emu_bn_scores.py — and through
BNLearnWrapper, prepare_predictor_data and latent_bo_search with a bde evaluator.  Every case is deterministic; the
refusal cases are handled paths that come back through `status`."""
import math

import numpy as np
import pytest

from tests import bn_score_corpus as bn
from tests import scoring_corpus as sc
from tests.helpers import graphs_from, load_npz

pytestmark = pytest.mark.gpu
WORST = {}


@pytest.fixture(scope="module")
def be():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@pytest.mark.parametrize("name", sc.BIC_CASE_NAMES)
def test_bn_case(be, name):
    """Every (type, argument) of bn.VARIANTS on one case of the BIC corpus, each run twice for equal bytes: local scores
    and per-DAG sums within 1e-12 * T of the 60-digit reference.  The device library's lgamma gets no allowance of its
    own.  Worst |got - ref| / T on an MI355X: see DESIGN.md §9 (printed per type by test_report_worst_error_per_type)."""
    bn.check_all_variants(be, sc.bic_case(name), True, WORST)


def test_report_worst_error_per_type(be):
    bn.report(WORST, "device")


def test_k2_equals_the_log_of_exact_factorials(be):
    bn.check_k2_against_factorials(be)


def test_covered_edge_reversal_keeps_bde_bic_aic_loglik_and_moves_k2_bdj(be):
    bn.check_covered_edge_reversal(be)


@pytest.mark.parametrize("name", bn.BYTES_CASES)
def test_bic_bytes_equal_dvs_bic_scores_and_aic_meets_bic_and_loglik(be, name):
    bn.check_bic_bytes_and_aic_relations(be, name)


@pytest.mark.parametrize("name", bn.BDS_CASES)
def test_bds_equals_bde_where_every_configuration_is_observed(be, name):
    same, diff = bn.check_bds_against_bde(be, name)
    print(f"\n{name}: bds == bde in {same} cells, apart in {diff}")
    assert same > 0 and (diff > 0 or name != "levels")


def test_dense_and_sort_paths_agree_on_one_table(be):
    worst = bn.check_dense_and_sort_paths_agree(be)
    print(f"\ndense vs sort: worst |dense - sort| / T = {worst:.3g}")


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def _asia():
    from dags_vae_search_amd import LabeledGraph
    data = load_npz("bn_asia_data.npz")["data"]
    graphs = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_predictor_graphs.npz"), 8)]
    return data, graphs


def _reference_scores(data, graphs, typ, arg):
    """per-graph (score, T) from the corpus reference; graph vertex v stands for variable labels[v]"""
    card = (data.max(0) + 1).astype(np.uint8)
    data = data.astype(np.uint8)
    memo, out = {}, []
    for g in graphs:
        parents = {int(l): [] for l in g.labels}
        for u, v in g.edges:
            parents[int(g.labels[v])].append(int(g.labels[u]))
        loc = []
        for v, ps in parents.items():
            key = (v, tuple(sorted(ps)))
            if key not in memo:
                memo[key] = bn.reference_local(bn.cell_counts(data, card, v, ps), typ, arg)
            loc.append(memo[key])
        out.append((math.fsum(x for x, _ in loc), math.fsum(t for _, t in loc)))
    return out


@pytest.mark.parametrize("typ,kw", [("bde", {"iss": 10}), ("bde", {}), ("bds", {"iss": 3}), ("k2", {}), ("bdj", {}),
                                    ("loglik", {}), ("aic", {}), ("aic", {"k": 2.5}), ("bic", {"k": 0.75})])
def test_wrapper_score_batch_against_the_corpus_reference(typ, kw):
    import torch
    from dags_vae_search_amd import BNLearnWrapper
    data, graphs = _asia()
    graphs = graphs[:200]
    ev = BNLearnWrapper("asia", typ, data=data, **kw)
    got = ev.score_batch(graphs)
    want = _reference_scores(data, graphs, typ, kw.get("iss", kw.get("k")))
    for g, (w, T) in zip(got, want):
        assert abs(g - w) <= bn.RTOL * T, (typ, kw, g, w)
    assert ev.score(graphs[3]) == got[3]
    masks = torch.from_numpy(ev._parent_masks(graphs, "type").view(np.int64))
    total, local = ev.score_masks(masks, local=True)
    assert local.shape == (len(graphs), 8) and local.dtype == torch.float64 and total.shape == (len(graphs),)
    assert torch.equal(total, ev.score_masks(masks))
    loc = local.cpu().numpy()
    seq = np.zeros(len(graphs))
    for v in range(8):                                  # k_bic_sum adds the variables in order
        seq = seq + loc[:, v]
    assert np.array_equal(seq, total.cpu().numpy())
    assert total.cpu().tolist() == got


def test_wrapper_default_bic_is_unchanged_and_iss_with_bic_is_refused():
    import torch
    from dags_vae_search_amd import BNLearnWrapper
    data, graphs = _asia()
    with pytest.raises(ValueError):
        BNLearnWrapper("asia", "bic", data=data, iss=10)
    with pytest.raises(ValueError):
        BNLearnWrapper("asia", "bde", data=data, k=1.0)
    with pytest.raises(NotImplementedError):
        BNLearnWrapper("asia", "mbde", data=data)
    a = BNLearnWrapper("asia", "bic", data=data).score_batch(graphs[:64])
    b = BNLearnWrapper("asia", "bic", data=data, k=0.5 * math.log(len(data))).score_batch(graphs[:64])
    assert a[0] == pytest.approx(b[0], rel=1e-12) and max(abs(x - y) for x, y in zip(a, b)) <= 1e-9


def _asia_model():
    import torch
    from dags_vae_search_amd import PaceVaeV3
    ck = load_npz("asia_ckpt110.npz")
    m = PaceVaeV3(8, 8, 32, 8, 3, 64, 32, 32, 0.15)
    m.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    return m.to("cuda:0").eval()


def test_predictor_data_with_a_bde_evaluator_gives_score_batch_targets():
    from dags_vae_search_amd import BNLearnWrapper, prepare_predictor_data
    data, graphs = _asia()
    graphs = graphs[:192]
    ev = BNLearnWrapper("asia", "bde", data=data, iss=10)
    vec, tgt = prepare_predictor_data(_asia_model(), graphs, ev, batch_size=64)
    assert vec.shape == (192, 32) and tgt.is_cuda
    assert tgt.cpu().tolist() == ev.score_batch(graphs)
    _, tgt2 = prepare_predictor_data(_asia_model(), graphs[:64], ev.score, batch_size=64)     # the reference's call shape
    assert tgt2.cpu().tolist() == ev.score_batch(graphs[:64])
    bic = BNLearnWrapper("asia", "bic", data=data).score_batch(graphs[:8])
    assert all(abs(x - y) > 1e-3 for x, y in zip(bic, tgt.cpu().tolist()[:8]))                  # it is not BIC again


def test_latent_search_on_device_candidates_with_a_bde_evaluator():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, latent_bo_search
    from tests.test_gpu_search import shipped_gp
    data, graphs = _asia()
    graphs = graphs[:256]
    ev = BNLearnWrapper("asia", "bde", data=data, iss=10)
    fix = load_npz("asia_predictor.npz")
    y0 = torch.tensor(ev.score_batch(graphs), dtype=torch.float64)
    gp = shipped_gp(torch.from_numpy(fix["x"][:256]), y0)
    res = latent_bo_search(_asia_model(), gp, ev, graphs, iterations=2, batch_size=32, n_starts=256, steps=30, lr=0.02,
                           decode_tries=4, xi=0.0, variance="sor", seed=1234, candidates="device")
    assert res.n_initial == 256 and len(res.history) == 2 and len(res.evaluated) >= 256
    print(f"\nbde search: {[(h.n_candidates, h.n_valid, h.n_new, h.best_score) for h in res.history]}")
    again = ev.score_batch([g for g, _ in res.evaluated])
    assert [s for _, s in res.evaluated] == again
    assert res.best_score == max(again) and ev.score(res.best_graph) == res.best_score
