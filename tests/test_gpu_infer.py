"""GPU: inference on a fitted network (csrc/dvs_infer.h) through the raw calls with the cases, references and checks of
tests/infer_corpus.py — shared with the emulator twin tests/test_emu_infer.py — plus the Python surface
(dags_vae_search_amd/infer.py: cpquery, cpdist, posterior, predict; params.py: cross_validate's prediction losses)."""
import functools

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import infer_corpus as ic
from tests import params_corpus as pm
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, U64).view(np.int64)).cuda()


def _fitted(net):
    from dags_vae_search_amd import FittedBN
    return FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables)


@pytest.mark.parametrize("n_particles", ic.PARTICLE_COUNTS)
@pytest.mark.parametrize("name", ic.LW_NETWORKS)
def test_lw_equals_the_restatement(name, n_particles):
    ic.check_lw_case(backend(), name, n_particles)


def test_lw_evidence_of_probability_zero_weighs_exactly_zero():
    ic.check_lw_zero_theta(backend())


def test_lw_one_call_equals_each_query_alone_with_its_offset():
    ic.check_lw_query_offset(backend())


def test_lw_lds_and_global_thresholds_give_the_same_bytes():
    ic.check_lw_lds_and_global(backend())


def test_lw_refusals():
    ic.check_lw_refusals(backend())


@pytest.mark.parametrize("n_rows", ic.ROW_COUNTS)
@pytest.mark.parametrize("name", ("asia", "sachs"))
def test_blanket_posterior_equals_the_numpy_products(name, n_rows):
    ic.check_blanket_rows(backend(), name, n_rows)


def test_blanket_posterior_ties_zero_rows_nan_bad_level_and_bad_slot():
    ic.check_blanket_special(backend())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    ic.check_argument_refusals(dl.load())


@pytest.mark.parametrize("case", ic.STAT_BLANKET_CASES, ids=lambda c: f"{c.network}-target{c.targets.bit_length() - 1}")
def test_lw_on_the_device_agrees_with_the_exact_blanket_posterior(case):
    """the device's own numbers, both kernels: every variable but the target observed, 4096 particles, 5 standard errors"""
    net = ic.stat_network(case.network)
    n = len(net.card)
    (target,) = ic.targets_of(case.targets)
    row = np.zeros((1, n), np.uint8)
    for v, k in case.evidence.items():
        row[0, v] = k
    observed = ((1 << n) - 1) & ~(1 << target)
    lw = ic.run_lw(backend(), net, row, [observed], ic.STAT_PARTICLES, case.seed, 0, None, case.targets, False)
    offsets, cpt = pm.flat_network(net)
    exact = ic.run_blanket(backend(), row, net.card, net.masks[None, :], offsets, cpt, target, 1)
    assert lw.rc == exact.rc == 0 and lw.status == exact.status == 0
    se = ic.lw_exact(net, row[0], observed, None, case.targets).marginal_se[0, :int(net.card[target])]
    dev = np.abs(lw.marginals[0, 0, :len(se)] / lw.sums[0, 0] - exact.posterior[0, 0]) / se
    print(f"{case.network} target {target}: deviations {dev.tolist()} standard errors")
    assert (dev <= ic.STAT_SIGMAS).all()


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_cpquery_cpdist_and_posterior_equal_the_raw_call():
    import torch
    from dags_vae_search_amd import cpdist, cpquery, posterior
    net = ic.hand_four()
    f = _fitted(net)
    event = {1: 1, 2: [0, 2]}
    words = ic.event_words(4, {1: [1], 2: [0, 2]})
    ev = np.array([[0, 0, 0, 1]], np.uint8)
    raw = ic.run_lw(backend(), net, ev, [0b1000], 1000, 5, 0, words, 0b0111, True)
    got = cpquery(f, event, {3: 1}, n=1000, seed=5)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (1,)
    assert got.cpu().numpy().tobytes() == (raw.sums[:, 2] / raw.sums[:, 0]).tobytes()
    post = posterior(f, [2, 0, 1], {3: 1}, n=1000, seed=5)
    assert post.shape == (1, 3, 16) and post.cpu().numpy().tobytes() == (raw.marginals / raw.sums[:, 0, None, None]).tobytes()
    parts, wts, ess = cpdist(f, [0, 2], {3: 1}, n=1000, seed=5)
    keep = U64(0xF0F)
    assert parts.shape == (1, 1000, 1) and parts.cpu().numpy().view(U64).tobytes() == (raw.particles & keep).tobytes()
    assert wts.cpu().numpy().tobytes() == raw.weights.tobytes()
    assert ess.cpu().numpy().tobytes() == (raw.sums[:, 0] * raw.sums[:, 0] / raw.sums[:, 1]).tobytes()
    # a batch of queries with a mask each, cut into calls
    rows = pm.sample_ref(net, 5, seed=8)
    observed = [0b1000, 0b0001, 0, 0b1111, 0b0110]
    raw = ic.run_lw(backend(), net, rows, observed, 300, 6, 0, words, 0, False)
    batch = (_dev(sc.pack(rows)), torch.tensor(observed, dtype=torch.int64).cuda())
    got = cpquery(f, event, batch, n=300, seed=6)
    assert got.cpu().numpy().tobytes() == (raw.sums[:, 2] / raw.sums[:, 0]).tobytes()
    tail = cpquery(f, event, (batch[0][2:], batch[1][2:]), n=300, seed=6, query_offset=2)
    assert torch.equal(tail, got[2:])
    shared = cpquery(f, event, (batch[0], 0b1000), n=300, seed=6)                # one mask for every row
    assert shared[0] == got[0]
    # impossible evidence is NaN, not an error; a level beyond the variable's count is one
    hand = _fitted(pm.network("hand"))
    assert torch.isnan(cpquery(hand, {0: 1}, {0: 0, 1: 0, 2: 1}, n=100, seed=1)).all()
    with pytest.raises(ValueError, match="level"):
        cpquery(hand, {0: 1}, {2: 3}, n=100, seed=1)
    with pytest.raises(ValueError, match="event"):
        cpquery(hand, {0: 2}, {2: 1}, n=100, seed=1)
    bad = [t.copy() for t in pm.network("hand").tables]
    bad[1][0] = [0.5, 0.6]
    from dags_vae_search_amd import FittedBN
    with pytest.raises(ValueError, match="probability vector"):
        cpquery(FittedBN.from_tables([0, 1, 3], [2, 2, 2], bad), {0: 1}, {2: 1}, n=100, seed=1)


def test_predict_equals_the_raw_calls():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, bn_fit, predict
    data, card, masks, offsets, _ = ic.bayes_fit("asia")
    ev = BNLearnWrapper("asia", "bic", data=data)
    f = bn_fit(ev, _dev(masks), method="bayes", iss=10.0)
    cpt = f.cpt.cpu().numpy()
    rows = data[:700]
    packed = _dev(sc.pack(rows))
    for target in (1, 7):
        for method, use_children in (("parents", 0), ("exact", 1)):
            raw = ic.run_blanket(backend(), rows, card, masks, offsets, cpt, target, use_children)
            for b in (0, 2):
                pred, post = predict(f, target, packed, method=method, prob=True, index=b)
                assert pred.dtype == torch.uint8 and pred.shape == (700,) and post.shape == (700, 2)
                assert pred.cpu().numpy().tobytes() == raw.pred[b].tobytes()
                assert post.cpu().numpy().tobytes() == raw.posterior[b].tobytes()
        assert torch.equal(predict(f, target, ev, method="exact", index=2)[:700], pred)     # an evaluator, predictions alone
        net = pm.Network("asia", card, masks[0], pm.tables_of(cpt, card, masks, offsets)[0])
        off0, cpt0 = offsets[:9], cpt[:int(offsets[8])]
        lw = ic.run_lw(backend(), net, rows, [0xFF & ~(1 << target)] * 700, 500, 0, 0, None, 1 << target, False,
                       offsets=off0, cpt=cpt0)
        pred, post = predict(f, target, packed, method="bayes-lw", prob=True)
        assert post.cpu().numpy().tobytes() == (lw.marginals[:, 0, :2] / lw.sums[:, :1]).tobytes()
        ref_post, ref_pred = ic.predict_lw_ref(net, rows, target, 500, 0)
        assert post.cpu().numpy().tobytes() == ref_post.tobytes() and pred.cpu().numpy().tobytes() == ref_pred.tobytes()
    with pytest.raises(ValueError, match="method"):
        predict(f, 1, packed, method="bayes")
    with pytest.raises(ValueError, match="level code"):
        high = rows.copy()
        high[3, 2] = 2
        predict(f, 1, _dev(sc.pack(high)), method="exact")


def test_exact_prediction_beats_parents_for_a_target_with_children():
    """rain in the hand network: its parents (none) always say "no rain"; sprinkler and wet grass tell more"""
    from dags_vae_search_amd import predict, sample
    net = pm.network("hand")
    f = _fitted(net)
    rows = sample(f, 5000, seed=21)
    truth = (rows[:, 0] & 15).cpu().numpy()
    wrong = {m: float((predict(f, 0, rows, method=m).cpu().numpy() != truth).mean()) for m in ("parents", "exact", "bayes-lw")}
    print(f"hand network, target rain, 5000 sampled rows: share predicted wrongly {wrong}")
    assert wrong["exact"] < wrong["parents"] and wrong["bayes-lw"] < wrong["parents"]
    assert abs(wrong["parents"] - 0.2) < 5 * (0.2 * 0.8 / 5000) ** 0.5          # the prior of rain, within 5 binomial sigmas


@pytest.mark.parametrize("loss", ("pred", "pred-exact", "pred-lw"))
@pytest.mark.parametrize("folds", (2, 10))
def test_cross_validate_prediction_losses_equal_the_numpy_restatement(folds, loss):
    from dags_vae_search_amd import BNLearnWrapper, cross_validate
    case = hc.hc_case("asia")
    masks = np.stack([sc.masks_of(8, hc.ASIA_KNOWN)[0], np.zeros(8, U64)])
    ev = BNLearnWrapper("asia", "bic", data=case.data)
    target = 4                                                                   # bronc: a parent (smoke) and two children
    got = cross_validate(ev, _dev(masks), folds=folds, seed=3, method="bayes", iss=1.0, loss=loss, target=target,
                         **({"n": 128} if loss == "pred-lw" else {}))
    ref = ic.cv_pred_reference(case.data, case.card, masks, folds, 3, 1.0, target, loss, M=128)
    print(f"cross_validate folds {folds} {loss}: {got.tolist()} reference {ref.tolist()}")
    assert got.cpu().numpy().tobytes() == ref.tobytes()
    assert got[0] < got[1]                                                       # the golden structure predicts bronc better than none
    if loss == "pred":
        with pytest.raises(ValueError, match="target"):
            cross_validate(ev, _dev(masks), folds=folds, loss=loss)
        with pytest.raises(ValueError, match="pred-lw"):
            cross_validate(ev, _dev(masks), folds=folds, loss=loss, target=target, n=100)
        with pytest.raises(ValueError, match="loss"):
            cross_validate(ev, _dev(masks), folds=folds, loss="hamming", target=1)
