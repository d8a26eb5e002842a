"""GPU: BN parameters (csrc/dvs_params.h) through the raw calls with the cases, references and checks of
tests/params_corpus.py — shared with the emulator twin tests/test_emu_params.py — plus the Python surface
(dags_vae_search_amd/params.py): FittedBN, bn_fit, sample, log_likelihood, cross_validate, BNLearnWrapper.from_packed."""
import ctypes
import functools

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import params_corpus as pm
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _dev_masks(masks):
    import torch
    return torch.from_numpy(np.ascontiguousarray(masks, U64).view(np.int64)).cuda()


@pytest.mark.parametrize("name", pm.FIT_CASE_NAMES)
def test_fit_equals_exact_rationals(name):
    pm.check_fit_case(backend(), name)


def test_fit_refuses_a_bad_slot_alone():
    pm.check_fit_bad_slots(backend())


@pytest.mark.parametrize("n_rows", pm.ROW_COUNTS)
def test_sample_equals_the_restatement(n_rows):
    pm.check_sample(backend(), "small", n_rows)


@pytest.mark.parametrize("name", ("chain48", "hand"))
def test_sample_networks(name):
    pm.check_sample(backend(), name, 300)


def test_sample_never_draws_a_zero_probability_level():
    pm.check_sample_zero_levels(backend())


def test_sample_lds_and_global_thresholds_give_the_same_bytes():
    pm.check_sample_lds_and_global(backend())


def test_sample_chunks_and_row_offset():
    pm.check_sample_chunks(backend())


def test_sample_refusals():
    pm.check_sample_refusals(backend())


@pytest.mark.parametrize("n_rows", pm.ROW_COUNTS)
def test_loglik_equals_fsum_of_logs(n_rows):
    pm.check_loglik_rows(backend(), n_rows)


def test_loglik_zero_nan_bad_level_and_bad_slot():
    pm.check_loglik_special(backend())


@pytest.mark.parametrize("name", ("asia", "sachs"))
def test_loglik_of_the_mle_fit_equals_the_scorer(name):
    pm.check_loglik_equals_scorer(backend(), name)


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    pm.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_bn_fit_surface_equals_the_raw_call_and_refuses_an_oversized_family():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, FittedBN, bn_fit
    case = pm.fit_case("sixS1000")
    ev = BNLearnWrapper("six", "bic", data=case.data)
    ev = BNLearnWrapper.from_packed("six", "bic", ev.packed, case.card)          # card as given: variable 1 misses its top level
    offsets = pm.offsets_of(case.card, case.masks)
    for method, iss, unobserved in (("mle", None, "nan"), ("mle", None, "uniform"), ("bayes", 10.0, "nan")):
        f = bn_fit(ev, _dev_masks(case.masks), method=method, iss=iss, unobserved=unobserved)
        assert isinstance(f, FittedBN) and f.cpt.is_cuda and f.cpt.dtype == torch.float64 and (f.batch, f.n_vars) == (3, 6)
        _, raw, status = pm.run_fit(backend(), case.data, case.card, case.masks, 0 if method == "mle" else 1, iss or 1.0,
                                    1 if unobserved == "uniform" else 0)
        assert status == 0 and f.cpt.cpu().numpy().tobytes() == raw.tobytes() and f.offsets_host == offsets.tolist()
    t = f.table(3, 0)                                                            # parents 2 and 5: 256 configurations of 2 levels
    assert t.shape == (256, 2) and t.data_ptr() == f.cpt.data_ptr() + 8 * int(offsets[3])
    assert f.n_params(1) == sum(c - 1 for c in pm.SIX_CARDS) and f.n_params(0) == 2 + 3 * 3 + 15 * 12 + 256 + 0 + 15
    one = bn_fit(ev, _dev_masks(case.masks[1]))                                  # [n]: one structure
    assert one.batch == 1 and one.cpt.numel() == sum(pm.SIX_CARDS)
    cards, _ = pm.boundary_cards()
    big = pm.fit_case("boundary")
    evb = BNLearnWrapper.from_packed("boundary", "bic", _dev_masks(sc.pack(big.data)), big.card)
    with pytest.raises(ValueError, match="cells"):
        bn_fit(evb, _dev_masks(big.masks))
    assert bn_fit(evb, _dev_masks(sc.masks_of(len(cards), {0: [1, 2, 3]}))).table(0).shape == (4096, 9)
    with pytest.raises(ValueError, match="iss"):
        bn_fit(ev, _dev_masks(case.masks), iss=1.0)
    with pytest.raises(ValueError, match="method"):
        bn_fit(ev, _dev_masks(case.masks), method="em")


def test_sample_surface_from_tables_chunks_and_from_packed_scores():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, FittedBN, sample
    net = pm.network("hand")
    f = FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables)
    rows = sample(f, 1000, seed=11)
    assert rows.is_cuda and rows.dtype == torch.int64 and rows.shape == (1000, 1)
    ref = pm.sample_ref(net, 1000, 11)
    assert rows.cpu().numpy().view(U64).tobytes() == sc.pack(ref).tobytes()
    assert torch.equal(rows, torch.cat([sample(f, 400, seed=11), sample(f, 600, seed=11, row_offset=400)]))
    # a sample scores like an evaluator built from the unpacked array, with no host round trip
    masks = _dev_masks(np.stack([net.masks, np.zeros(3, U64)]))
    packed = BNLearnWrapper.from_packed("hand", "bic", rows, net.card)
    unpacked = BNLearnWrapper("hand", "bic", data=ref)
    assert packed.card_host == unpacked.card_host                              # every level was drawn here
    assert packed.score_masks(masks).cpu().numpy().tobytes() == unpacked.score_masks(masks).cpu().numpy().tobytes()
    bde = BNLearnWrapper.from_packed("hand", "bde", rows, net.card, iss=10.0)
    assert bde.score_masks(masks).cpu().numpy().tobytes() == \
        BNLearnWrapper("hand", "bde", data=ref, iss=10.0).score_masks(masks).cpu().numpy().tobytes()
    bad = [t.copy() for t in net.tables]
    bad[1][0] = [0.5, 0.6]
    with pytest.raises(ValueError, match="probability vector"):
        sample(FittedBN.from_tables([int(m) for m in net.masks], net.card, bad), 10, seed=1)
    with pytest.raises(ValueError, match="cycle"):
        sample(FittedBN.from_tables([4, 1, 3], net.card, [np.full((2, 2), 0.5)] + net.tables[1:]), 10, seed=1)
    with pytest.raises(ValueError, match=r"\[q, r\]"):
        FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables[:2] + [np.full((2, 2), 0.5)])


def test_log_likelihood_surface_equals_the_raw_call():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, bn_fit, log_likelihood
    data, card, masks, offsets, cpt = pm.loglik_inputs()
    ev = BNLearnWrapper.from_packed("six", "bic", _dev_masks(sc.pack(data)), card)
    f = bn_fit(ev, _dev_masks(masks), method="bayes", iss=1.0)
    _, raw_rows, raw_out, _ = pm.run_loglik(backend(), data, card, masks, offsets, f.cpt.cpu().numpy())
    out, rows = log_likelihood(f, ev, per_row=True)
    assert out.is_cuda and out.dtype == torch.float64 and rows.shape == (3, 1000)
    assert out.cpu().numpy().tobytes() == raw_out.tobytes() and rows.cpu().numpy().tobytes() == raw_rows.tobytes()
    assert log_likelihood(f, ev.packed).cpu().numpy().tobytes() == raw_out.tobytes()
    high = data.copy()
    high[7, 3] = 5
    with pytest.raises(ValueError, match="level code"):
        log_likelihood(f, _dev_masks(sc.pack(high)))


@pytest.mark.parametrize("method,iss", (("mle", None), ("bayes", 1.0)))
@pytest.mark.parametrize("folds", (2, 10))
def test_cross_validate_equals_the_numpy_restatement(folds, method, iss):
    from dags_vae_search_amd import BNLearnWrapper, cross_validate, cv_folds
    case = hc.hc_case("asia")
    masks = np.stack([sc.masks_of(8, hc.ASIA_KNOWN)[0], np.zeros(8, U64)])
    ev = BNLearnWrapper("asia", "bic", data=case.data)
    assert np.array_equal(np.concatenate(cv_folds(5000, folds, 3)), pm.cv_permutation(5000, 3))
    got = cross_validate(ev, _dev_masks(masks), folds=folds, seed=3, method=method, iss=iss).cpu().numpy()
    ref, T = pm.cv_reference(case.data, case.card, masks, folds, 3, 0 if method == "mle" else 1, iss or 1.0)
    print(f"cross_validate folds {folds} {method}: {got.tolist()} reference {ref.tolist()}")
    pm._close(got, ref, T, ("cross_validate", folds, method))
    if method == "bayes":
        assert np.isfinite(got).all() and got[0] < got[1]                        # the golden structure predicts better than none
