"""GPU: learning from incomplete data (csrc/dvs_incomplete.h) through the raw calls with the cases, references and checks of
tests/incomplete_corpus.py — shared with the emulator twin tests/test_emu_incomplete.py — plus the Python surface
(dags_vae_search_amd/incomplete.py: expected_counts, fit_counts, em_fit, impute, family_plans, incomplete_rows)."""
import functools

import numpy as np
import pytest

from tests import incomplete_corpus as nc
from tests import params_corpus as pm
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@functools.lru_cache(maxsize=None)
def _fitted(name):
    from dags_vae_search_amd import FittedBN
    net = nc.network(name)
    return FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables)


def _data(levels, observed):
    import torch
    return (torch.from_numpy(sc.pack(levels).view(np.int64)).cuda(), torch.from_numpy(observed.astype(U64).view(np.int64)).cuda())


def _bytes(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("n_rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("name", nc.BYTES_NETWORKS)
def test_expected_counts_equal_the_restatement(name, n_rows):
    nc.check_counts_bytes(backend(), name, n_rows)


@pytest.mark.parametrize("n_rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("name", nc.BYTES_NETWORKS)
def test_impute_equals_the_restatement(name, n_rows):
    nc.check_impute_bytes(backend(), name, n_rows)


def test_band48_equals_the_restatement():
    nc.check_counts_bytes(backend(), "band48", 257)
    nc.check_impute_bytes(backend(), "band48", 257)


@pytest.mark.parametrize("name", ("hand", "six", "asia", "band48"))
def test_rows_per_group_does_not_change_the_bytes(name):
    nc.check_counts_bytes(backend(), name, 257, nc.ROWS_PER_GROUP)
    nc.check_impute_bytes(backend(), name, 257, nc.ROWS_PER_GROUP)


@pytest.mark.parametrize("name", ("handfour", "wide3"))
def test_exact_ties_and_a_table_beyond_the_register_accumulators(name):
    nc.check_counts_bytes(backend(), name, 257, (0, 3))
    nc.check_impute_bytes(backend(), name, 257, (0, 3))


def test_plans_over_the_cap_are_a_value_error_through_the_python_surface():
    import torch
    import dags_vae_search_amd as dvs
    net = nc.network("full4")
    fitted = dvs.FittedBN.from_tables([int(m) for m in net.masks], net.card, nc.uniform_tables(net._replace(tables=[
        np.zeros((q, r)) for q, r in ((1, 16), (1, 16), (1, 16), (4096, 4))])))
    data = (torch.zeros(4, 1, dtype=torch.int64, device="cuda"), 0b0111)
    for call in (lambda: dvs.family_plans(fitted), lambda: dvs.expected_counts(fitted, data),
                 lambda: dvs.em_fit([int(m) for m in net.masks], net.card, data, max_iter=1)):
        with pytest.raises(ValueError, match="a last step of 16384 cells need 17472 cells; the cap is 16384"):
            call()
    rows, seen = dvs.impute(fitted, data)                                              # the plans of impute fit
    assert seen.tolist() == [15] * 4 and rows.tolist() == [[0]] * 4


def test_more_than_256_chunks_go_through_the_slots_of_the_tree():
    """65 537 rows of the three-variable network: larger than every other case on purpose — only beyond 256 chunks does a slot
    of the chunk tree and of the log-likelihood tree add more than one chunk value"""
    nc.check_counts_bytes(backend(), "hand", nc.MANY_CHUNKS_ROWS)
    nc.check_impute_bytes(backend(), "hand", nc.MANY_CHUNKS_ROWS)


def test_two_calls_give_equal_bytes():
    net = nc.network("asia")
    levels, observed, _ = nc.counts_case("asia", 600)
    words = [p.words for p in nc.family_plans("asia")]
    a = nc.run_expected_counts(backend(), net, words, levels, observed)
    b = nc.run_expected_counts(backend(), net, words, levels, observed)
    assert a.counts.tobytes() == b.counts.tobytes() and a.row_z.tobytes() == b.row_z.tobytes()
    assert np.float64(a.loglik).tobytes() == np.float64(b.loglik).tobytes()


@pytest.mark.parametrize("name", ("hand", "six", "zeroone", "asia"))
def test_fully_observed_counts_are_integers_and_fit_counts_is_bn_fit(name):
    nc.check_fully_observed(backend(), name)


def test_fit_counts_on_fractional_and_bad_counts():
    nc.check_fit_counts_fractional(backend())


def test_em_iterations_equal_the_restatement():
    nc.check_em_step(backend())


@pytest.mark.parametrize("name,targets", (("asia", (1, 4, 7)), ("band48", (0, 23, 47))))
def test_impute_with_every_other_variable_observed_equals_predict_exact(name, targets):
    nc.check_impute_equals_blanket(backend(), name, targets)


def test_malformed_plans_are_refused_alone_and_nothing_is_touched_outside_the_buffers():
    nc.check_malformed(backend())


def test_argument_refusals():
    nc.check_argument_refusals(backend().lib)


# ---- the Python surface ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("asia", "six"))
def test_expected_counts_and_fit_counts_equal_the_raw_calls(name):
    import dags_vae_search_amd as dvs
    net = nc.network(name)
    levels, observed = nc.incomplete_case(name, 257, special=False)
    ref = nc.restate_counts(net, nc.family_plans(name), levels, observed)
    fitted, data = _fitted(name), _data(levels, observed)
    got = dvs.expected_counts(fitted, data)
    assert _bytes(got.counts) == ref.counts.tobytes() and _bytes(got.row_z) == ref.row_z.tobytes()
    assert int(got.skipped.item()) == ref.skipped and got.n_rows == 257
    assert abs(float(got.log_likelihood.item()) - ref.loglik) <= pm.LOG_RTOL * ref.loglik_tol
    offsets = pm.offsets_of(net.card, net.masks[None, :])
    for v in range(len(net.card)):
        _, q, r = pm.family_shape(net.card, net.masks[v], v)
        assert got.table(v).shape == (q, r) and _bytes(got.table(v)) == ref.counts[int(offsets[v]):int(offsets[v + 1])].tobytes()
    plans = dvs.family_plans(fitted)
    again = dvs.expected_counts(fitted, data, plans=plans, rows_per_group=3)
    assert _bytes(again.counts) == _bytes(got.counts) and _bytes(again.log_likelihood) == _bytes(got.log_likelihood)
    with pytest.raises(ValueError, match="plans must be"):
        dvs.expected_counts(fitted, data, plans=plans[:-1])
    for method, iss, unobserved in (("mle", None, "nan"), ("mle", None, "uniform"), ("bayes", 2.5, "nan")):
        new = dvs.fit_counts(got, method=method, iss=iss, unobserved=unobserved)
        want = nc.fit_counts_ref(net, ref.counts, dvs._lib.FIT_METHODS[method], 1.0 if iss is None else iss, unobserved == "uniform")
        assert _bytes(new.cpt) == want.tobytes() and new.n_vars == len(net.card) and new.table(1).shape == got.table(1).shape


def test_a_bad_level_is_a_value_error_and_an_impossible_row_is_skipped():
    import dags_vae_search_amd as dvs
    levels, observed, ref = nc.counts_case("zeroone", 257)
    fitted = _fitted("zeroone")
    with pytest.raises(ValueError, match="level count"):
        dvs.expected_counts(fitted, _data(levels, observed))
    with pytest.raises(ValueError, match="level count"):
        dvs.impute(fitted, _data(levels, observed))
    keep = np.arange(257) != 3
    net = nc.network("zeroone")
    want = nc.restate_counts(net, nc.family_plans("zeroone"), levels[keep], observed[keep])
    got = dvs.expected_counts(fitted, _data(levels[keep], observed[keep]))
    assert want.skipped == 1 and int(got.skipped.item()) == 1 and _bytes(got.counts) == want.counts.tobytes()
    rows, seen = dvs.impute(fitted, _data(levels[keep], observed[keep]))
    assert int(seen[2].item()) == int(observed[2]) and int(rows[2, 0].item()) == int(sc.pack(np.where(nc.seen_of(observed, 5), levels, 0)[2:3])[0, 0])


def test_fully_observed_em_iteration_is_bn_fit():
    import torch
    import dags_vae_search_amd as dvs
    net = nc.network("asia")
    levels = pm.sample_ref(net, 300, seed=43)
    packed = torch.from_numpy(sc.pack(levels).view(np.int64)).cuda()
    ev = dvs.BNLearnWrapper.from_packed("asia-sample", "bic", packed, [int(c) for c in net.card])
    parents = torch.from_numpy(net.masks.view(np.int64)).cuda()
    for method, iss in (("mle", None), ("bayes", 3.0)):
        ref = dvs.bn_fit(ev, parents, method=method, iss=iss, unobserved="uniform")
        em = dvs.em_fit([int(m) for m in net.masks], net.card, (packed, (1 << 8) - 1), method=method, iss=iss, max_iter=1)
        assert _bytes(em.fitted.cpt) == _bytes(ref.cpt) and em.iterations == 1 and not em.converged and em.skipped == 0


def test_em_fit_on_asia_is_monotone_equals_the_restatement_and_reports_skipped():
    import dags_vae_search_amd as dvs
    net = nc.network("asia")
    levels, observed = nc.incomplete_case("asia", 200, rate=0.2, special=False)
    tables, trace = nc.em_ref(net, nc.family_plans("asia"), levels, observed, 12)
    em = dvs.em_fit([int(m) for m in net.masks], net.card, _data(levels, observed), max_iter=12, tol=0.0)
    assert em.iterations == 12 and not em.converged and em.skipped == 0
    assert _bytes(em.fitted.cpt) == np.concatenate([t.reshape(-1) for t in tables]).tobytes()
    for t, (got, (ref, tol)) in enumerate(zip(em.log_likelihood, trace)):
        assert abs(got - ref) <= 2 * pm.LOG_RTOL * tol, (t, got, ref)
        if t:
            assert got >= em.log_likelihood[t - 1] - pm.LOG_RTOL * (tol + trace[t - 1][1]), (t, em.log_likelihood)
    print("asia EM log-likelihood:", [f"{x:.6f}" for x in em.log_likelihood])
    stop = dvs.em_fit([int(m) for m in net.masks], net.card, _data(levels, observed), max_iter=50, tol=1e-3)
    assert stop.converged and 2 <= stop.iterations < 50
    start = dvs.em_fit([int(m) for m in net.masks], net.card, _data(levels, observed), start=_fitted("asia"), max_iter=2, tol=0.0)
    assert start.log_likelihood[0] > em.log_likelihood[0]                               # the generating tables beat the uniform ones
    zero = dvs.em_fit([int(m) for m in nc.network("zeroone").masks], nc.network("zeroone").card,
                      _data(*[a[np.arange(257) != 3] for a in nc.counts_case("zeroone", 257)[:2]]), start=_fitted("zeroone"), max_iter=1)
    assert zero.skipped == 1


@pytest.mark.parametrize("name", ("asia", "handfour"))
def test_impute_equals_the_raw_call_and_plans_are_reusable(name):
    import dags_vae_search_amd as dvs
    net = nc.network(name)
    levels, observed = nc.incomplete_case(name, 257, special=False)
    want_levels, want_seen, status = nc.restate_impute(net, nc.target_plans(name), levels, observed)
    fitted, data = _fitted(name), _data(levels, observed)
    rows, seen = dvs.impute(fitted, data)
    assert status == 0 and _bytes(rows) == sc.pack(want_levels).tobytes() and _bytes(seen) == want_seen.tobytes()
    again = dvs.impute(fitted, data, plans=dvs.target_plans(fitted))
    assert _bytes(again[0]) == _bytes(rows) and _bytes(again[1]) == _bytes(seen)
    with pytest.raises(ValueError, match="plans must be"):
        dvs.impute(fitted, data, plans=dvs.family_plans(fitted)[:-1])
    # hard EM composes: impute, then fit on the completed rows
    ev = dvs.BNLearnWrapper.from_packed("imputed", "bic", rows, [int(c) for c in net.card])
    import torch
    hard = dvs.bn_fit(ev, torch.from_numpy(net.masks.view(np.int64)).cuda(), method="bayes")
    assert bool(torch.isfinite(hard.cpt).all())


def test_incomplete_rows_round_trips():
    import dags_vae_search_amd as dvs
    levels, observed = nc.incomplete_case("band48", 70, special=False)
    seen = nc.seen_of(observed, 48)
    rows, obs = dvs.incomplete_rows(np.where(seen, levels.astype(np.int64), -1))
    assert _bytes(obs) == observed.tobytes() and _bytes(rows) == sc.pack(np.where(seen, levels, 0).astype(np.uint8)).tobytes()
    assert (pm.unpack(rows.cpu().numpy().view(U64), 48)[seen] == levels[seen]).all()
    for bad in (np.zeros((3,), np.int64), np.zeros((2, 49), np.int64), np.full((2, 3), 16), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            dvs.incomplete_rows(bad)
