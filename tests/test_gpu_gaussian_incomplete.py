"""GPU: a normal conditioned on every row's observed part (csrc/dvs_gaussian_incomplete.h) through the raw call with the cases,
the restatement and the checks of tests/gaussian_incomplete_corpus.py — shared with the emulator twin
tests/test_emu_gaussian_incomplete.py — plus the Python surface (dags_vae_search_amd/gaussian_incomplete.py): gaussian_condition,
gaussian_posterior, gaussian_impute, gaussian_incomplete_log_likelihood, expected_moments, gaussian_em_fit, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

from tests import gaussian_corpus as gc
from tests import gaussian_incomplete_corpus as gi
from tests import gaussian_params_corpus as gp
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _fitted(nets):
    import torch
    from dags_vae_search_amd import FittedGBN
    par, coef, icpt, sd = gp.stack(nets)
    return FittedGBN(torch.from_numpy(par.view(np.int64)).cuda(), torch.from_numpy(coef).cuda(), torch.from_numpy(icpt).cuda(),
                     torch.from_numpy(sd).cuda())


def _pair(x, masks):
    import torch
    return torch.from_numpy(np.array(x, np.float64, order="C")).cuda(), torch.from_numpy(np.asarray(masks, U64).view(np.int64).copy()).cuda()


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _net_of(fit):
    """the first structure of a FittedGBN as a corpus Net (host copies)"""
    par = [int(v) for v in fit.parents[0].cpu().numpy().view(U64)]
    return gp.Net(n=len(par), parents=par, coef=fit.coef[0].cpu().numpy(), intercept=fit.intercept[0].cpu().numpy(), sd=fit.sd[0].cpu().numpy())


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("n, S, kind", gi.shape_cases())
def test_condition_equals_the_restatement(n, S, kind):
    print(f"n {n} S {S} {kind}: worst logp difference / allowance {gi.check_condition(backend(), n, S, kind):.3e}")


def test_every_row_its_own_pattern():
    gi.check_unique_patterns(backend())


def test_a_run_across_a_chunk_boundary():
    gi.check_straddle(backend())


def test_second_level_of_the_tree():
    gi.check_second_level(backend())


def test_orders():
    gi.check_orders(backend())


def test_null_outputs_keep_the_other_bytes():
    gi.check_null_outputs(backend())


def test_refusals_between_neighbours():
    gi.check_refusals(backend())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    gi.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_python_functions_equal_the_raw_call():
    import torch
    from dags_vae_search_amd import (gaussian_condition, gaussian_impute, gaussian_incomplete_log_likelihood, gaussian_posterior,
                                     incomplete_real_rows)
    be, n, S = backend(), 17, 300
    nets = [gp.NETS[("hub", n)], gp.NETS[gi.NET_KEYS[n]]]
    fitted = _fitted(nets)
    x, masks = np.array(gp.rows_for(n, S), copy=True), gi.masks_for(n, S, "few")
    mean, cov = gi.joint_of(n)
    order = gi.sorted_order(masks)
    raw = gi.run_condition(be, mean, cov, x, masks, order)
    # incomplete_real_rows: NaN is missing, the stored cell is +0, and the unobserved cell never matters
    holes = np.where(((masks[:, None] >> np.arange(n, dtype=U64)) & U64(1)).astype(bool), x, np.nan)
    data = incomplete_real_rows(holes)
    assert _bytes(data[1]) == masks.tobytes() and _bytes(data[0]) == np.where(np.isnan(holes), 0.0, holes).tobytes()
    for pair in (data, _pair(x, masks)):
        got = gaussian_condition(fitted, pair, 1)
        assert _bytes(got.completed) == raw.completed.tobytes() and _bytes(got.var) == raw.cvar.tobytes()
        assert _bytes(got.quad) == raw.quad.tobytes() and _bytes(got.log_density) == raw.logp.tobytes()
        assert float(got.log_likelihood) == raw.loglik and _bytes(got.cov_sum) == raw.ccov.tobytes() and int(got.refused) == 0
    lean = gaussian_condition(fitted, data, 1, cov=False)
    assert lean.var is None and lean.cov_sum is None and _bytes(lean.completed) == raw.completed.tobytes()
    unsorted = gaussian_condition(fitted, data, 1, order=None)
    assert _bytes(unsorted.completed) == raw.completed.tobytes() and _bytes(unsorted.log_density) == raw.logp.tobytes()
    assert float(unsorted.log_likelihood) == gi.run_condition(be, mean, cov, x, masks).loglik
    # impute leaves observed cells bit-identical; the log-likelihood and its rows
    filled = gaussian_impute(fitted, data, 1)
    seen = ~np.isnan(holes)
    assert _bytes(filled) == raw.completed.tobytes() and filled.cpu().numpy()[seen].tobytes() == x[seen].tobytes()
    total, rows = gaussian_incomplete_log_likelihood(fitted, data, 1, per_row=True)
    assert float(total) == raw.loglik and _bytes(rows) == raw.logp.tobytes()
    assert _bytes(gaussian_incomplete_log_likelihood(fitted, data, 1)) == _bytes(total)
    # the posterior of some targets: a dict is one evidence row
    pm, pv = gaussian_posterior(fitted, [3, 0, 16], data, 1)
    assert _bytes(pm) == raw.completed[:, [3, 0, 16]].tobytes() and _bytes(pv) == raw.cvar[:, [3, 0, 16]].tobytes()
    r = 5
    ev = {v: float(x[r, v]) for v in range(n) if (int(masks[r]) >> v) & 1}
    dm, dv = gaussian_posterior(fitted, [3, 0, 16], ev, 1)
    assert _bytes(dm) == raw.completed[r:r + 1, [3, 0, 16]].tobytes() and _bytes(dv) == raw.cvar[r:r + 1, [3, 0, 16]].tobytes()
    nothing = gaussian_posterior(fitted, 2, {}, 1)
    assert float(nothing[0]) == mean[2] and float(nothing[1]) == cov[2, 2]


@pytest.mark.parametrize("n", gp.PREDICT_N)
def test_posterior_given_the_whole_blanket_meets_the_exact_prediction(n):
    import torch
    from dags_vae_search_amd import gaussian_posterior, gaussian_predict
    net = gp.NETS[gi.NET_KEYS[n]]
    fitted, x = _fitted([net]), np.array(gp.rows_for(n, 6), copy=True)
    xd = torch.from_numpy(x).cuda()
    for t in gp.sinks_and_sources(net):
        mask = gi.blanket_mask(net, t)
        pred, var = gaussian_predict(fitted, t, xd, method="exact", var=True)
        pm, pv = gaussian_posterior(fitted, t, _pair(x, np.full(len(x), mask, U64)))
        ref = gi.pattern_reference(n, mask)
        for i in range(len(x)):
            bound, rel = gp.predict_bound(net, t, x[i])
            b = gi.row_reference(n, mask, x[i])[3]
            assert abs(float(pred[0, i]) - float(pm[i, 0])) <= bound + b.mean + gc.U * abs(float(pred[0, i])), (n, t, i)
        assert abs(float(var[0]) - float(pv[0, 0])) <= rel * float(var[0]) + ref.T_bound, (n, t)


def test_expected_moments_of_complete_data_are_the_evaluators_and_drive_the_searches_alike():
    import torch
    from dags_vae_search_amd import (GaussianEvaluator, GaussianMomentsEvaluator, ci_tests, exact_search, expected_moments, gaussian_fit,
                                     hill_climb)
    n = 5
    x = gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[0]
    fitted = _fitted([gp.LOOP_NET])
    full = np.full(len(x), (1 << n) - 1, U64)
    em = expected_moments(fitted, _pair(x, full))
    ev = GaussianEvaluator("loop", "bge", data=x)
    assert _bytes(em.moments) == _bytes(ev.moments) and em.refused == 0
    mine = em.evaluator("bge")
    assert isinstance(mine, GaussianMomentsEvaluator) and (mine.n_vars, mine.n_samples, mine.data_kind) == (n, len(x), "continuous")
    a, b = exact_search(ev), exact_search(mine)
    assert _bytes(a.parents) == _bytes(b.parents) and _bytes(a.scores) == _bytes(b.scores) and _bytes(a.rescored) == _bytes(b.rescored)
    start = torch.zeros(2, n, dtype=torch.int64, device="cuda")
    ha, hb = hill_climb(GaussianEvaluator("loop", "bic-g", data=x), start, max_steps=40), hill_climb(em.evaluator("bic-g"), start, max_steps=40)
    assert _bytes(ha.parents) == _bytes(hb.parents) and _bytes(ha.scores) == _bytes(hb.scores)
    fa, fb = gaussian_fit(ev, fitted.parents), gaussian_fit(mine, fitted.parents)
    assert all(_bytes(p) == _bytes(q) for p, q in zip((fa.coef, fa.intercept, fa.sd), (fb.coef, fb.intercept, fb.sd)))
    with pytest.raises(NotImplementedError, match="holds moments, not rows"):
        mine.with_rows(torch.zeros(1, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="expected\\) moments, not rows"):
        ci_tests(mine, torch.tensor([[0, 1]], dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"), test="cor")


def test_one_unbiased_em_step_on_complete_data_is_gaussian_fit():
    from dags_vae_search_amd import GaussianEvaluator, gaussian_em_fit, gaussian_fit
    x = gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[0]
    em = gaussian_em_fit(gp.LOOP_NET.parents, _pair(x, np.full(len(x), 31, U64)), variance="unbiased", max_iter=1)
    fit = gaussian_fit(GaussianEvaluator("loop", "bic-g", data=x), _fitted([gp.LOOP_NET]).parents)
    assert (em.iterations, em.converged, len(em.log_likelihood)) == (1, False, 1)
    assert all(_bytes(p) == _bytes(q) for p, q in zip((em.fitted.coef, em.fitted.intercept, em.fitted.sd), (fit.coef, fit.intercept, fit.sd)))


def test_em_steps_teacher_forced_against_the_restatement():
    """every step starts from the device's own parameters and is compared with one restated step from them: the parameters as
    bytes (neither the joint, the conditioning's cells, the moments nor the fit calls a library function: the bound the
    conditioning's cells carry between builds is zero, and dvs_gbn_fit adds none to a zero difference), the log-likelihood within
    the between-builds allowance for log; under variance="mle" the trace does not fall beyond that allowance"""
    from dags_vae_search_amd import gaussian_em_fit, gaussian_sample
    n = 5
    x = gaussian_sample(_fitted([gp.LOOP_NET]), gi.EM_ROWS, seed=gi.EM_SEED).cpu().numpy()
    masks = gi.em_masks(gi.EM_ROWS, n, 0.2, gi.EM_MASK_SEED)
    assert 0.15 < 1 - np.mean([bin(int(m)).count("1") for m in masks]) / n < 0.25
    data, order = _pair(x, masks), gi.sorted_order(masks)
    for variance in ("mle", "unbiased"):
        fit = gaussian_em_fit(gp.LOOP_NET.parents, data, variance=variance, max_iter=1).fitted
        trace, allow = [], []
        for step in range(gi.EM_STEPS):
            before = _net_of(fit)
            em = gaussian_em_fit(gp.LOOP_NET.parents, data, start=fit, variance=variance, max_iter=1)
            want, ll, res = gi.restated_em_step(before, x, masks, variance)
            fit = em.fitted
            assert _bytes(fit.coef) == want.coef.tobytes() and _bytes(fit.intercept) == want.intercept.tobytes(), (variance, step)
            assert _bytes(fit.sd) == want.sd.tobytes(), (variance, step)
            bounds = gi.build_bound(res)
            ob = gp.out_bound_between_builds(res.logp[order], bounds)
            assert abs(em.log_likelihood[0] - ll) <= ob, (variance, step, em.log_likelihood[0], ll, ob)
            trace.append(em.log_likelihood[0])
            allow.append(ob)
        if variance == "mle":
            assert all(trace[t] >= trace[t - 1] - (allow[t] + allow[t - 1]) for t in range(1, len(trace))), trace
            whole = gaussian_em_fit(gp.LOOP_NET.parents, data, variance="mle", max_iter=gi.EM_STEPS + 1, tol=0.0)
            assert whole.log_likelihood[1:] == trace and _bytes(whole.fitted.sd) == _bytes(fit.sd)
            stop = gaussian_em_fit(gp.LOOP_NET.parents, data, max_iter=60, tol=1e-4)
            assert stop.converged and 1 < stop.iterations < 60


def test_em_meets_the_closed_form_when_one_variable_is_missing_at_random():
    from dags_vae_search_amd import gaussian_em_fit
    x, masks = gi.closed_form_case()
    data, f = _pair(x, masks), None
    for _ in range(gi.CLOSED_ITERATIONS):                    # one step a call: the stopping rule ends a run whose trace repeats
        f = gaussian_em_fit(gi.CLOSED_NET.parents, data, start=f, max_iter=1).fitted
    part = gi.assert_meets_closed_form(f.coef[0].cpu().numpy(), f.intercept[0].cpu().numpy(), f.sd[0].cpu().numpy(), x, masks, "device")
    print(f"distance to the closed form / tolerance {part:.3e}")


def test_the_loop_closes_on_the_device_with_a_tenth_of_the_cells_missing():
    """EM under the complete DAG -> expected moments -> exact_search under bge -> the generator's CPDAG (SHD 0), at the setting at
    which the restatement alone does so on the CPU, with its gap asserted first"""
    import torch
    from dags_vae_search_amd import compare_structures, exact_search, expected_moments, gaussian_em_fit
    ref = gi.missing_loop_reference()
    assert ref.gap > 1.0 and ref.best_key == ref.truth
    x, masks = gi.missing_loop_case()
    data = _pair(np.array(x, copy=True), masks)
    em = gaussian_em_fit(gi.MISSING_LOOP_DAG, data, max_iter=gi.MISSING_LOOP_STEPS, tol=0.0)
    assert em.iterations == gi.MISSING_LOOP_STEPS
    found = exact_search(expected_moments(em.fitted, data).evaluator("bge"))
    learned = found.parents.reshape(1, 5)
    assert gc.cpdag_key([int(v) for v in learned.cpu().numpy().view(U64).ravel()]) == ref.truth
    cmp = compare_structures(learned, _fitted([gp.LOOP_NET]).parents, equivalence=True)
    assert int(cmp.shd[0]) == 0


def test_refusals():
    import torch
    from dags_vae_search_amd import (BNLearnWrapper, GaussianEvaluator, bn_fit, expected_moments, gaussian_condition, gaussian_em_fit,
                                     gaussian_impute, gaussian_incomplete_log_likelihood, gaussian_posterior, incomplete_real_rows)
    n = 5
    net = gp.NETS[("dag", n)]
    fitted = _fitted([net])
    x, masks = np.array(gp.rows_for(n, 64), copy=True), gi.masks_for(n, 64, "few")
    data = _pair(x, masks)
    disc = BNLearnWrapper("disc5", "bic", data=np.random.default_rng(3).integers(0, 3, (200, n)))
    table = bn_fit(disc, torch.zeros(1, n, dtype=torch.int64, device="cuda"))
    # a conditional Gaussian network and a mixed evaluator: one factor and three real columns
    from dags_vae_search_amd import FittedCGBN, GaussianMomentsEvaluator, MixedEvaluator, cg_sample
    cg = FittedCGBN.from_parameters([0, 1, 1, 0], [2, 0, 0, 0], [None, np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((1, 4))],
                                    [None, np.array([-3.0, 3.0]), np.array([2.5, -2.5]), np.array([0.5])],
                                    [None, np.array([1.0, 1.2]), np.array([0.9, 1.0]), np.array([1.0])], [np.array([[0.5, 0.5]]), None, None, None])
    mixed = MixedEvaluator.from_device("mixed4", "bic-cg", *cg_sample(cg, 64, seed=1), [2, 0, 0, 0])
    cyclic = _fitted([gp.malformed(net, "cycle")])
    # every function as (network, data[, index]); gaussian_em_fit takes the network as its start
    calls = {"gaussian_condition": gaussian_condition, "gaussian_impute": gaussian_impute,
             "gaussian_incomplete_log_likelihood": gaussian_incomplete_log_likelihood, "expected_moments": expected_moments,
             "gaussian_posterior": lambda f, d, *index: gaussian_posterior(f, 0, d, *index),
             "gaussian_em_fit": lambda f, d: gaussian_em_fit(net.parents, d, start=f, max_iter=1)}
    for name, fn in calls.items():
        with pytest.raises(ValueError, match=f"{name}: takes a FittedGBN, got a FittedBN: a discrete network's counterparts are exact_posterior"):
            fn(table, data)
        with pytest.raises(ValueError, match=f"{name}: takes a FittedGBN, got a FittedCGBN: incomplete mixed data is not built"):
            fn(cg, data)
        with pytest.raises(ValueError, match=f"{name}: data must be .* not an evaluator: discrete data goes to expected_counts, impute and em_fit"):
            fn(fitted, disc)
        with pytest.raises(ValueError, match=f"{name}: data must be .* not an evaluator: gaussian_log_likelihood and gaussian_predict take its complete rows"):
            fn(fitted, GaussianEvaluator("g", "bic-g", data=x))
        with pytest.raises(ValueError, match=f"{name}: data must be .* not an evaluator: incomplete mixed data is not built"):
            fn(fitted, mixed)
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(fitted, (data[0].cpu(), data[1].cpu()))
        with pytest.raises(ValueError, match=rf"{name}: x must be float64 / float32 \[S >= 1, 5\]"):
            fn(fitted, (data[0][:, :4].contiguous(), data[1]))
        with pytest.raises(ValueError, match=f"{name}: x must be float64 / float32"):
            fn(fitted, (data[0].long(), data[1]))
        with pytest.raises(ValueError, match=rf"{name}: observed must be int64 \[64\]"):
            fn(fitted, (data[0], data[1].int()))
        if name != "gaussian_em_fit":                        # it fits one structure and takes no index; a start of another structure is its refusal
            with pytest.raises(ValueError, match=f"{name}: index must be in"):
                fn(fitted, data, 1)
            with pytest.raises(ValueError, match=f"{name}: the structure has a cycle"):
                fn(cyclic, data)
    with pytest.raises(ValueError, match="gaussian_em_fit: start must be a FittedGBN of this one structure"):
        gaussian_em_fit(net.parents, data, start=cyclic, max_iter=1)
    with pytest.raises(ValueError, match=r"moments must be float64 \[1, 1 \+ n \+ n n\]"):
        GaussianMomentsEvaluator("none", "bic-g", torch.zeros(1, 0, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="got a FittedBN"):
        gaussian_posterior(table, 0, {1: 0.5})
    with pytest.raises(ValueError, match="targets must name variables"):
        gaussian_posterior(fitted, 5, {1: 0.5})
    with pytest.raises(ValueError, match="evidence names variable 7"):
        gaussian_posterior(fitted, 0, {7: 0.5})
    with pytest.raises(ValueError, match="order must be"):
        gaussian_condition(fitted, data, order="random")
    with pytest.raises(ValueError, match="must be a permutation"):
        gaussian_condition(fitted, data, order=torch.zeros(64, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="values must be a real array"):
        incomplete_real_rows(np.zeros((4, 3), np.int64))
    # a refused row is counted by gaussian_condition and raised, with its index, by what needs every row
    bad = masks.copy()
    bad[9] |= U64(1 << n)
    got = gaussian_condition(fitted, _pair(x, bad))
    assert int(got.refused) == 1 and bool(torch.isnan(got.completed[9]).all()) and not bool(torch.isnan(got.completed[8]).any())
    with pytest.raises(ValueError, match=r"expected_moments: refused rows \[9\]: the observed variables are collinear"):
        expected_moments(fitted, _pair(x, bad))
    with pytest.raises(ValueError, match=r"gaussian_em_fit: refused rows \[9\] \(iteration 0\)"):
        gaussian_em_fit(net.parents, _pair(x, bad), max_iter=2)
    with pytest.raises(ValueError, match=r"gaussian_posterior: refused evidence rows \[9\]"):
        gaussian_posterior(fitted, 0, _pair(x, bad))
    # what gaussian_em_fit checks itself
    with pytest.raises(ValueError, match="variance must be"):
        gaussian_em_fit(net.parents, data, variance="ml")
    with pytest.raises(ValueError, match="max_iter must be >= 1 and tol >= 0"):
        gaussian_em_fit(net.parents, data, max_iter=0)
    with pytest.raises(ValueError, match=r"x must be float64 / float32 \[S >= 1, 4\]"):
        gaussian_em_fit(net.parents[:4], data)
    with pytest.raises(ValueError, match="start must be a FittedGBN of this one structure"):
        gaussian_em_fit(net.parents, data, start=_fitted([gp.NETS[("batch", 3)]]))
    wide_x, over = np.array(gc.gauss_data(17, 389), copy=True), [0] * 17
    over[16] = (1 << 12) - 1
    with pytest.raises(ValueError, match=r"gaussian_em_fit: refused families \(structure, variable\): \[\[0, 16\]\] \(iteration 0\): collinear"):
        gaussian_em_fit(over, _pair(wide_x, np.full(389, (1 << 17) - 1, U64)), max_iter=1)
