"""GPU: a fitted Gaussian network (csrc/dvs_gaussian_params.h) through the raw calls with the cases, references and checks of
tests/gaussian_params_corpus.py — shared with the emulator twin tests/test_emu_gaussian_params.py — plus the Python surface:
gaussian_joint, gaussian_sample, gaussian_log_likelihood, gaussian_predict and gaussian_cross_validate, the closed loop
sample -> learn -> compare, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

from tests import gaussian_corpus as gc
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


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
def test_quantiles():
    print(gp.check_quantiles(backend()))


@pytest.mark.parametrize("n", gp.N_VALUES)
def test_joint_equals_the_restatement(n):
    gp.check_joint(backend(), n)


@pytest.mark.parametrize("n_rows", gp.SAMPLE_ROWS)
@pytest.mark.parametrize("n", gp.N_VALUES)
def test_sample(n, n_rows):
    central, worst = gp.check_sample(backend(), n, n_rows)
    print(f"n {n} rows {n_rows}: {central} central rows equal as bytes, worst error / bound elsewhere {worst:.3e}")


def test_sample_cut_into_calls():
    gp.check_sample_cut(backend())


def test_sample_refusals_leave_the_output_untouched():
    gp.check_sample_refusals(backend())


@pytest.mark.parametrize("S", gp.LOGLIK_S)
@pytest.mark.parametrize("B", gp.LOGLIK_B)
def test_loglik(B, S):
    print(f"B {B} S {S}: worst error / bound {gp.check_loglik(backend(), B, S):.3e}")


def test_loglik_two_chunks_in_a_slot():
    gp.check_loglik_two_chunks_in_a_slot(backend())


def test_loglik_many_structures_per_workgroup():
    print(f"B {gp.MANY_B} S {gp.MANY_S}: worst error / bound {gp.check_loglik_many_structures_per_workgroup(backend()):.3e}")


def test_predict_many_structures_per_workgroup():
    gp.check_predict_many_structures_per_workgroup(backend())


@pytest.mark.parametrize("n", (17, 48))
def test_loglik_wide(n):
    print(f"n {n}: worst error / bound {gp.check_loglik_wide(backend(), n):.3e}")


def test_loglik_malformed_between_neighbours():
    gp.check_loglik_malformed(backend())


@pytest.mark.parametrize("n", gp.PREDICT_N)
def test_predict(n):
    print(f"n {n}: worst mode 1 error / bound {gp.check_predict(backend(), n):.3e}")


def test_predict_malformed_between_neighbours():
    gp.check_predict_malformed(backend())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    gp.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_python_functions_equal_the_raw_calls():
    import torch
    from dags_vae_search_amd import (GaussianEvaluator, gaussian_joint, gaussian_log_likelihood, gaussian_predict, gaussian_sample)
    be, n, S = backend(), 17, 300
    nets = [gp.NETS[("hub", n)], gp.NETS[("dag", n)], gp.NETS[("full", n)]]
    fitted, x = _fitted(nets), np.array(gp.rows_for(n, S))
    assert (fitted.batch, fitted.n_vars, fitted.device.type) == (3, n, "cuda")
    mean, cov = gaussian_joint(fitted)
    m, c, _ = gp.run_joint(be, nets)
    assert _bytes(mean) == m.tobytes() and _bytes(cov) == c.tobytes()
    rows = gaussian_sample(fitted, 300, seed=9, row_offset=4, index=2)
    assert _bytes(rows) == gp.run_sample(be, nets[2], 300, 9, row_offset=4)[0].tobytes()
    assert _bytes(torch.cat([gaussian_sample(fitted, 100, seed=9, row_offset=4, index=2),
                             gaussian_sample(fitted, 200, seed=9, row_offset=104, index=2)])) == _bytes(rows)
    xd = torch.from_numpy(x).cuda()
    out, per = gaussian_log_likelihood(fitted, xd, per_row=True)
    o, r, _ = gp.run_loglik(be, nets, x)
    assert _bytes(out) == o.tobytes() and _bytes(per) == r.tobytes() and _bytes(gaussian_log_likelihood(fitted, xd)) == o.tobytes()
    ev = GaussianEvaluator("held", "bic-g", data=x)
    assert _bytes(gaussian_log_likelihood(fitted, ev)) == o.tobytes()
    x32 = x.astype(np.float32)
    assert _bytes(gaussian_log_likelihood(fitted, torch.from_numpy(x32).cuda())) == gp.run_loglik(be, nets, x32.astype(np.float64))[0].tobytes()
    for method, mode in (("parents", 0), ("exact", 1)):
        pred, var = gaussian_predict(fitted, 5, xd, method=method, var=True)
        p, v, _ = gp.run_predict(be, nets, x, 5, mode)
        assert _bytes(pred) == p.tobytes() and _bytes(var) == v.tobytes() and _bytes(gaussian_predict(fitted, 5, ev, method=method)) == p.tobytes()
    # the rows of a sample feed an evaluator with no host round trip, and the fit of the generator on them is near it
    big = gaussian_sample(fitted, 20000, seed=3, index=1)
    from dags_vae_search_amd import gaussian_fit
    back = gaussian_fit(GaussianEvaluator.from_device("sampled", "bic-g", big), fitted.parents[1])
    assert float((back.sd[0] / fitted.sd[1] - 1).abs().max()) < 6 / np.sqrt(2 * 20000)      # sd^ / sd - 1 has s.e. 1 / sqrt(2 m)


def test_the_loop_closes_on_the_device():
    """sample -> from_device -> exact_search -> compare_structures: the SHD of the CPDAGs is 0, as the restatement alone (the
    restated rows, the restated bge scores, all 29 281 DAGs) says it must be, with its gap asserted first"""
    import torch
    from dags_vae_search_amd import GaussianEvaluator, compare_structures, exact_search, gaussian_sample
    ref = gp.loop_reference()
    assert ref.gap > 1.0 and ref.best_key == ref.truth
    fitted = _fitted([gp.LOOP_NET])
    rows = gaussian_sample(fitted, gp.LOOP_ROWS, seed=gp.LOOP_SEED)
    central = ~gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[2].any(axis=1)
    assert rows.cpu().numpy()[central].tobytes() == ref.x[central].tobytes()
    ev = GaussianEvaluator.from_device("loop", "bge", rows)
    found = exact_search(ev)
    learned = found.parents.reshape(1, 5)
    assert gc.cpdag_key([int(v) for v in learned.cpu().numpy().view(U64).ravel()]) == ref.truth
    cmp = compare_structures(learned, fitted.parents, equivalence=True)
    assert int(cmp.shd[0]) == 0


@pytest.mark.parametrize("folds", (2, 3))
def test_cross_validation_equals_the_per_fold_composition_as_bytes(folds):
    import torch
    from dags_vae_search_amd import (GaussianEvaluator, cv_folds, gaussian_cross_validate, gaussian_fit, gaussian_log_likelihood)
    n, S = 5, 389
    x = torch.from_numpy(gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[0][:S].copy()).cuda()
    ev = GaussianEvaluator.from_device("cv", "bic-g", x)
    parents = torch.from_numpy(np.asarray([gp.LOOP_NET.parents, [0] * n, gp.NETS[("batch", 3)].parents], U64).view(np.int64)).cuda()
    got = gaussian_cross_validate(ev, parents, folds=folds, seed=4)
    parts = [torch.from_numpy(p).cuda() for p in cv_folds(S, folds, 4)]
    assert len({len(p) for p in parts}) == (1 if S % folds == 0 else 2)
    total = None
    for f, part in enumerate(parts):
        rest = torch.cat([p for g, p in enumerate(parts) if g != f])
        fit = gaussian_fit(GaussianEvaluator.from_device("rest", "bic-g", x[rest]), parents)
        ll = gaussian_log_likelihood(fit, x[part])
        total = ll if total is None else total + ll
    assert _bytes(got) == _bytes(-total / S)
    assert got.shape == (3,) and bool(torch.isfinite(got).all())


def test_losses_rank_the_generator_first():
    import torch
    from dags_vae_search_amd import GaussianEvaluator, gaussian_cross_validate
    n = 5
    x = torch.from_numpy(gp.restated_sample(("loop", 5), gp.LOOP_ROWS, gp.LOOP_SEED)[0].copy()).cuda()
    ev = GaussianEvaluator.from_device("cv", "bic-g", x)
    parents = torch.from_numpy(np.asarray([gp.LOOP_NET.parents, [0] * n], U64).view(np.int64)).cuda()
    logl = gaussian_cross_validate(ev, parents)
    assert float(logl[0]) < float(logl[1])
    mse = gaussian_cross_validate(ev, parents[:1], loss="mse", target=2)
    exact = gaussian_cross_validate(ev, parents[:1], loss="mse-exact", target=2)          # 2 has the children 3 and 4
    assert float(exact[0]) <= float(mse[0]) and float(exact[0]) > 0
    # a family the fit refuses on a fold names the fold: 12 parents are over the cap whatever the rows
    wide = GaussianEvaluator("wide", "bic-g", data=gc.gauss_data(17, 389))
    over = torch.zeros(1, 17, dtype=torch.int64, device="cuda")
    over[0, 16] = (1 << 12) - 1
    with pytest.raises(ValueError, match=r"gaussian_cross_validate: refused families \(fold, structure, variable\): \[\(\d, 0, 16\)"):
        gaussian_cross_validate(wide, over, folds=3)


def test_refusals():
    import torch
    from dags_vae_search_amd import (BNLearnWrapper, FittedGBN, GaussianEvaluator, bn_fit, gaussian_cross_validate, gaussian_fit,
                                     gaussian_joint, gaussian_log_likelihood, gaussian_predict, gaussian_sample)
    n = 5
    fitted = _fitted([gp.NETS[("dag", n)]])
    rng = np.random.default_rng(3)
    disc = BNLearnWrapper("disc5", "bic", data=rng.integers(0, 3, (200, n)))
    empty = torch.zeros(1, n, dtype=torch.int64, device="cuda")
    table = bn_fit(disc, empty)
    # a discrete evaluator, or a discrete network, is refused by every new function
    for fn in (lambda: gaussian_log_likelihood(fitted, disc), lambda: gaussian_predict(fitted, 0, disc),
               lambda: gaussian_cross_validate(disc, empty), lambda: gaussian_joint(table), lambda: gaussian_sample(table, 4, seed=0),
               lambda: gaussian_log_likelihood(table, disc), lambda: gaussian_predict(table, 0, disc)):
        with pytest.raises(ValueError, match="discrete"):
            fn()
    # a status bit says which rule
    rules = (("cycle", "has a cycle"), ("bit", "at or above the number of variables"), ("sd0", "not finite, or an sd is not > 0"))
    for rule, text in rules:
        bad = _fitted([gp.malformed(gp.NETS[("dag", n)], rule)])
        for fn in (lambda: gaussian_joint(bad), lambda: gaussian_sample(bad, 4, seed=0),
                   lambda: gaussian_log_likelihood(bad, torch.zeros(3, n, dtype=torch.float64, device="cuda")),
                   lambda: gaussian_predict(bad, 1, torch.zeros(3, n, dtype=torch.float64, device="cuda"))):
            with pytest.raises(ValueError, match=text) as err:
                fn()
            assert sum(t in str(err.value) for _, t in rules) == 1          # that rule and no other
    sound = gp.NETS[("dag", n)]
    mixed = _fitted([sound, gp.malformed(sound, "cycle"), sound, gp.malformed(sound, "cycle")])
    with pytest.raises(ValueError, match=r"gaussian_log_likelihood: malformed structures \[1, 3\]: the structure has a cycle$"):
        gaussian_log_likelihood(mixed, torch.zeros(3, n, dtype=torch.float64, device="cuda"))
    # no CUDA: the package's usual RuntimeError
    host = FittedGBN(fitted.parents.cpu(), fitted.coef.cpu(), fitted.intercept.cpu(), fitted.sd.cpu())
    for fn in (lambda: gaussian_joint(host), lambda: gaussian_sample(host, 4, seed=0),
               lambda: gaussian_log_likelihood(fitted, torch.zeros(3, n, dtype=torch.float64))):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn()
    ev = GaussianEvaluator("g", "bic-g", data=gc.gauss_data(n, 129))
    with pytest.raises(ValueError, match="folds must be in"):
        gaussian_cross_validate(ev, empty, folds=1)
    with pytest.raises(ValueError, match="loss must be one of"):
        gaussian_cross_validate(ev, empty, loss="logl")
    with pytest.raises(ValueError, match="target is the argument"):
        gaussian_cross_validate(ev, empty, loss="mse")
    with pytest.raises(ValueError, match="method must be one of"):
        gaussian_predict(fitted, 0, ev, method="bayes-lw")
    with pytest.raises(ValueError, match="index must be in"):
        gaussian_sample(fitted, 4, seed=0, index=1)
    assert gaussian_fit(ev, empty).batch == 1
