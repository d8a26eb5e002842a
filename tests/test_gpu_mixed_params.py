"""GPU: a fitted conditional Gaussian network (csrc/dvs_mixed_params.h) through the raw calls with the cases, references and
checks of tests/mixed_params_corpus.py — shared with the emulator twin tests/test_emu_mixed_params.py — plus the Python
surface: FittedCGBN.from_parameters, cg_sample, cg_log_likelihood, cg_predict and cg_cross_validate against the raw calls and
their discrete halves, the closed loop sample -> fit, and the refusals."""
import functools

import numpy as np
import pytest

from tests import mixed_params_corpus as mc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
KEYS = ("small", "mid", "wide")


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_sample(key, S):
    central, worst = mc.check_sample(backend(), key, S)
    print(f"{key} rows {S}: {central} central rows equal as bytes, worst error / bound elsewhere {worst:.3e}")


def test_sample_cut_into_calls():
    mc.check_sample_cut(backend())


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_loglik(key, S):
    print(f"{key} S {S}: worst error / bound {mc.check_loglik(backend(), key, S):.3e}")


def test_loglik_two_chunks_in_a_slot():
    print(f"small S {mc.BIG_S}: worst error / bound {mc.check_loglik(backend(), 'small', mc.BIG_S):.3e}")


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_predict_real_targets(key, S):
    print(f"{key} S {S}: worst mode 1 error / bound {mc.check_predict_real(backend(), key, S):.3e}")


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS + ("kids",))
def test_predict_class(key, S):
    print(f"{key} S {S}: worst posterior error / bound {mc.check_predict_class(backend(), key, S):.3e}")


def test_all_continuous_networks_give_the_gaussian_entry_points_bytes():
    mc.check_all_continuous_identities(backend())


def test_malformed_networks():
    mc.check_malformed(backend())


def test_rows_that_meet_trouble():
    mc.check_row_trouble(backend())


# ---- the Python surface ---------------------------------------------------------------------------------------------------
def _bytes(t):
    return t.cpu().numpy().tobytes()


def _tables(net, seed=0):
    """a [q, r] table of positive rows that sum to 1 for every factor of the corpus network, None for a real column"""
    rng = np.random.default_rng(35000 + seed)
    out = []
    for v in range(net.n):
        if not net.card[v]:
            out.append(None)
            continue
        q = int(np.prod([net.card[u] for u in net.pa(v)], dtype=np.int64))
        t = rng.uniform(0.2, 1.0, (q, net.card[v]))
        out.append(t / t.sum(axis=1, keepdims=True))
    return out


@functools.lru_cache(maxsize=None)
def _fitted(key):
    from dags_vae_search_amd import FittedCGBN
    net = mc.net_of(key)
    per = lambda a: [a[int(net.offset[v]):int(net.offset[v + 1])] if not net.card[v] else None for v in range(net.n)]
    return FittedCGBN.from_parameters(net.parents, net.card, per(net.coef), per(net.intercept), per(net.sd), _tables(net))


def _device_rows(key, S):
    import torch
    _, packed, x = mc.rows_of(key, S)
    return torch.from_numpy(packed.view(np.int64).copy()).cuda(), torch.from_numpy(np.array(x)).cuda()


@pytest.mark.parametrize("key", ("small", "mid"))
def test_cg_sample_is_the_discrete_sample_and_the_raw_call(key):
    from dags_vae_search_amd import cg_sample
    from dags_vae_search_amd.params import sample
    f, net, S = _fitted(key), mc.net_of(key), 700
    packed, x = cg_sample(f, S, seed=91, row_offset=3)
    levels = mc.unpack(packed.cpu().numpy().view(np.uint64), net.n)
    sub = sample(f.discrete, S, seed=91, row_offset=3).cpu().numpy().view(np.uint64)
    dvars = [v for v in range(net.n) if net.card[v]]
    assert f.discrete_vars == dvars
    assert np.array_equal(levels[:, dvars], mc.unpack(sub, len(dvars)))
    assert not levels[:, net.cvars].any()                    # the nibbles of the real columns are zero
    raw, st = mc.run_sample(backend(), net, packed.cpu().numpy().view(np.uint64), 91, row_offset=3)
    assert st == 0 and _bytes(x) == raw.tobytes()
    cut = [cg_sample(f, m, seed=91, row_offset=3 + at) for at, m in ((0, 300), (300, 400))]
    assert _bytes(packed) == b"".join(_bytes(p) for p, _ in cut) and _bytes(x) == b"".join(_bytes(c) for _, c in cut)


@pytest.mark.parametrize("key", ("small", "mid"))
def test_cg_log_likelihood_is_one_addition_of_the_two_halves(key):
    import torch
    from dags_vae_search_amd import MixedEvaluator, cg_log_likelihood
    from dags_vae_search_amd.mixed import _sub_rows
    from dags_vae_search_amd.params import log_likelihood
    f, net, S = _fitted(key), mc.net_of(key), 700
    packed, x = _device_rows(key, S)
    out, rows = cg_log_likelihood(f, (packed, x), per_row=True)
    d_out, d_rows = log_likelihood(f.discrete, _sub_rows(packed, f.discrete_vars), per_row=True)
    c_out, c_rows, st = mc.run_loglik(backend(), net, mc.rows_of(key, S)[1], mc.rows_of(key, S)[2])
    assert st == 0
    assert _bytes(out) == np.float64(d_out[0].item() + c_out).tobytes()
    assert _bytes(rows) == (d_rows[0].cpu().numpy() + c_rows).tobytes()
    ev = MixedEvaluator.from_device("rows", "loglik-cg", packed, x, net.card)
    assert _bytes(cg_log_likelihood(f, ev)) == _bytes(out)
    assert torch.isfinite(out)


@pytest.mark.parametrize("key", ("small", "mid"))
def test_cg_predict_equals_the_raw_calls(key):
    from dags_vae_search_amd import cg_predict, infer
    from dags_vae_search_amd.mixed import _sub_rows
    f, net, S = _fitted(key), mc.net_of(key), 700
    packed, x = _device_rows(key, S)
    _, hp, hx = mc.rows_of(key, S)
    for t in mc.real_targets(key):
        for mode, method in ((0, "parents"), (1, "exact")):
            pred, var = cg_predict(f, t, (packed, x), method=method, var=True)
            rp, rv, st = mc.run_predict(backend(), net, hp, hx, t, mode)
            assert st == 0 and _bytes(pred) == rp.tobytes() and _bytes(var) == rv.tobytes(), (t, mode)
            assert _bytes(cg_predict(f, t, (packed, x), method=method)) == rp.tobytes()
    sub = _sub_rows(packed, f.discrete_vars)
    for t in mc.class_targets(key):
        rank = f.discrete_vars.index(t)
        want, prior = infer.predict(f.discrete, rank, sub, method="exact", prob=True)
        pred, post = cg_predict(f, t, (packed, x), method="exact", prob=True)
        if any(t in net.pa(c) for c in net.cvars):
            rp, rpost, st = mc.run_predict(backend(), net, hp, hx, t, 2, prior.cpu().numpy())
            assert st == 0 and _bytes(pred) == rp.tobytes() and _bytes(post) == rpost.tobytes(), t
        else:                                                # no real children: the sub-network's answer as it is
            assert _bytes(pred) == _bytes(want) and _bytes(post) == _bytes(prior), t
        par = infer.predict(f.discrete, rank, sub, method="parents")
        assert _bytes(cg_predict(f, t, (packed, x), method="parents")) == _bytes(par)


def test_sampled_rows_fitted_with_the_true_structure_recover_the_parameters():
    """20 000 rows of the small network: every regression of cg_fit lies within 5 standard errors of the hand-written
    parameters; the standard errors are sd^2 (X^T X)^-1 of the configuration's rows (known sd) and sd / sqrt(2 (m - p - 1))"""
    import torch
    from dags_vae_search_amd import MixedEvaluator, cg_fit, cg_sample
    f, net, S = _fitted("small"), mc.net_of("small"), 20000
    packed, x = cg_sample(f, S, seed=2024)
    ev = MixedEvaluator.from_device("loop", "bic-cg", packed, x, net.card)
    got = cg_fit(ev, torch.tensor(net.parents, dtype=torch.int64, device="cuda"))
    lev = mc.unpack(packed.cpu().numpy().view(np.uint64), net.n)
    xf = mc.full(net, x.cpu().numpy())
    for v in net.cvars:
        cell, _ = mc.cells_of(net, v, lev)
        pa = net.cpa(v)
        for z in range(net.q(v)):
            c = int(net.offset[v]) + z
            mine = cell == c
            m, sd = int(mine.sum()), float(net.sd[c])
            assert m >= 1000 and float(got.count[v][z]) == m
            X = np.column_stack([np.ones(m)] + [xf[mine, u] for u in pa])
            se = sd * np.sqrt(np.diag(np.linalg.inv(X.T @ X)))
            assert abs(float(got.intercept[v][z]) - net.intercept[c]) <= 5 * se[0], (v, z)
            for j, u in enumerate(pa):
                assert abs(float(got.coef[v][z, u]) - net.coef[c, u]) <= 5 * se[j + 1], (v, z, u)
            assert abs(float(got.sd[v][z]) - sd) <= 5 * sd / np.sqrt(2 * (m - len(pa) - 1)), (v, z)
    assert _bytes(got.coef_flat) == b"".join(_bytes(got.coef[v]) for v in net.cvars)


def _class_network():
    """a class with two well-separated real children and a real that is no child: [class, child, child, other]"""
    from dags_vae_search_amd import FittedCGBN
    coef = [None, np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((1, 4))]
    icpt = [None, np.array([-3.0, 3.0]), np.array([2.5, -2.5]), np.array([0.5])]
    sd = [None, np.array([1.0, 1.2]), np.array([0.9, 1.0]), np.array([1.0])]
    return FittedCGBN.from_parameters([0, 1, 1, 0], [2, 0, 0, 0], coef, icpt, sd, [np.array([[0.5, 0.5]]), None, None, None])


@pytest.mark.parametrize("loss,target", (("logl-cg", None), ("mse", 1), ("mse-exact", 3), ("pred", 0), ("pred-exact", 0)))
def test_cg_cross_validate_is_its_composition(loss, target):
    import torch
    from dags_vae_search_amd import MixedEvaluator, cg_cross_validate, cg_fit, cg_log_likelihood, cg_predict, cg_sample
    from dags_vae_search_amd.params import cv_folds
    f = _class_network()
    packed, x = cg_sample(f, 2000, seed=7)
    ev = MixedEvaluator.from_device("cv", "bic-cg", packed, x, f.card)
    got = cg_cross_validate(ev, f.parents, folds=5, seed=3, loss=loss, target=target)
    parts = [torch.from_numpy(p).cuda() for p in cv_folds(2000, 5, 3)]
    total = None
    for i, part in enumerate(parts):
        rest = torch.cat([p for g, p in enumerate(parts) if g != i])
        fit = cg_fit(MixedEvaluator.from_device("cv", "bic-cg", packed[rest], x[rest], f.card), f.parents)
        held = (packed[part].contiguous(), x[part].contiguous())
        if loss == "logl-cg":
            value = cg_log_likelihood(fit, held)
        else:
            pred = cg_predict(fit, target, held, method="exact" if loss.endswith("exact") else "parents")
            if loss.startswith("mse"):
                err = pred - held[1][:, target - 1]
                value = (err * err).sum()
            else:
                value = (pred != (held[0][:, 0] & 15).to(torch.uint8)).sum().to(torch.float64)
        total = value if total is None else total + value
    want = (-total if loss == "logl-cg" else total) / torch.full_like(total, 2000.0)
    assert _bytes(got) == _bytes(want) and torch.isfinite(got)


def test_pred_exact_beats_pred_when_the_class_drives_its_children():
    from dags_vae_search_amd import MixedEvaluator, cg_cross_validate, cg_sample
    f = _class_network()
    packed, x = cg_sample(f, 2000, seed=8)
    ev = MixedEvaluator.from_device("cv", "bic-cg", packed, x, f.card)
    plain = float(cg_cross_validate(ev, f.parents, folds=5, seed=1, loss="pred", target=0))
    exact = float(cg_cross_validate(ev, f.parents, folds=5, seed=1, loss="pred-exact", target=0))
    print(f"pred {plain:.4f}  pred-exact {exact:.4f}")
    assert exact < 0.05 < 0.3 < plain


def test_refusals_name_the_rule():
    import torch
    from dags_vae_search_amd import FittedCGBN, MixedEvaluator, cg_log_likelihood, cg_predict, cg_sample
    from dags_vae_search_amd.gaussian import gaussian_fit
    from dags_vae_search_amd.params import bn_fit, cross_validate
    net = mc.net_of("small")
    per = lambda a: [a[int(net.offset[v]):int(net.offset[v + 1])] if not net.card[v] else None for v in range(net.n)]
    args = lambda **kw: {**dict(parents=net.parents, card=net.card, coef=per(net.coef), intercept=per(net.intercept), sd=per(net.sd),
                                tables=_tables(net)), **kw}
    cyc = list(net.parents)
    cyc[3] |= 1 << 4
    bad_sd = per(net.sd.copy())
    bad_sd[1] = np.array([1.0, 0.0, 1.0])
    for kw, text in ((dict(parents=cyc), "cycle"), (dict(parents=[1 << 3] + list(net.parents[1:])), "continuous parent"),
                     (dict(parents=[1 << 5] + list(net.parents[1:])), "parent bit"), (dict(sd=bad_sd), "sd is not > 0")):
        with pytest.raises(ValueError, match=text):
            FittedCGBN.from_parameters(**args(**kw))
    # the same rules on the device: a network whose fields were put together by hand
    f = _fitted("small")
    broken = FittedCGBN(f.parents.clone(), f.kind, f.card, f.coef, f.intercept, f.sd, f.count, f.discrete, f.discrete_vars)
    broken.parents[3] |= 1 << 4
    with pytest.raises(ValueError, match="cycle"):
        cg_sample(broken, 10, seed=1)
    packed, x = _device_rows("small", 300)
    with pytest.raises(ValueError, match="cycle"):
        cg_log_likelihood(broken, (packed, x))
    nosd = FittedCGBN(f.parents, f.kind, f.card, f.coef, f.intercept, [None if s is None else s * 0 for s in f.sd], f.count, f.discrete,
                      f.discrete_vars)
    with pytest.raises(ValueError, match="not > 0"):
        cg_predict(nosd, 4, (packed, x))
    high = packed.clone()
    high[11] |= 5 << 8                                       # factor 2 has two levels
    with pytest.raises(ValueError, match="level code"):
        cg_log_likelihood(f, (high, x))
    with pytest.raises(ValueError, match="prob is the argument"):
        cg_predict(f, 4, (packed, x), prob=True)
    # what was refused on mixed data before still is
    ev = MixedEvaluator.from_device("rows", "bic-cg", packed, x, net.card)
    P = torch.tensor(net.parents, dtype=torch.int64, device="cuda")
    for fn in (lambda: cross_validate(ev, P[None]), lambda: bn_fit(ev, P), lambda: gaussian_fit(ev, P[None])):
        with pytest.raises(ValueError, match="mixed data"):
            fn()


def test_the_tie_to_the_scorer():
    """cg_log_likelihood(cg_fit(ev, P), ev) is ev.score_masks(P) under loglik-cg: RSS_z / s2_z = dof_z in every configuration
    and the tables are the MLE tables.  The bound is the sum of the two sides', from the inputs alone:
      scorer    LL_z = -(m_z / 2) log(2 pi s2_z) - dof_z / 2: s2_z comes from moments summed over m_z rows and a Cholesky of p + 1
                columns, relative error kappa_z gamma(m_z + 3 (p + 2) + 4), kappa_z the condition number of the configuration's
                covariance of (parents, v), computed here from the rows; times m_z / 2, plus 4 u |LL_z|.
      this side the fitted sd carries the same relative error and dLL_z / dlog(sd) = -(p + 1) <= m_z / 2 (the coefficients are
                at a stationary point: second order), so the same term again; evaluating the rows adds gamma(4 (p + 2) + 56)
                on the sum of |row terms| (mu, the residual, the square, c, two additions, the two trees).
      factors   both sides sum N_jk log(N_jk / N_j) in their own order: 2 gamma(S + 8) on |the discrete total|."""
    import torch
    from dags_vae_search_amd import MixedEvaluator, cg_fit, cg_log_likelihood, cg_sample
    from dags_vae_search_amd.mixed import _sub_rows
    from dags_vae_search_amd.params import log_likelihood
    f, net, S = _fitted("small"), mc.net_of("small"), 4000
    packed, x = cg_sample(f, S, seed=11)
    ev = MixedEvaluator.from_device("tie", "loglik-cg", packed, x, net.card)
    P = torch.tensor(net.parents, dtype=torch.int64, device="cuda")
    fit = cg_fit(ev, P)
    out, rows = cg_log_likelihood(fit, ev, per_row=True)
    d_out, d_rows = log_likelihood(fit.discrete, _sub_rows(packed, fit.discrete_vars), per_row=True)
    score = ev.score_masks(P[None])[0]
    lev, xf = mc.unpack(packed.cpu().numpy().view(np.uint64), net.n), mc.full(net, x.cpu().numpy())
    c_rows = (rows - d_rows[0]).abs().sum().item() + 2.0 ** -52 * rows.abs().sum().item()
    pmax = max(len(net.cpa(v)) for v in net.cvars)
    bound = mc.gamma(4 * (pmax + 2) + 56) * c_rows + 2 * mc.gamma(S + 8) * abs(d_out[0].item())
    for v in net.cvars:
        cell, _ = mc.cells_of(net, v, lev)
        cols = net.cpa(v) + [v]
        for z in range(net.q(v)):
            mine = cell == int(net.offset[v]) + z
            m = int(mine.sum())
            assert m >= 4 * (len(cols) + 1), (v, z, m)
            kappa = float(np.linalg.cond(np.atleast_2d(np.cov(xf[mine][:, cols], rowvar=False))))
            sd = float(fit.sd[v][z])
            ll_z = abs(-(m / 2) * np.log(2 * np.pi * sd * sd) - (m - len(cols)) / 2)
            bound += 2 * (m / 2) * kappa * mc.gamma(m + 3 * (len(cols) + 1) + 4) + 4 * mc.U * ll_z
    print(f"loglik {float(out):.6f} score {float(score):.6f} difference {abs(float(out) - float(score)):.3e} bound {bound:.3e}")
    assert abs(float(out) - float(score)) <= bound
