"""CPU: the eighth companion header (include/dvs_gaussian_params.h) as the binding reads it, and the Python restatement of its
definitions (tests/gaussian_params_corpus.py) against exact references: mpmath for the quantile, the log-likelihood and the
exact conditional, rationals for the joint.  The emulator and GPU twins run the same corpus through the C ABI.

Apart from the header binding and the site list, the tests here check the oracle, not the library: they hold the restatement to
references it shares nothing with, and would pass without the kernels.  The tests that fail without the feature are the header
binding here and everything in the emulator and GPU files."""
import math

import mpmath as mp
import numpy as np
import pytest

from dags_vae_search_amd import _lib as dl
from tests import gaussian_corpus as gc
from tests import gaussian_params_corpus as gp


def test_header_binding():
    assert list(dl.GPAR_SIGNATURES) == ["dvs_gbn_joint", "dvs_gbn_quantiles", "dvs_gbn_sample_workspace_bytes", "dvs_gbn_sample",
                                        "dvs_gbn_loglik", "dvs_gbn_predict"]
    others = (dl.SIGNATURES, dl.EXT_SIGNATURES, dl.INC_SIGNATURES, dl.AVAIL_SIGNATURES, dl.LOCAL_SIGNATURES, dl.PERM_SIGNATURES,
              dl.GAUSS_SIGNATURES, dl.GCI_SIGNATURES)
    assert all(not set(dl.GPAR_SIGNATURES) & set(t) for t in others)
    assert len(dl.SIGNATURES) == 64 and dl.ABI_VERSION == 202 and len(dl.GAUSS_SIGNATURES) == 5 and len(dl.GCI_SIGNATURES) == 2
    assert dl.signature("dvs_gbn_predict") is dl.GPAR_SIGNATURES["dvs_gbn_predict"]
    assert [k for k, _ in dl.GPAR_SIGNATURES["dvs_gbn_sample"][1]] == [
        "n_vars", "n_rows", "parents", "coef", "intercept", "sd", "seed", "row_offset", "workspace", "workspace_bytes", "data_out",
        "status", "stream"]
    assert [k for k, _ in dl.GPAR_SIGNATURES["dvs_gbn_predict"][1]] == [
        "batch", "n_vars", "n_rows", "data", "parents", "coef", "intercept", "sd", "target", "mode", "pred", "var", "workspace",
        "workspace_bytes", "status", "stream"]
    assert dl.GBN_PREDICT_MODES == {"parents": 0, "exact": 1}
    with pytest.raises(KeyError, match="dvs_gaussian_params.h"):
        dl.signature("dvs_gbn_nothing")


def test_site_510_is_restated_as_the_oracle_restates_500():
    from oracle import rng
    for seed in (0, 5, (7 << 32) + 11):
        for g in (0, 1, 77, (1 << 32) - 1):
            key = gp.site_key(seed, gp.SITE, g)
            assert key == int(rng.site_key(seed, 510, g))
            assert all(gp.draw(key, e) == int(rng.draw(key, e)) for e in (0, 1, 94, 95))
    with open(dl.GPAR_HEADER.replace("include/dvs_gaussian_params.h", "dags_vae_search_amd/csrc/dvs_device.h")) as f:
        assert "DVS_SITE_GBN_SAMPLE = 510u" in f.read()


def test_quantile_restatement_against_mpmath():
    worst, points = gp.quantile_grid_error()
    print("restated quantile: largest relative error", {b: f"{worst[b]:.3e}" for b in gp.BRANCHES}, "points", points)
    for b in gp.BRANCHES:
        assert worst[b] <= gp.QUANTILE_RTOL[b], (b, worst[b])
        assert gp.QUANTILE_RTOL[b] <= 1.1 * gp.QUANTILE_MEASURED[b] + 1e-17 and worst[b] >= 0.9 * gp.QUANTILE_MEASURED[b], (b, worst[b])
        assert points[b] >= 100
    ks = gp.quantile_grid()
    assert {0, 1, gp.TWO52 - 1} <= set(ks)
    with mp.workdps(60):
        for k in (0, 1, gp.TWO52 - 1):                       # the reference's own round trip at the ends of the domain
            z, u = gp.exact_quantile(k), (mp.mpf(k) + mp.mpf(1) / 2) / gp.TWO52
            assert abs(mp.erfc(-z / mp.sqrt(2)) / 2 - u) / min(u, 1 - u) < mp.mpf(10) ** -50
    # both sides of the two thresholds are on the grid, and the branches change there
    lo, far = int(0.075 * gp.TWO52), int(math.exp(-25.0) * gp.TWO52)
    assert {gp.restated_quantile(lo + d)[1] for d in range(-3, 4)} == {0, 1}
    assert {gp.restated_quantile(far + d)[1] for d in range(-3, 4)} == {1, 2}
    assert math.isnan(gp.restated_quantile(gp.TWO52)[0])


def test_quantile_restatement_is_odd_as_bytes():
    for k in gp.quantile_grid():
        a, b = gp.restated_quantile(k)[0], gp.restated_quantile(gp.TWO52 - 1 - k)[0]
        assert np.float64(a).tobytes() == np.float64(-b).tobytes(), k


@pytest.mark.parametrize("key", gp.joint_cases())
def test_joint_restatement_against_exact_rationals(key):
    net = gp.NETS[key]
    mean, cov = gp.restated_joint(net)
    worst = gp.assert_joint(mean, cov, key, key)
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes()
    print(f"{key}: largest joint error / bound {worst:.3e}")


def test_malformed_networks_by_rule():
    net = gp.NETS[("dag", 5)]
    assert gp.net_status(net)[0] == 0 and gp.net_status(net)[1] != list(range(5))
    for rule, bit in gp.RULES.items():
        bad = gp.malformed(net, rule)
        assert gp.net_status(bad)[0] == bit, rule
        assert np.isnan(gp.restated_joint(bad)[1]).all()


@pytest.mark.parametrize("n, S", [(5, 257), (17, 64)])
def test_loglik_restatement_against_mpmath(n, S):
    key = ("batch", 1) if n == 5 else ("dag", 17)
    net, x = gp.NETS[key], gp.rows_for(n, S)
    terms, bounds = gp.loglik_reference(key, n, S)
    rest = gp.restated_loglik_rows(net, x)
    worst = 0.0
    for i in range(S):
        err = float(abs(mp.mpf(float(rest[i])) - terms[i]))
        assert err <= bounds[i], (i, err, bounds[i])
        worst = max(worst, err / bounds[i])
    with mp.workdps(gc.DPS):
        err = float(abs(mp.mpf(gp.stated_sum(rest)) - mp.fsum(terms)))
    assert err <= gp.out_bound([float(abs(t)) for t in terms], bounds, S)
    # the closed form through the joint: the sum of the row terms is the multivariate normal's log-density, row by row
    mean, cov = gp.exact_joint(key)
    with mp.workdps(gc.DPS):
        q = lambda f: mp.mpf(f.numerator) / mp.mpf(f.denominator)
        Sg = mp.matrix([[q(c) for c in row] for row in cov])
        d = mp.matrix([mp.mpf(float(x[0, v])) - q(mean[v]) for v in range(n)])
        dens = -(n * mp.log(2 * mp.pi) + mp.log(mp.det(Sg)) + (d.T * mp.lu_solve(Sg, d))[0]) / 2
        assert abs(dens - terms[0]) < mp.mpf(10) ** -40
    print(f"n {n} S {S}: largest row error / bound {worst:.3e}")


@pytest.mark.parametrize("n", gp.PREDICT_N)
def test_exact_prediction_restatement_against_the_conditioned_joint(n):
    key = ("hub", n)
    net, x = gp.NETS[key], gp.rows_for(n, 24)
    worst = 0.0
    for t in gp.sinks_and_sources(net):
        pred, var = gp.restated_predict(net, t, 1, x)
        for i in range(len(x)):
            want, wvar = gp.exact_conditional_row(key, t, x[i])
            bound, rel = gp.predict_bound(net, t, x[i])
            err = float(abs(mp.mpf(float(pred[i])) - want))
            assert err <= bound, (n, t, i, err, bound)
            worst = max(worst, err / bound)
        assert float(abs(mp.mpf(var) - wvar) / wvar) <= rel
        p0, v0 = gp.restated_predict(net, t, 0, x)
        assert v0 == float(net.sd[t]) ** 2 and p0[0] == gp.restated_mu(net, t, x[0])
    print(f"n {n}: largest mode 1 error / bound {worst:.3e}")


def test_sampler_restatement_moments_and_central_share():
    key, N = ("full", 5), 16384
    x, z, branch = gp.restated_sample(key, N, 1)
    central = ~branch.any(axis=1)
    assert central.mean() >= 0.25, central.mean()            # 0.85^5 = 0.44 expected
    mean, cov = gp.exact_joint(key)
    mean, cov = np.asarray([float(m) for m in mean]), np.asarray([[float(c) for c in r] for r in cov])
    got_mean, got_cov = x.mean(axis=0), np.cov(x.T, bias=True)
    worst = 0.0
    for i in range(5):
        worst = max(worst, abs(got_mean[i] - mean[i]) / math.sqrt(cov[i, i] / N))
        for j in range(5):
            se = math.sqrt((cov[i, i] * cov[j, j] + cov[i, j] ** 2) / N)
            worst = max(worst, abs(got_cov[i, j] - cov[i, j]) / se)
    assert worst <= 5.0, worst
    # the draws: 52 bits, both halves used, rows keyed by the global index
    ks = [gp.draw_k(1, g, v) for g in range(64) for v in range(5)]
    assert len(set(ks)) == len(ks) and max(ks) < gp.TWO52 and max(ks) > gp.TWO52 // 2 and any(k & 1 for k in ks)
    assert gp.restated_sample(key, 8, 1, row_offset=3)[0].tobytes() == x[3:11].tobytes()
    print(f"central rows {central.mean():.3f}, largest deviation {worst:.2f} standard errors")


def test_vectorised_restatements_equal_the_scalar_ones_as_bytes():
    for key, n in ((("batch", 1), 5), (("hub", 17), 17)):
        net, x = gp.NETS[key], gp.rows_for(n, 40)
        assert gp.restated_loglik_rows_fast(net, x)[0].tobytes() == gp.restated_loglik_rows(net, x).tobytes()
        for t in gp.sinks_and_sources(net) if n == 17 else (2,):
            for mode in (0, 1):
                fp, fv = gp.restated_predict_fast(net, t, mode, x)
                sp, sv = gp.restated_predict(net, t, mode, x)
                assert fp.tobytes() == sp.tobytes() and np.float64(fv).tobytes() == np.float64(sv).tobytes(), (key, t, mode)
    nets = gp.many_nets()
    assert [gp.net_status(nets[b])[0] for b in sorted(gp.MANY_BAD)] == [1, 64, 16]
    assert sum(1 for net in nets if gp.net_status(net)[0]) == 3


def test_a_quarter_of_the_sampler_cases_rows_are_central_at_five_variables():
    """what check_sample asserts on both back ends, on the restatement alone: the byte comparison is not vacuous at n = 5"""
    for n_rows in gp.SAMPLE_ROWS[1:]:
        branch = gp.restated_sample(gp.sample_key(5), n_rows, 77)[2]
        assert int((~branch.any(axis=1)).sum()) >= n_rows // 4, n_rows


def test_the_loop_closes_on_the_restatement():
    ref = gp.loop_reference()
    assert ref.n_dags == 29281
    assert ref.gap > 1.0, ref.gap
    assert ref.best_key == ref.truth
    print(f"closed loop on the CPU: best DAG {ref.best}, score {ref.score:.3f}, gap to the best other class {ref.gap:.3f}")
