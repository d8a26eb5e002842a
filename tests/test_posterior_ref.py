"""CPU pins of the references of tests/posterior_corpus.py, before any kernel is trusted against them: ref_dp (numpy,
np.logaddexp) against brute force over every labelled DAG weighted by its linear extensions (ref_brute, mpmath, n <= 5) and
against the mpmath restatement of the programme with exact products (ref_mp, n = 6 and 7); the closed form of the all-zero
table; and the bound itself at the scale the derivation was measured at."""
import math

import numpy as np
import pytest

from tests import exact_corpus as ex
from tests import posterior_corpus as po


def test_linear_extension_counts():
    assert [len(ex.dag_rows(n)) for n in (1, 2, 3, 4)] == [1, 3, 25, 543]
    for n in (1, 2, 3, 4, 5):
        D, ext = ex.dag_rows(n), po.linear_extensions(n)
        assert ext[(D == 0).all(1)].tolist() == [math.factorial(n)]             # the empty graph: every order
        assert ext.min() == 1 and int(ext.sum()) == math.factorial(n) * 2 ** (n * (n - 1) // 2)     # (order, subgraph) pairs


@pytest.mark.parametrize("kind", po.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_ref_dp_equals_brute_force_over_all_dags(n, kind):
    tables, cap, forb, prior, refs = po.brute_case(n, kind)
    for t in range(po.BRUTE_BATCH):
        ref = po.ref_dp(tables[t], cap, forb, prior)
        eps = po.eps_of(ref.f)
        assert ref.flag == 0 == refs[t].flag
        po.assert_close(ref.log_z, refs[t].log_z, eps, "log_z")
        po.assert_close(ref.log_z_back, refs[t].log_z, eps, "log_z_back")
        po.assert_close(ref.prob, refs[t].prob, po.prob_tol(eps, n), "prob")
        po.assert_close(ref.family, refs[t].family, po.prob_tol(eps, n), "family")
        assert abs(refs[t].family.sum(0) - 1.0).max() <= 1e-15 * (1 << n)


def test_ref_brute_with_a_nan_cell_and_a_forbidden_arc():
    """n = 4, one NaN cell and one forbidden arc: the filtered enumeration and the programme agree, the arc is exactly 0"""
    table = po.make_tables("random", 1, 4, seed=9)[0]
    table[0b0101, 1] = np.nan
    forb = np.zeros(4, np.uint64)
    forb[3] = np.uint64(0b0100)                                                  # 2 -> 3 is barred
    brute, ref = po.ref_brute(table, None, forb), po.ref_dp(table, None, forb)
    eps = po.eps_of(ref.f)
    po.assert_close(ref.log_z, brute.log_z, eps, "log_z")
    po.assert_close(ref.prob, brute.prob, po.prob_tol(eps, 4), "prob")
    assert ref.prob[2, 3] == 0.0 == brute.prob[2, 3] and ref.family[0b0101, 1] == 0.0 == brute.family[0b0101, 1]


@pytest.mark.parametrize("n,scale", [(6, 3.0), (7, 3.0), (7, 300.0)])
def test_ref_dp_equals_the_mpmath_programme(n, scale):
    table = po.make_tables("nan", 1, n, seed=n, scale=scale)[0]
    cap, forb, prior = 4, ex.random_forbidden(np.random.default_rng(n), n, 0.1), np.linspace(0.5, -1.0, n)
    ref, mp = po.ref_dp(table, cap, forb, prior), po.ref_mp(table, cap, forb, prior)
    eps = po.eps_of(ref.f)
    worst = 0.0
    for name in ("L", "Rb", "gamma", "log_z", "log_z_back"):
        worst = max(worst, po.assert_close(getattr(ref, name), getattr(mp, name), eps, name))
    for name in ("prob", "family"):
        po.assert_close(getattr(ref, name), getattr(mp, name), po.prob_tol(eps, n), name)
    print(f"\nn {n} scale {scale}: ref_dp's worst log-domain error {worst:.3e} against eps {eps:.3e}")


@pytest.mark.parametrize("n", [1, 2, 6])
def test_ref_dp_on_the_all_zero_table(n):
    ref = po.ref_dp(np.zeros((1 << n, n)))
    log_z, p = po.closed_form(n, None)
    assert abs(ref.log_z - (math.lgamma(n + 1) + n * (n - 1) / 2 * math.log(2.0))) <= 1e-13 and abs(ref.log_z - log_z) <= 1e-13
    want = np.full((n, n), 0.25 if n > 1 else 0.0)
    np.fill_diagonal(want, 0.0)
    assert np.abs(ref.prob - want).max() <= 1e-14
    for cap in (1, 2):
        capped = po.ref_dp(np.zeros((1 << n, n)), cap)
        lz, pc = po.closed_form(n, cap)
        off = capped.prob[~np.eye(n, dtype=bool)]
        assert abs(capped.log_z - lz) <= 1e-13 and (n == 1 or np.abs(off - pc).max() <= 1e-14)


def test_ref_dp_survives_tables_whose_exp_underflows():
    for which in ("offsets", "dominated"):
        tables, ref = po.range_case(which, 6)
        mp = po.ref_mp(tables[0])
        eps = po.eps_of(ref.f)
        po.assert_close(ref.log_z, mp.log_z, eps, which)
        po.assert_close(ref.prob, mp.prob, po.prob_tol(eps, 6), which)
        assert np.isfinite(ref.log_z) and ref.log_z < -20000.0


def test_flag_reference():
    table = po.make_tables("random", 1, 3, seed=1)[0]
    table[:, 1] = np.nan
    for ref in (po.ref_dp(table), po.ref_brute(table), po.ref_mp(table)):
        assert ref.flag == 1 and ref.log_z == -np.inf and not ref.prob.any() and not ref.family.any()


def test_the_package_name_posterior_is_still_the_inference_function():
    """dags_vae_search_amd/posterior.py is a submodule whose name the package already exports as infer.posterior: the
    function wins, and the new entry points are exported next to it"""
    import sys
    import types
    import dags_vae_search_amd as pkg
    assert isinstance(pkg.posterior, types.FunctionType) and pkg.posterior.__module__ == "dags_vae_search_amd.infer"
    mod = sys.modules["dags_vae_search_amd.posterior"]
    assert pkg.arc_posterior is mod.arc_posterior and pkg.arc_posterior_from_tables is mod.arc_posterior_from_tables
    assert pkg.ArcPosterior is mod.ArcPosterior and "order-modular" in mod.__doc__.lower() and "order-modular" in mod.arc_posterior_from_tables.__doc__
