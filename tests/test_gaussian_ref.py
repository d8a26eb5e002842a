"""CPU only: the numpy restatement of include/dvs_gaussian.h (tests/gaussian_corpus.py) against exact rationals, against mpmath
at 60 digits and against a route that never forms a Cholesky factor (lstsq on the raw rows, slogdet), all under the bounds the
corpus derives; score equivalence of the bge restatement, which pins the constants of the Kuipers correction; the sixth
header's binding; and that the corpus holds the shapes it names."""
import math

import mpmath as mp
import numpy as np
import pytest

from dags_vae_search_amd import gaussian  # noqa: F401  (the module under test: its absence fails every test of this file)
from tests import gaussian_corpus as gc


@gc.at60
def test_bge_restatement_is_score_equivalent_on_four_vertices():
    """run first: all DAGs of one Markov equivalence class get the same total, in mpmath; if this fails the formula of the
    header is wrong, not the kernel"""
    n, S = 4, 40
    x = gc.gauss_data(n, S, seed=3)
    for a1, a2 in ((None, None), (2.0, None), (0.5, n + 5.5)):
        ref = gc.Reference(gc.ExactMoments(x))
        table = {(v, m): ref.local(v, gc.bits_of(m), "bge", a1, a2)[0] for v in range(n) for m in range(1 << n) if not (m >> v) & 1}
        classes = {}
        for P in gc.all_dags(n):
            classes.setdefault(gc.cpdag_key(P), []).append(sum(table[v, int(P[v])] for v in range(n)))
        assert len(classes) == 185                                      # the Markov equivalence classes on 4 vertices
        spread = max(max(c) - min(c) for c in classes.values())
        assert spread < mp.mpf(10) ** -50, float(spread)
        totals = sorted(c[0] for c in classes.values())
        assert min(b - a for a, b in zip(totals, totals[1:])) > mp.mpf(10) ** -6      # and the classes do differ
    # the likelihood scores are score equivalent as well: loglik-g of a complete DAG does not depend on the order
    tab = {(v, m): ref.local(v, gc.bits_of(m), "loglik-g")[0] for v in range(n) for m in range(1 << n) if not (m >> v) & 1}
    full = [sum(tab[v, gc.mask_of(order[:k])] for k, v in enumerate(order)) for order in ([0, 1, 2, 3], [3, 1, 0, 2], [2, 3, 1, 0])]
    # RSS / dof with dof = m - p - 1 is NOT order invariant (the unbiased variance), RSS / m would be: the restated
    # definition is bnlearn's as recalled, so only closeness is asserted
    assert max(full) - min(full) < 1


@pytest.mark.parametrize("S", gc.S_VALUES)
@pytest.mark.parametrize("n", gc.N_VALUES)
def test_restated_moments_against_exact_rationals(n, S):
    x = gc.gauss_data(n, S)
    worst = gc.moments_against_exact(gc.restated_moments(x)[0], gc.exact_of(n, S))
    rows = gc.row_sets(S, max(1, S // 2 + 3))
    sets = gc.restated_moments(x, rows)
    for r in range(len(rows)):
        assert sets[r].tobytes() == gc.restated_moments(np.ascontiguousarray(x[rows[r]]))[0].tobytes()
    print(f"n {n} S {S}: worst moment error / bound {worst:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
@gc.at60
def test_restated_scores_and_the_lstsq_route_against_mpmath(n, S):
    """the independent route passes under the bound before anything else is compared with it, then the restatement"""
    x, ref = gc.gauss_data(n, S), gc.reference_of(n, S)
    mom = gc.restated_moments(x)[0]
    worst_ls = worst_rs = 0.0
    for variant in gc.SCORE_VARIANTS:
        typ, a1, a2 = gc.variant_args(n, variant)
        for v, pa in gc.score_families(n):
            want, bound = ref.local(v, pa, typ, a1, a2)
            e_ls = float(abs(mp.mpf(gc.lstsq_family(x, v, pa, typ, a1, a2)) - want))
            e_rs = float(abs(mp.mpf(gc.restated_local(mom, n, v, gc.mask_of(pa), typ, a1, a2)) - want))
            assert e_ls <= bound, ("lstsq", typ, v, pa, e_ls, bound)
            assert e_rs <= bound, ("restated", typ, v, pa, e_rs, bound)
            worst_ls, worst_rs = max(worst_ls, e_ls / bound), max(worst_rs, e_rs / bound)
    print(f"n {n} S {S}: worst score error / bound: lstsq route {worst_ls:.3e}, restatement {worst_rs:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
@gc.at60
def test_restated_fit_and_lstsq_against_mpmath(n, S):
    x, ref = gc.gauss_data(n, S), gc.reference_of(n, S)
    mom = gc.restated_moments(x)[0]
    worst = 0.0
    for v, pa in gc.score_families(n):
        (beta, c0, sd), (cb, ib, sb) = ref.fit(v, pa)
        for name, (coef, icpt, s) in (("lstsq", gc.lstsq_fit(x, v, pa)), ("restated", gc.restated_fit(mom, n, v, gc.mask_of(pa)))):
            for u in pa:
                e = float(abs(mp.mpf(float(coef[u])) - beta[u]))
                assert e <= cb, (name, "coef", v, pa, u, e, cb)
                worst = max(worst, e / cb)
            e1, e2 = float(abs(mp.mpf(float(icpt)) - c0)), float(abs(mp.mpf(float(s)) - sd))
            assert e1 <= ib and e2 <= sb, (name, v, pa, e1, ib, e2, sb)
    print(f"n {n} S {S}: worst coefficient error / bound {worst:.3e}")


def test_restated_refusals():
    for name, x, rows, n, v, pm, by_lik, by_bge in gc.refusal_cases():
        mom = gc.restated_moments(x, rows)[0]
        assert math.isnan(gc.restated_local(mom, n, v, pm, "loglik-g")) == by_lik, name
        assert math.isnan(gc.restated_local(mom, n, v, pm, "bic-g")) == by_lik, name
        assert math.isnan(gc.restated_local(mom, n, v, pm, "bge")) == by_bge, name
        assert math.isnan(gc.restated_fit(mom, n, v, pm)[2]) == by_lik, name
    # exact singularity on the data set whose moments are exact
    mom = gc.restated_moments(gc.degenerate_data())[0]
    assert mom[6:].tobytes() == gc.ExactMoments(gc.degenerate_data()).C_float().tobytes()
    for v, pa in gc.score_families(5):
        assert math.isnan(gc.restated_local(mom, 5, v, gc.mask_of(pa), "loglik-g")) == gc.degenerate_singular(v, gc.mask_of(pa)), (v, pa)


def test_corpus_shapes():
    from dags_vae_search_amd import _lib as dl
    assert gc.CHUNK == 128 and gc.CAP == dl.GBN_MAX_PARENTS >= 8
    assert gc.S_VALUES == (2, 127, 128, 129, 389) and gc.N_VALUES == (1, 3, 5, 17, 48)
    assert len(gc.score_families(5)) == 5 * 16
    assert max(len(pa) for _, pa in gc.score_families(17)) == gc.CAP
    names = [c[0] for c in gc.refusal_cases()]
    for want in ("p = cap", "p = cap + 1", "m = p + 1", "m = p + 2", "duplicated column", "linear combination", "bit 47", "bit >= n"):
        assert want in names
    assert [len(gc.all_dags(k)) for k in (3, 4, 5)] == [25, 543, 29281]


def test_sixth_header_binding():
    from dags_vae_search_amd import _lib as dl
    assert list(dl.GAUSS_SIGNATURES) == ["dvs_gbn_moments_workspace_bytes", "dvs_gbn_moments", "dvs_gbn_scores",
                                         "dvs_gbn_toggle_scores", "dvs_gbn_fit"]
    assert not set(dl.GAUSS_SIGNATURES) & (set(dl.SIGNATURES) | set(dl.EXT_SIGNATURES) | set(dl.INC_SIGNATURES)
                                           | set(dl.AVAIL_SIGNATURES) | set(dl.LOCAL_SIGNATURES) | set(dl.PERM_SIGNATURES))
    assert len(dl.SIGNATURES) == 64 and dl.ABI_VERSION == 202
    assert dl.signature("dvs_gbn_fit") is dl.GAUSS_SIGNATURES["dvs_gbn_fit"]
    assert dl.GSCORE_TYPES == {t: i for i, t in enumerate(gc.TYPES)}
    with pytest.raises(KeyError, match="dvs_gaussian.h"):
        dl.signature("dvs_nothing")
