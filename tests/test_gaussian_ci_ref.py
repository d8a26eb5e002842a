"""CPU: the Gaussian CI tests' seventh companion header (include/dvs_gaussian_ci.h) as the binding reads it, and the Python
restatement of its definitions (tests/gaussian_ci_corpus.py) against mpmath at 60 digits on exact moments: the tail's evaluation
error over the grid, every pool case under the derived bounds, and the guards of the PC-stable and MMPC restatements."""
import pytest

from dags_vae_search_amd import _lib as dl
from tests import gaussian_ci_corpus as gi


def test_the_seventh_header_adds_two_entry_points_and_leaves_the_rest():
    assert list(dl.GCI_SIGNATURES) == ["dvs_gbn_ci_tests", "dvs_gbn_ci_tests_group"]
    others = (dl.SIGNATURES, dl.EXT_SIGNATURES, dl.INC_SIGNATURES, dl.AVAIL_SIGNATURES, dl.LOCAL_SIGNATURES, dl.PERM_SIGNATURES,
              dl.GAUSS_SIGNATURES)
    assert all(not set(dl.GCI_SIGNATURES) & set(t) for t in others)
    assert len(dl.EXPORTS) == 64 and dl.ABI_VERSION == 202
    assert list(dl.GAUSS_SIGNATURES) == ["dvs_gbn_moments_workspace_bytes", "dvs_gbn_moments", "dvs_gbn_scores",
                                         "dvs_gbn_toggle_scores", "dvs_gbn_fit"]
    assert dl.signature("dvs_gbn_ci_tests_group") is dl.GCI_SIGNATURES["dvs_gbn_ci_tests_group"]
    assert dl.GCI_TYPES == {"cor": 0, "zf": 1, "mi-g": 2} and dl.GCI_MAX_COND == 10 and dl.GCI_MAX_COND + 2 == dl.GBN_MAX_PARENTS + 1
    assert [k for k, _ in dl.GCI_SIGNATURES["dvs_gbn_ci_tests"][1]] == [
        "n_tests", "n_vars", "moments", "n_sets", "set_of", "pairs", "cond", "test_type", "out", "out_bytes", "status", "stream"]
    assert [k for k, _ in dl.GCI_SIGNATURES["dvs_gbn_ci_tests_group"][1]] == [
        "n_groups", "n_vars", "moments", "n_sets", "set_of", "target", "cond", "candidates", "test_type", "out", "out_bytes", "status",
        "stream"]
    with pytest.raises(KeyError, match="dvs_gaussian_ci.h"):
        dl.signature("dvs_gbn_ci_nothing")


@pytest.mark.parametrize("typ", gi.TYPES)
def test_tail_evaluation_error_over_the_grid_is_what_the_corpus_records(typ):
    worst, tiny, points, stat = gi.tail_grid_error(typ)
    print(f"{typ}: {points} points, largest relative p error {worst:.3e} (recorded {gi.TAIL_MEASURED[typ]:.3e}, held to "
          f"{gi.TAIL_RTOL[typ]:.1e}), largest absolute error below 2^-1022 {tiny:.1e}, largest relative statistic error {stat:.1e}")
    assert points == 2 * len(gi.TAIL_DF) * len(gi.TAIL_R2) and worst <= gi.TAIL_RTOL[typ] and tiny <= gi.P_FLOOR
    assert gi.TAIL_MEASURED[typ] <= gi.TAIL_RTOL[typ] <= 1.05 * gi.TAIL_MEASURED[typ]


def test_the_positive_series_is_mpmath_betainc_where_both_converge():
    import mpmath as mp
    with mp.workdps(60):
        for df, x in ((1, "0.3"), (10, "0.9"), (126, "0.75"), (387, "0.5"), (5000, "0.4"), (5000, "0.9"), (65536, "0.5")):
            a, b, x = mp.mpf(df) / 2, mp.mpf(1) / 2, mp.mpf(x)
            want = mp.betainc(a, b, 0, x, regularized=True)
            assert abs(gi.mp_beta_series(a, b, x, 1 - x) - want) <= want * mp.mpf(10) ** -50, (df, x)


def test_tail_error_of_cor_grows_with_df_as_the_header_states():
    worst = gi.tail_grid_error("cor", dfs=(65536,))[0]
    print(f"cor at df = 65 536: largest relative p error {worst:.3e}")
    assert gi.TAIL_RTOL["cor"] < worst < 1e-10


@pytest.mark.parametrize("n, S", gi.DATA_SHAPES)
def test_restatement_against_mpmath_on_exact_moments(n, S):
    cases, ws, wp, kappa = gi.check_restatement(n, S)
    print(f"n {n} S {S}: {cases} cases, worst statistic error / bound {ws:.3e}, worst p error / bound {wp:.3e}, largest kappa {kappa:.3e}")
    assert kappa < 3.0e2                     # what 3000 random submatrices of 2 to 12 variables of these data sets stayed below
    assert {len(Z) for _, _, Z in gi.pool(n)} == ({0, 1, 2, 3} if n == 5 else {0, 1, 2, 10})


def test_restatement_refuses_what_the_header_refuses():
    from tests import gaussian_corpus as gc
    for name, key, n, (x, y, zm), refusing in gi.refusal_cases():
        data = {"x17": gc.gauss_data(17, 389), "x48": gc.gauss_data(48, 389), "deg": gc.degenerate_data()}[key]
        mom = gc.restated_moments(data)[0]
        for typ in gi.TYPES:
            got = gi.restated_test(mom, n, x, y, zm, typ)
            assert (got[0] != got[0]) == (typ in refusing), (name, typ, got)


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_pc_stable_restatement_decides_clear_of_the_tolerance(n, S, typ):
    gi.check_pc_guard(n, S, typ)


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_mmpc_restatement_decides_and_selects_clear_of_the_tolerance(n, S, typ):
    gi.check_mmpc_guard(n, S, typ)
