"""dvs_bn_scores (csrc/k_bic.hip: loglik, aic, bic, bde, bds, k2, bdj) on the host emulator: every case, reference,
tolerance and check comes from tests/bn_score_corpus.py, which tests/test_gpu_bn_scores.py runs unchanged on the device;
the cases themselves are those of tests/scoring_corpus.py.  The emulator build calls libm's re-entrant lgamma where the
device build calls the device math library's."""
import pytest

from tests import bn_score_corpus as bn
from tests import scoring_corpus as sc

WORST = {}


@pytest.fixture(scope="module")
def be():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


def test_corpus_cases_keep_their_refusals_to_one_dag_in_four():
    """The condition this module shares with tests/test_emu_scoring.py, re-asserted on the imported cases: the refused
    cells of a case are exactly those the documented limits refuse, in at most one DAG in four."""
    bn.check_shared_condition()


@pytest.mark.parametrize("name", sc.BIC_CASE_NAMES)
def test_emu_bn_case(be, name):
    """Every (type, argument) of bn.VARIANTS on one case of the BIC corpus: local scores and per-DAG sums within
    1e-12 * T of the 60-digit reference (itself cross-checked by a float64 scipy.special.gammaln evaluation), refusals,
    bitwise pairs, exact zeros; the small cases twice for equal bytes.  Worst |got - ref| / T measured on the emulator
    build over all cases: loglik 6.8e-16, aic 6.8e-16, bic 6.8e-16, bde 3.5e-16, bds 3.5e-16, k2 2.1e-16, bdj 2.8e-16."""
    bn.check_all_variants(be, sc.bic_case(name), name.startswith(("batch", "keybits", "levels")), WORST)


def test_emu_report_worst_error_per_type(be):
    """Prints the worst |got - ref| / T per type over the cases run so far (run the module whole for all of them)."""
    bn.report(WORST, "emulator")


def test_emu_k2_equals_the_log_of_exact_factorials(be):
    bn.check_k2_against_factorials(be)


def test_emu_covered_edge_reversal_keeps_bde_bic_aic_loglik_and_moves_k2_bdj(be):
    bn.check_covered_edge_reversal(be)


@pytest.mark.parametrize("name", bn.BYTES_CASES)
def test_emu_bic_bytes_equal_dvs_bic_scores_and_aic_meets_bic_and_loglik(be, name):
    bn.check_bic_bytes_and_aic_relations(be, name)


@pytest.mark.parametrize("name", bn.BDS_CASES)
def test_emu_bds_equals_bde_where_every_configuration_is_observed(be, name):
    same, diff = bn.check_bds_against_bde(be, name)
    print(f"\n{name}: bds == bde in {same} cells, apart in {diff}")
    assert same > 0 and (diff > 0 or name != "levels")


def test_emu_dense_and_sort_paths_agree_on_one_table(be):
    worst = bn.check_dense_and_sort_paths_agree(be)
    print(f"\ndense vs sort: worst |dense - sort| / T = {worst:.3g}")


def test_emu_argument_refusals(be):
    import ctypes
    bn.check_argument_refusals(be.lib, ctypes.c_void_p(4096))
