"""The restated MMPC of tests/local_corpus.py against truth, on the CPU: fed by an exact d-separation oracle it returns the
skeleton of every labelled DAG on up to five vertices; the binding of the fourth companion header."""
import pytest

from dags_vae_search_amd import _lib as dl
from tests import local_corpus as lc


@pytest.mark.parametrize("n", (3, 4, 5))
def test_restated_mmpc_with_a_dsep_oracle_finds_the_true_skeleton_of_every_dag(n):
    classes, asymmetric = lc.check_oracle_all_dags(n)
    print(f"\nn = {n}: {classes} equivalence classes, {asymmetric} members removed by the symmetry correction")


def test_fourth_companion_header_binding():
    assert list(dl.LOCAL_SIGNATURES) == ["dvs_ci_tests_group", "dvs_mmpc_update"]
    assert not set(dl.LOCAL_SIGNATURES) & (set(dl.SIGNATURES) | set(dl.EXT_SIGNATURES) | set(dl.INC_SIGNATURES) | set(dl.AVAIL_SIGNATURES))
    assert len(dl.EXPORTS) == 64 and dl.ABI_VERSION == 202
    assert dl.signature("dvs_ci_tests_group") is dl.LOCAL_SIGNATURES["dvs_ci_tests_group"]
    assert [n for n, _ in dl.signature("dvs_ci_tests_group")[1]] == [
        "n_groups", "n_vars", "n_samples", "data", "card", "target", "cond", "candidates", "test_type", "lds_cells", "out", "out_bytes",
        "status", "stream"]
    assert [n for n, _ in dl.signature("dvs_mmpc_update")[1]] == [
        "n_vars", "n_groups", "phase", "target", "cond", "candidates", "group_offsets", "out", "out_bytes", "alpha", "cpc", "cand",
        "cpc_next", "cand_next", "last", "pmax", "smin", "sepset", "state_bytes", "refused", "result", "result_bytes", "stream"]
    lib = dl.load()
    assert lib.dvs_ci_tests_group.argtypes == [c for _, c in dl.LOCAL_SIGNATURES["dvs_ci_tests_group"][1]]
    with pytest.raises(KeyError, match="dvs_local.h"):
        dl.signature("dvs_no_such_call")
