"""The numpy restatement of tests/available_corpus.py against truth, on the CPU: the definition of the available-case local
score against 60-digit mpmath on the gathered rows and against two closed forms; the conditions the corpus sets itself; and
the binding of the third companion header."""
import numpy as np
import pytest

from dags_vae_search_amd import _lib as dl
from tests import available_corpus as av


def test_restatement_against_mpmath_on_every_family_of_n12_heavy():
    assert len(av.truth_families()) >= 40
    print(f"\nthe largest error is {av.check_restatement_against_mpmath():.3f} of its bound")


def test_restatement_against_the_closed_forms():
    av.check_hand_cases(None)


def test_the_formula_is_one_division_two_products_one_subtraction():
    LL, m, k, r, q = np.float64(-123.456789), 7, 97 ** -0.25, 3, 27.0
    assert av.formula(LL, m, k, r, q) == LL / 7 - (k * 2.0) * 27.0
    assert av.formula(LL, m, 0.0, r, q) == LL / 7


def test_third_companion_header_binding():
    assert list(dl.AVAIL_SIGNATURES) == ["dvs_bn_scores_avail", "dvs_bn_toggle_scores_avail"]
    assert not set(dl.AVAIL_SIGNATURES) & (set(dl.SIGNATURES) | set(dl.EXT_SIGNATURES) | set(dl.INC_SIGNATURES))
    assert len(dl.EXPORTS) == 64 and dl.ABI_VERSION == 202 and len(dl.SCORE_TYPES) == 7
    assert dl.signature("dvs_bn_scores_avail") is dl.AVAIL_SIGNATURES["dvs_bn_scores_avail"]
    assert [n for n, _ in dl.signature("dvs_bn_scores_avail")[1]] == [
        "batch", "n_vars", "n_samples", "data", "observed", "card", "parents", "k", "local", "out", "used", "status", "stream"]
    assert [n for n, _ in dl.signature("dvs_bn_toggle_scores_avail")[1]] == [
        "batch", "n_vars", "n_samples", "data", "observed", "card", "parents", "k", "worklist", "local", "local_bytes", "toggles",
        "toggles_bytes", "status", "stream"]
    lib = dl.load()
    assert lib.dvs_bn_scores_avail.argtypes == [c for _, c in dl.AVAIL_SIGNATURES["dvs_bn_scores_avail"][1]]
    with pytest.raises(KeyError, match="dvs_available.h"):
        dl.signature("dvs_no_such_call")


def test_a_missing_third_companion_header_is_an_error_that_gives_its_path(tmp_path):
    path = str(tmp_path / "include" / "dvs_available.h")
    with pytest.raises(RuntimeError, match="dvs_available.h not found at") as e:
        dl._read_header(path)
    assert path in str(e.value)
