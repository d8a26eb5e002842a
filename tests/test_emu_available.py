"""Available-case scoring on incomplete data (csrc/dvs_available.h: dvs_bn_scores_avail, dvs_bn_toggle_scores_avail) on the
host emulator: every case, reference and check comes from tests/available_corpus.py, which tests/test_gpu_available.py runs
unchanged on the device."""
import ctypes
import functools

import pytest

from tests import available_corpus as av
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return av.AvailDriver(sc.EmuBackend(emu()))


def test_the_corpus_meets_its_own_conditions():
    print(f"\n(scored m = 0, scored m = 1, toggled m = 0, toggled m = 1) per data set: {av.check_conditions()}")


@pytest.mark.parametrize("kind", av.MASK_SETS)
@pytest.mark.parametrize("name", av.DATASETS)
def test_emu_scores_are_the_formula_over_the_plain_scorer_on_the_rows_that_count(name, kind):
    print(f"\n{name} {kind}: {dict(av.check_scores(driver(), name, kind))}")


@pytest.mark.parametrize("name", av.DATASETS)
def test_emu_everything_observed_is_the_plain_scorer_over_n_samples(name):
    av.check_everything_observed(driver(), name)


@pytest.mark.parametrize("kind", ("light", "heavy"))
@pytest.mark.parametrize("name", av.DATASETS)
def test_emu_toggle_cells_are_the_scorer_on_the_flipped_structure(name, kind):
    av.check_toggles(driver(), name, kind)


def test_emu_kernels_against_the_restatement():
    av.check_kernels_against_restatement(driver())


def test_emu_hand_cases_in_closed_form():
    av.check_hand_cases(driver())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    av.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    av.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def test_emu_refusals_leave_the_outputs_untouched():
    av.check_refusals_leave_outputs_untouched(driver())
