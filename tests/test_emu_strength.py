"""Model averaging (csrc/dvs_strength.h: the row-set scorer, dvs_bootstrap_rows, dvs_arc_strength, dvs_averaged_network) on
the host emulator: every case, reference and check comes from tests/strength_corpus.py, which tests/test_gpu_strength.py runs
unchanged on the device.  The CPU-only pins of the references (the restated draw's uniformity, the closed-form threshold
against exact L1 minimisation) live here too."""
import ctypes
import functools

import pytest

from tests import scoring_corpus as sc
from tests import strength_corpus as st


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return st.Driver(sc.EmuBackend(emu()))


@pytest.mark.parametrize("set_size", st.SET_SIZES)
@pytest.mark.parametrize("name", st.ROW_DATASETS)
def test_emu_scores_rows_equal_the_plain_scorer_on_gathered_rows(name, set_size):
    st.check_scores_rows(driver(), name, set_size)


@pytest.mark.parametrize("plan", st.toggle_plan(), ids=lambda p: f"{p[0]}-S{p[1]}-{p[2]}-{p[4]}")
def test_emu_toggle_rows_equal_the_plain_toggle_pass_on_gathered_rows(plan):
    st.check_toggle_rows(driver(), *plan)


@pytest.mark.parametrize("name", st.ROW_DATASETS)
def test_emu_identity_row_set_is_the_plain_call(name):
    st.check_identity_set(driver(), name)


def test_emu_row_set_refusals_leave_the_outputs_untouched():
    st.check_rows_refusals(driver())


@pytest.mark.parametrize("set_size", st.BOOT_SET_SIZES)
def test_emu_bootstrap_rows_bytes(set_size):
    st.check_bootstrap_bytes(driver(), set_size)


def test_emu_bootstrap_rows_offsets_and_wrap():
    st.check_bootstrap_offsets(driver())


def test_restated_bootstrap_draw_is_uniform():
    print(f"\nchi-square over {st.CHI2_BINS} bins: {st.check_restatement_is_uniform():.1f} (bound {st.CHI2_BOUND})")


@pytest.mark.parametrize("n", st.ARC_SIZES)
def test_emu_arc_strength_random_pdags(n):
    st.check_arc_random(driver(), n)


def test_emu_arc_strength_empty_and_complete():
    st.check_arc_extremes(driver())


@pytest.mark.parametrize("n", [3, 8, 48])
def test_emu_averaged_network_random_counts(n):
    st.check_averaged_random(driver(), n)


def test_emu_averaged_network_hand_made():
    st.check_averaged_hand(driver())


def test_emu_averaged_network_sweep_equals_single_calls():
    st.check_averaged_sweep(driver())


def test_closed_form_threshold_equals_exact_l1_minimisation():
    print(f"\ncount sets by kind: {st.check_closed_form_threshold(1000)}")


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    st.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    st.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
