"""Structure comparison (csrc/dvs_cpdag.h: dvs_cpdag, dvs_pdag_compare) on the host emulator: every case, reference and
check comes from tests/cpdag_corpus.py, which tests/test_gpu_cpdag.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import cpdag_corpus as cp
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return cp.Driver(sc.EmuBackend(emu()))


@pytest.mark.parametrize("n", [4, 5])
def test_emu_cpdag_all_labelled_dags(n):
    """all 543 and all 29 281, each as one launch: the emulator is quick enough for the whole of n = 5"""
    assert cp.check_all_dags(driver(), n) == cp.DAG_COUNTS[n]


@pytest.mark.parametrize("n", cp.RANDOM_SIZES)
def test_emu_cpdag_random_dags_in_permuted_order(n):
    print(f"\nemulator n = {n}: rules fired {sorted(cp.check_random(driver(), n))}")


def test_emu_cpdag_complete_order_and_empty_graph():
    cp.check_extremes(driver())


@pytest.mark.parametrize("n", [33, 48])
def test_emu_cpdag_is_unchanged_by_a_covered_edge_reversal(n):
    cp.check_covered_edge(driver(), n)


def test_emu_cpdag_flags_sit_between_clean_rows():
    cp.check_flags(driver())


def test_emu_pdag_compare_hand_made_pairs():
    cp.check_compare_hand(driver())


@pytest.mark.parametrize("n", [5, 33, 48])
def test_emu_pdag_compare_random_pairs(n):
    assert cp.check_compare_random(driver(), n) > 0


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    cp.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    cp.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
