"""Grouped CI tests and the MMPC round (csrc/dvs_local.h: dvs_ci_tests_group, dvs_mmpc_update) on the host emulator: every
case, reference and check comes from tests/local_corpus.py, which tests/test_gpu_local.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import local_corpus as lc
from tests import pc_corpus as pc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("typ", pc.TYPES)
@pytest.mark.parametrize("S", pc.SAMPLE_COUNTS)
def test_emu_grouped_cells_are_the_bytes_of_the_per_test_kernel(S, typ):
    assert lc.check_group_equal_bytes(backend(), S, typ) == 80


def test_emu_grouped_refusals():
    lc.check_group_refusals(backend())


def test_emu_grouped_wide_rows():
    assert lc.check_group_wide(backend()) == 6 * 47


def test_emu_mmpc_update_hand_made_rounds():
    lc.check_update_hand(backend())


@pytest.mark.parametrize("n, seed", [(1, 2711), (7, 2712), (48, 2713), (48, 2714)])
def test_emu_mmpc_update_seeded_rounds(n, seed):
    lc.check_update_seeded(backend(), n, seed)


@pytest.mark.parametrize("name, S, typ", lc.EMU_E2E_CASES)
def test_emu_mmpc_end_to_end_through_the_raw_abi(name, S, typ):
    lc.check_e2e_raw(backend(), name, S, typ)


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    lc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    lc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
