"""Monte Carlo permutation CI tests (csrc/dvs_permtest.h: dvs_ci_perm_tests) through the raw ABI on the host emulator: every
case, the restatement and the checks come from tests/permtest_corpus.py, which tests/test_gpu_permtest.py runs unchanged on
the device."""
import ctypes
import functools

import pytest

from tests import pc_corpus as pc
from tests import permtest_corpus as pt
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("typ", pt.TYPES)
@pytest.mark.parametrize("S, B", pt.SHAPES)
def test_emu_kernel_is_the_restatement(S, B, typ):
    worst = pt.check_kernel_is_restatement(backend(), S, B, typ, pc.P_RTOL_EMU)
    print(f"S {S} B {B} {typ}: worst relative sp p error {worst:.3e} (allowed {pc.P_RTOL_EMU:.1e})")


def test_emu_klnk_table_and_log_paths_give_equal_bytes():
    pt.check_klnk_paths(backend())


def test_emu_smc_stops():
    pt.check_smc_stops(backend())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    pt.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    pt.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
