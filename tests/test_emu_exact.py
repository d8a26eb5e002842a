"""Exact structure search (csrc/dvs_exact.h: dvs_exact_workspace_bytes, dvs_exact_search) on the host emulator: every case,
reference and check comes from tests/exact_corpus.py, which tests/test_gpu_exact.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import exact_corpus as ex
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return ex.Driver(sc.EmuBackend(emu()))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_emu_exact_score_is_the_maximum_over_all_labelled_dags(n):
    assert ex.check_optimal(driver(), n) == 6


@pytest.mark.parametrize("kind", ex.KINDS)
@pytest.mark.parametrize("n", ex.BYTES_SIZES)
def test_emu_exact_every_stage_equals_ref_dp(n, kind):
    if n >= ex.BIG and kind != "random":
        return                                                             # the three-pass size runs the plain table only
    ex.check_bytes(driver(), n, kind)


@pytest.mark.parametrize("n", [1, 5, 9])
def test_emu_exact_flag_for_a_table_without_any_dag(n):
    ex.check_flags(driver(), n)


@pytest.mark.parametrize("typ,arg", ex.REAL_TYPES)
def test_emu_exact_on_asia(typ, arg):
    from tests.emu.harness import emu
    ex.check_real(ex.EmuReal(emu(), "asia", typ, arg), "asia")


def test_emu_exact_on_sachs_capped():
    """the emulator keeps to bic on the capped sachs table (562 rows of 11 families); the device runs all four types"""
    from tests.emu.harness import emu
    ex.check_real(ex.EmuReal(emu(), "sachs", "bic", None), "sachs")


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    ex.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    ex.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
