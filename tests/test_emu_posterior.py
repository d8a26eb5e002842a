"""Exact arc posterior (csrc/dvs_posterior.h: dvs_arc_posterior_workspace_bytes, dvs_arc_posterior) on the host emulator: every
case, reference and check comes from tests/posterior_corpus.py, which tests/test_gpu_posterior.py runs unchanged on the
device (the emulator takes under two seconds for the three-pass size n = 17, so it runs here too; sachs is left to the device)."""
import ctypes
import functools

import pytest

from tests import exact_corpus as ex
from tests import posterior_corpus as po
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return po.Driver(sc.EmuBackend(emu()))


@pytest.mark.parametrize("kind", po.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_emu_posterior_equals_brute_force_over_all_dags(n, kind):
    po.check_brute(driver(), n, kind)


@pytest.mark.parametrize("kind", po.KINDS)
@pytest.mark.parametrize("n", po.STAGE_SIZES)
def test_emu_posterior_every_stage_matches_ref_dp(n, kind):
    if n >= po.BIG and kind != "random":
        return                                                             # the three-pass size runs the plain table only
    po.check_stages(driver(), n, kind)


@pytest.mark.parametrize("n,cap", [(2, None), (2, 1), (9, None), (9, 2), (10, None), (10, 3), (17, None)])
def test_emu_posterior_closed_form_on_the_all_zero_table(n, cap):
    po.check_closed_form(driver(), n, cap)


@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("which", ["offsets", "dominated"])
def test_emu_posterior_on_tables_whose_exp_underflows(which, n):
    po.check_range(driver(), which, n)


@pytest.mark.parametrize("n", [1, 5, 9])
def test_emu_posterior_flag_for_a_table_without_any_dag(n):
    po.check_flags(driver(), n)


def test_emu_posterior_two_calls_give_equal_bytes():
    po.check_determinism(driver())


@pytest.mark.parametrize("typ,arg", [("bic", None), ("bde", 10.0)])
def test_emu_posterior_on_asia(typ, arg):
    from tests.emu.harness import emu
    real = ex.EmuReal(emu(), "asia", typ, arg)
    po.check_real_asia(real, po.Driver(real.be))


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    po.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    po.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
