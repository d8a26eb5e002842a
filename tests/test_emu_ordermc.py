"""Order MCMC (csrc/dvs_ordermc.h: dvs_order_mcmc, dvs_order_mcmc_finish) on the host emulator: every case, reference and
check comes from tests/ordermc_corpus.py, which tests/test_gpu_ordermc.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import ordermc_corpus as oc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def driver():
    from tests.emu.harness import emu
    return oc.Driver(sc.EmuBackend(emu()))


@pytest.mark.parametrize("name", sorted(oc.TRAJECTORIES))
def test_emu_order_mcmc_follows_the_reference_trajectory(name):
    oc.check_trajectory(driver(), name)


def test_emu_order_mcmc_all_zero_scores_closed_form():
    oc.check_all_zero(driver())


@pytest.mark.parametrize("which", ["offsets", "dominated"])
def test_emu_order_mcmc_on_scores_whose_exp_underflows(which):
    oc.check_range(driver(), which)


def test_emu_order_mcmc_cut_into_calls_and_shards_gives_equal_bytes():
    oc.check_cutting(driver())


def test_emu_order_mcmc_flags_a_malformed_list_and_leaves_the_outputs():
    oc.check_flags(driver())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    oc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    oc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
