"""BN parameters (csrc/dvs_params.h: dvs_bn_fit, dvs_bn_sample, dvs_bn_loglik) on the host emulator through the raw C ABI:
every case, reference and check comes from tests/params_corpus.py, which tests/test_gpu_params.py runs unchanged on the
device."""
import ctypes
import functools

import pytest

from tests import params_corpus as pm
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("name", pm.FIT_CASE_NAMES)
def test_emu_fit_equals_exact_rationals(name):
    pm.check_fit_case(backend(), name)


def test_emu_fit_refuses_a_bad_slot_alone():
    pm.check_fit_bad_slots(backend())


@pytest.mark.parametrize("n_rows", pm.ROW_COUNTS)
def test_emu_sample_equals_the_restatement(n_rows):
    pm.check_sample(backend(), "small", n_rows)


@pytest.mark.parametrize("name", ("chain48", "hand"))
def test_emu_sample_networks(name):
    pm.check_sample(backend(), name, 300)


def test_emu_sample_never_draws_a_zero_probability_level():
    pm.check_sample_zero_levels(backend())


def test_emu_sample_lds_and_global_thresholds_give_the_same_bytes():
    pm.check_sample_lds_and_global(backend())


def test_emu_sample_chunks_and_row_offset():
    pm.check_sample_chunks(backend())


def test_emu_sample_refusals():
    pm.check_sample_refusals(backend())


@pytest.mark.parametrize("n_rows", pm.ROW_COUNTS)
def test_emu_loglik_equals_fsum_of_logs(n_rows):
    pm.check_loglik_rows(backend(), n_rows)


def test_emu_loglik_zero_nan_bad_level_and_bad_slot():
    pm.check_loglik_special(backend())


@pytest.mark.parametrize("name", ("asia", "sachs"))
def test_emu_loglik_of_the_mle_fit_equals_the_scorer(name):
    pm.check_loglik_equals_scorer(backend(), name)


def test_emu_argument_refusals():
    pm.check_argument_refusals(backend().lib, ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    pm.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
