"""A fitted conditional Gaussian network (csrc/dvs_mixed_params.h: dvs_cgbn_sample, dvs_cgbn_loglik, dvs_cgbn_predict) through the
raw ABI on the host emulator: every case, the restatement, the references and the checks come from
tests/mixed_params_corpus.py, which tests/test_gpu_mixed_params.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import mixed_params_corpus as mc
from tests import scoring_corpus as sc

KEYS = ("small", "mid", "wide")


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_emu_sample(key, S):
    central, worst = mc.check_sample(backend(), key, S)
    print(f"{key} rows {S}: {central} central rows equal as bytes, worst error / bound elsewhere {worst:.3e}")


def test_emu_sample_cut_into_calls():
    mc.check_sample_cut(backend())


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_emu_loglik(key, S):
    print(f"{key} S {S}: worst error / bound {mc.check_loglik(backend(), key, S):.3e}")


def test_emu_loglik_two_chunks_in_a_slot():
    print(f"small S {mc.BIG_S}: worst error / bound {mc.check_loglik(backend(), 'small', mc.BIG_S):.3e}")


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS)
def test_emu_predict_real_targets(key, S):
    print(f"{key} S {S}: worst mode 1 error / bound {mc.check_predict_real(backend(), key, S):.3e}")


@pytest.mark.parametrize("S", mc.S_VALUES)
@pytest.mark.parametrize("key", KEYS + ("kids",))
def test_emu_predict_class(key, S):
    print(f"{key} S {S}: worst posterior error / bound {mc.check_predict_class(backend(), key, S):.3e}")


def test_emu_all_continuous_networks_give_the_gaussian_entry_points_bytes():
    mc.check_all_continuous_identities(backend())


def test_emu_malformed_networks():
    mc.check_malformed(backend())


def test_emu_rows_that_meet_trouble():
    mc.check_row_trouble(backend())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    mc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    mc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
