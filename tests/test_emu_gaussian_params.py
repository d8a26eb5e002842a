"""A fitted Gaussian network (csrc/dvs_gaussian_params.h: dvs_gbn_joint, dvs_gbn_quantiles, dvs_gbn_sample, dvs_gbn_loglik,
dvs_gbn_predict) through the raw ABI on the host emulator: every case, the restatement, the references and the checks come from
tests/gaussian_params_corpus.py, which tests/test_gpu_gaussian_params.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import gaussian_params_corpus as gp
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


def test_emu_quantiles():
    print(gp.check_quantiles(backend()))


@pytest.mark.parametrize("n", gp.N_VALUES)
def test_emu_joint_equals_the_restatement(n):
    gp.check_joint(backend(), n)


@pytest.mark.parametrize("n_rows", gp.SAMPLE_ROWS)
@pytest.mark.parametrize("n", gp.N_VALUES)
def test_emu_sample(n, n_rows):
    central, worst = gp.check_sample(backend(), n, n_rows)
    print(f"n {n} rows {n_rows}: {central} central rows equal as bytes, worst error / bound elsewhere {worst:.3e}")


def test_emu_sample_cut_into_calls():
    gp.check_sample_cut(backend())


def test_emu_sample_refusals_leave_the_output_untouched():
    gp.check_sample_refusals(backend())


@pytest.mark.parametrize("S", gp.LOGLIK_S)
@pytest.mark.parametrize("B", gp.LOGLIK_B)
def test_emu_loglik(B, S):
    print(f"B {B} S {S}: worst error / bound {gp.check_loglik(backend(), B, S):.3e}")


def test_emu_loglik_two_chunks_in_a_slot():
    gp.check_loglik_two_chunks_in_a_slot(backend())


def test_emu_loglik_many_structures_per_workgroup():
    print(f"B {gp.MANY_B} S {gp.MANY_S}: worst error / bound {gp.check_loglik_many_structures_per_workgroup(backend()):.3e}")


def test_emu_predict_many_structures_per_workgroup():
    gp.check_predict_many_structures_per_workgroup(backend())


@pytest.mark.parametrize("n", (17, 48))
def test_emu_loglik_wide(n):
    print(f"n {n}: worst error / bound {gp.check_loglik_wide(backend(), n):.3e}")


def test_emu_loglik_malformed_between_neighbours():
    gp.check_loglik_malformed(backend())


@pytest.mark.parametrize("n", gp.PREDICT_N)
def test_emu_predict(n):
    print(f"n {n}: worst mode 1 error / bound {gp.check_predict(backend(), n):.3e}")


def test_emu_predict_malformed_between_neighbours():
    gp.check_predict_malformed(backend())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    gp.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    gp.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
