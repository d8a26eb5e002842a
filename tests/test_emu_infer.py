"""Inference on a fitted network (csrc/dvs_infer.h: dvs_bn_lw, dvs_bn_blanket_posterior) on the host emulator through the raw
C ABI: every case, reference and check comes from tests/infer_corpus.py, which tests/test_gpu_infer.py runs unchanged on the
device."""
import functools

import pytest

from tests import infer_corpus as ic
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("n_particles", ic.PARTICLE_COUNTS)
@pytest.mark.parametrize("name", ic.LW_NETWORKS)
def test_emu_lw_equals_the_restatement(name, n_particles):
    ic.check_lw_case(backend(), name, n_particles)


def test_emu_lw_evidence_of_probability_zero_weighs_exactly_zero():
    ic.check_lw_zero_theta(backend())


def test_emu_lw_one_call_equals_each_query_alone_with_its_offset():
    ic.check_lw_query_offset(backend())


def test_emu_lw_lds_and_global_thresholds_give_the_same_bytes():
    ic.check_lw_lds_and_global(backend())


def test_emu_lw_refusals():
    ic.check_lw_refusals(backend())


@pytest.mark.parametrize("n_rows", ic.ROW_COUNTS)
@pytest.mark.parametrize("name", ("asia", "sachs"))
def test_emu_blanket_posterior_equals_the_numpy_products(name, n_rows):
    ic.check_blanket_rows(backend(), name, n_rows)


def test_emu_blanket_posterior_ties_zero_rows_nan_bad_level_and_bad_slot():
    ic.check_blanket_special(backend())


def test_emu_argument_refusals():
    ic.check_argument_refusals(backend().lib)


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    ic.check_argument_refusals(dl.load())
