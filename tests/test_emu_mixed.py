"""Conditional Gaussian networks on mixed data (csrc/dvs_mixed.h: dvs_cg_partition, dvs_cg_moments, dvs_cg_scores,
dvs_cg_toggle_scores, dvs_cg_fit) through the raw ABI on the host emulator: every case, the references and the checks come from
tests/mixed_corpus.py, which tests/test_gpu_mixed.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from dags_vae_search_amd import mixed  # noqa: F401  (the module under test: its absence fails every test of this file)
from tests import mixed_corpus as mc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("S", mc.PARTITION_S)
def test_emu_partition_is_the_stable_sort(S):
    mc.check_partition(backend(), S)


def test_emu_partition_one_factor_in_each_packed_word():
    mc.check_partition_wide(backend())


def test_emu_partition_cut_into_spans():
    mc.check_partition_spans(backend())


def test_emu_partition_refusals():
    mc.check_partition_refusals(backend())


@pytest.mark.parametrize("nc", (1, 5, 17))
def test_emu_ragged_moments(nc):
    worst = mc.check_moments(backend(), nc)
    print(f"n_c {nc}: worst moment error / bound {worst:.3e}")


def test_emu_scores_against_mpmath():
    worst = mc.check_scores(backend())
    print(f"worst score error / bound {worst:.3e}")


def test_emu_byte_identities():
    mc.check_identities(backend())


def test_emu_refusals_between_sentinels():
    mc.check_refusals(backend())


@pytest.mark.parametrize("n", (5, 17, 48))
def test_emu_toggle_cells_are_the_scorer_bytes(n):
    mc.check_toggles(backend(), n, variants=(("bic-cg", None), ("aic-cg", 0.3)) if n == 5 else (("bic-cg", None),))


def test_emu_fit_against_mpmath():
    worst = mc.check_fit(backend())
    print(f"worst coefficient / intercept / sd error / bound {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e}")


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    mc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    mc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
