"""Gaussian networks (csrc/dvs_gaussian.h: dvs_gbn_moments, dvs_gbn_scores, dvs_gbn_toggle_scores, dvs_gbn_fit) through the raw
ABI on the host emulator: every case, the restatement, the references and the checks come from tests/gaussian_corpus.py, which
tests/test_gpu_gaussian.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from dags_vae_search_amd import gaussian  # noqa: F401  (the module under test: its absence fails every test of this file)
from tests import gaussian_corpus as gc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("S", gc.S_VALUES)
@pytest.mark.parametrize("n", gc.N_VALUES)
def test_emu_moments(n, S):
    worst = gc.check_moments(backend(), n, S)
    print(f"n {n} S {S}: worst moment error / bound {worst:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
def test_emu_scores_against_mpmath(n, S):
    worst = gc.check_scores(backend(), n, S)
    print(f"n {n} S {S}: worst score error / bound {worst:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
def test_emu_fit_against_mpmath(n, S):
    worst = gc.check_fit(backend(), n, S)
    print(f"n {n} S {S}: worst coefficient / intercept / sd error / bound {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e}")


def test_emu_refusals_between_sentinels():
    gc.check_refusals(backend())


@pytest.mark.parametrize("n", (5, 17, 48))
def test_emu_toggle_cells_are_the_scorer_bytes(n):
    gc.check_toggles(backend(), n, variants=gc.SCORE_VARIANTS if n == 5 else (("bic-g", None, None), ("bge", None, None)))


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    gc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    gc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
