"""A normal conditioned on every row's observed part (csrc/dvs_gaussian_incomplete.h: dvs_gbn_condition) through the raw ABI on
the host emulator: every case, the restatement and the checks come from tests/gaussian_incomplete_corpus.py, which
tests/test_gpu_gaussian_incomplete.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import gaussian_incomplete_corpus as gi
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("n, S, kind", gi.shape_cases())
def test_emu_condition_equals_the_restatement(n, S, kind):
    print(f"n {n} S {S} {kind}: worst logp difference / allowance {gi.check_condition(backend(), n, S, kind):.3e}")


def test_emu_every_row_its_own_pattern():
    gi.check_unique_patterns(backend())


def test_emu_a_run_across_a_chunk_boundary():
    gi.check_straddle(backend())


def test_emu_second_level_of_the_tree():
    gi.check_second_level(backend())


def test_emu_orders():
    gi.check_orders(backend())


def test_emu_null_outputs_keep_the_other_bytes():
    gi.check_null_outputs(backend())


def test_emu_refusals_between_neighbours():
    gi.check_refusals(backend())


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    gi.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    gi.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
