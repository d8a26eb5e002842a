"""Gaussian CI tests (csrc/dvs_gaussian_ci.h: dvs_gbn_ci_tests, dvs_gbn_ci_tests_group) through the raw ABI on the host emulator:
every case, the restatement, the references and the checks come from tests/gaussian_ci_corpus.py, which
tests/test_gpu_gaussian_ci.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import gaussian_ci_corpus as gi
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("T", gi.T_VALUES)
@pytest.mark.parametrize("n, S", gi.DATA_SHAPES)
def test_emu_tests_against_mpmath(n, S, T):
    ws, wp = gi.check_against_mpmath(backend(), n, S, T)
    print(f"n {n} S {S} T {T}: worst statistic error / bound {ws:.3e}, worst p error / bound {wp:.3e}")


def test_emu_four_rows_leave_cor_one_degree_of_freedom_and_zf_none():
    gi.check_short_set(backend())


def test_emu_refusals_between_sentinels():
    gi.check_refusals(backend())


@pytest.mark.parametrize("n, S", gi.DATA_SHAPES)
def test_emu_grouped_cells_are_the_per_test_bytes(n, S):
    cells = gi.check_group_equal_bytes(backend(), n, S)
    print(f"n {n}: {cells} grouped cells equal to dvs_gbn_ci_tests as bytes")


def test_emu_row_sets_are_the_gathered_rows_bytes():
    gi.check_row_sets(backend())


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_emu_pc_stable_equals_the_restatement(n, S, typ):
    got = gi.check_pc_raw(backend(), n, S, typ)
    assert sum(got.tests_per_level) == {5: 30, 8: 72, 17: 949}[n]


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_emu_mmpc_equals_the_restatement(n, S, typ):
    gi.check_mmpc_raw(backend(), n, S, typ)


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    gi.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    gi.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
