"""Constraint-based structure learning (csrc/dvs_citest.h: dvs_ci_tests, dvs_pc_expand, dvs_pc_reduce, dvs_pc_orient) on the
host emulator through the raw C ABI: every case, reference and check comes from tests/pc_corpus.py, which
tests/test_gpu_pc.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import pc_corpus as pc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("typ", pc.TYPES)
@pytest.mark.parametrize("name", pc.CI_CASE_NAMES)
def test_emu_ci_statistic_df_and_p_value(name, typ):
    pc.check_ci_case(backend(), name, typ)


def test_emu_ci_max_cells_refuses_the_larger_tables_only():
    pc.check_ci_max_cells(backend())


def test_emu_pc_expand_equals_sorted_combinations():
    assert pc.check_expand(backend()) > 1000


def test_emu_pc_reduce_hand_made_levels():
    pc.check_reduce(backend())


@pytest.mark.parametrize("n", [3, 4, 5])
def test_emu_pc_orient_with_a_dsep_oracle_gives_the_cpdag_of_every_dag(n):
    assert pc.check_orient_all_dags(backend(), n) == pc.cp.DAG_COUNTS[n]


def test_emu_pc_orient_conflicts_cycle_and_illegal_rows():
    pc.check_orient_hand(backend())


@pytest.mark.parametrize("name,S,typ", pc.EMU_E2E_CASES)
def test_emu_pc_stable_equals_the_restatement(name, S, typ):
    pc.check_e2e_raw(backend(), name, S, typ)


def test_emu_argument_refusals():
    pc.check_argument_refusals(backend().lib, ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    pc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
