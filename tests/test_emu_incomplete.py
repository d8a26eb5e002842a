"""Learning from incomplete data (csrc/dvs_incomplete.h: dvs_bn_expected_counts, dvs_bn_fit_counts, dvs_bn_impute) on the host
emulator through the raw C ABI: every case, reference and check comes from tests/incomplete_corpus.py, which
tests/test_gpu_incomplete.py runs unchanged on the device."""
import functools

import pytest

from tests import incomplete_corpus as nc
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("n_rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("name", nc.BYTES_NETWORKS)
def test_emu_expected_counts_equal_the_restatement(name, n_rows):
    nc.check_counts_bytes(backend(), name, n_rows)


@pytest.mark.parametrize("n_rows", nc.ROW_COUNTS)
@pytest.mark.parametrize("name", nc.BYTES_NETWORKS)
def test_emu_impute_equals_the_restatement(name, n_rows):
    nc.check_impute_bytes(backend(), name, n_rows)


def test_emu_band48_equals_the_restatement():
    nc.check_counts_bytes(backend(), "band48", 257)
    nc.check_impute_bytes(backend(), "band48", 257)


@pytest.mark.parametrize("name", ("hand", "six", "asia"))
def test_emu_rows_per_group_does_not_change_the_bytes(name):
    nc.check_counts_bytes(backend(), name, 257, nc.ROWS_PER_GROUP)
    nc.check_impute_bytes(backend(), name, 257, nc.ROWS_PER_GROUP)


@pytest.mark.parametrize("name", ("hand", "six", "zeroone", "asia"))
def test_emu_fully_observed_counts_are_integers_and_fit_counts_is_bn_fit(name):
    nc.check_fully_observed(backend(), name)


def test_emu_fit_counts_on_fractional_and_bad_counts():
    nc.check_fit_counts_fractional(backend())


def test_emu_em_iterations_equal_the_restatement():
    nc.check_em_step(backend())


@pytest.mark.parametrize("name,targets", (("asia", (1, 4, 7)), ("band48", (0, 23, 47))))
def test_emu_impute_with_every_other_variable_observed_equals_predict_exact(name, targets):
    nc.check_impute_equals_blanket(backend(), name, targets)


def test_emu_malformed_plans_are_refused_alone_and_nothing_is_touched_outside_the_buffers():
    nc.check_malformed(backend())


def test_emu_argument_refusals():
    nc.check_argument_refusals(backend().lib)


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    nc.check_argument_refusals(dl.load())


@pytest.mark.parametrize("name", ("handfour", "wide3"))
def test_emu_exact_ties_and_a_table_beyond_the_register_accumulators(name):
    """handfour: exact ties, so the kernel's lowest-level rule decides; wide3: a family of 1280 cells, more than the 1024 a
    workgroup accumulates in registers"""
    nc.check_counts_bytes(backend(), name, 257, (0, 3))
    nc.check_impute_bytes(backend(), name, 257, (0, 3))


def test_emu_more_than_256_chunks_go_through_the_slots_of_the_tree():
    """65 537 rows of the three-variable network: larger than every other case on purpose — only beyond 256 chunks does a slot
    of the chunk tree and of the log-likelihood tree add more than one chunk value"""
    nc.check_counts_bytes(backend(), "hand", nc.MANY_CHUNKS_ROWS)
