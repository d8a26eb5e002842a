"""Exact inference by variable elimination (csrc/dvs_eliminate.h: dvs_bn_eliminate) on the host emulator through the raw C ABI:
every case, reference and check comes from tests/eliminate_corpus.py, which tests/test_gpu_eliminate.py runs unchanged on the
device."""
import functools

import pytest

from tests import eliminate_corpus as ec
from tests import scoring_corpus as sc


@functools.lru_cache(maxsize=None)
def backend():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("n_rows", ec.ROW_COUNTS)
@pytest.mark.parametrize("name", ec.NETWORKS)
def test_emu_eliminate_equals_the_restatement(name, n_rows):
    ec.check_bytes(backend(), name, n_rows)


@pytest.mark.parametrize("name", ("hand", "six", "asia", "band48"))
def test_emu_rows_per_group_does_not_change_the_bytes(name):
    ec.check_rows_per_group(backend(), name)


def test_emu_loop_shapes():
    ec.check_loop_shapes(backend())


def test_emu_malformed_plans_are_refused_alone_and_nothing_is_touched_outside_the_buffers():
    ec.check_malformed(backend())


@pytest.mark.parametrize("name,targets", (("asia", (1, 4, 7)), ("band48", (0, 23, 47))))
def test_emu_every_other_variable_observed_equals_the_blanket_posterior(name, targets):
    ec.check_blanket_crosscheck(backend(), name, targets)


def test_emu_argument_refusals():
    ec.check_argument_refusals(backend().lib)


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    ec.check_argument_refusals(dl.load())
