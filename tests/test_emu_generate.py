"""CPU: dvs_generate_dags (csrc/dvs_generate.h) on the host emulator, through the C ABI, bit for bit against the numpy
restatement of its specification (tests/generate_corpus.py) — the same cases as tests/test_gpu_generate.py."""
import numpy as np
import pytest

from dags_vae_search_amd import _lib as dl
from tests import generate_corpus as gc
from tests.emu.harness import emu, ptr


def run(n, card, num_edges, *, seed, dag_offset=0, try_limit=100, flags=0):
    return gc.run_abi(emu(), ptr, n, card, num_edges, seed=seed, dag_offset=dag_offset, try_limit=try_limit, flags=flags)


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_case_equals_the_restatement(name):
    gc.check_case(run, name)


@pytest.mark.parametrize("group", [1, 2, 4, 7])
@pytest.mark.parametrize("name", ["n5_m5", "n8_m7_try2", "n12_mixed", "n14_m20", "n8_m_out_of_range"])
def test_lane_mapping_does_not_matter(name, group):
    """1, 2, 8 and 64 lanes per DAG (flags bits 8..11): the first accepted attempt in attempt order, whatever the mapping."""
    gc.check_case(run, name, group)


def test_sharding():
    gc.check_sharding(run)


def test_determinism_and_seed():
    gc.check_determinism(run)


def test_abi_refusals():
    gc.check_refusals(emu(), ptr, lambda nbytes: np.zeros(nbytes, np.uint8))


def test_edge_count_draws():
    """dvs_generate_edge_counts: entry i with weight (i + 1)^2, from site 302 of the global DAG index."""
    lib = emu()
    schema = [(11 + i, (i + 1) ** 2) for i in range(16)]
    counts = np.asarray([m for m, _ in schema], np.int32)
    cum = np.cumsum([w for _, w in schema]).astype(np.int32)
    B = 30000
    out = np.zeros(B, np.int32)
    dl.check(lib, lib.dvs_generate_edge_counts(B, 16, ptr(counts), ptr(cum), 5, 100, ptr(out), None), "edge counts")
    key = gc.rng.site_key(5, 302, np.arange(B, dtype=np.uint64) + np.uint64(100))
    r = (gc.rng.draw(key, np.uint64(0)) * np.uint64(cum[-1])) >> np.uint64(32)
    assert np.array_equal(out, counts[np.searchsorted(cum, r.astype(np.int64), side="right")])
    exp = B * np.asarray([w for _, w in schema]) / cum[-1]
    chi2 = ((np.bincount(out - 11, minlength=16) - exp) ** 2 / exp).sum()
    assert chi2 < 37.7                                         # 15 d.o.f., 99.9 %
    tail = np.zeros(50, np.int32)
    dl.check(lib, lib.dvs_generate_edge_counts(50, 16, ptr(counts), ptr(cum), 5, 150, ptr(tail), None), "edge counts")
    assert np.array_equal(tail, out[50:100])
