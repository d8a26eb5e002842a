"""GPU: structure comparison (csrc/dvs_cpdag.h) through the raw calls with the cases, references and checks of
tests/cpdag_corpus.py — shared with the emulator twin tests/test_emu_cpdag.py — plus the Python surface
(dags_vae_search_amd/compare.py): cpdag, compare_structures, shd, equivalence_classes."""
import ctypes
import functools

import numpy as np
import pytest

from tests import cpdag_corpus as cp
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def driver():
    from dags_vae_search_amd import _lib as dl
    return cp.Driver(sc.GpuBackend(dl.load()))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, U64).view(np.int64).copy()).cuda()


def _rows(t):
    return t.cpu().numpy().view(U64)


@pytest.mark.parametrize("n", [4, 5])
def test_cpdag_all_labelled_dags(n):
    """all 543 and all 29 281, each as one launch"""
    assert cp.check_all_dags(driver(), n) == cp.DAG_COUNTS[n]


@pytest.mark.parametrize("n", cp.RANDOM_SIZES)
def test_cpdag_random_dags_in_permuted_order(n):
    print(f"\ndevice n = {n}: rules fired {sorted(cp.check_random(driver(), n))}")


def test_cpdag_complete_order_and_empty_graph():
    cp.check_extremes(driver())


@pytest.mark.parametrize("n", [33, 48])
def test_cpdag_is_unchanged_by_a_covered_edge_reversal(n):
    cp.check_covered_edge(driver(), n)


def test_cpdag_flags_sit_between_clean_rows():
    cp.check_flags(driver())


def test_pdag_compare_hand_made_pairs():
    cp.check_compare_hand(driver())


@pytest.mark.parametrize("n", [5, 33, 48])
def test_pdag_compare_random_pairs(n):
    assert cp.check_compare_random(driver(), n) > 0


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    cp.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ---------------------------------------------------------------------------------------------
def test_shd_of_a_batch_with_itself_and_with_a_covered_edge_reversed():
    import torch
    from dags_vae_search_amd import StructureComparison, compare_structures, shd
    P = cp.random_dags(33, 24, cp.SPARSE(33), seed=77 + 33)
    Q = P.copy()
    changed = []
    for b in range(len(P)):
        cov = cp.covered_edges(P[b])
        if cov:
            Q[b] = np.array(cp.reverse_edge(P[b], *cov[0]), U64)
            changed.append(b)
    assert len(changed) >= 12
    x, y = _t(P), _t(Q)
    kept = x.clone(), y.clone()
    assert not bool(shd(x, x).any()) and not bool(shd(x, x, equivalence=False).any())
    r = compare_structures(y, x)
    assert isinstance(r, StructureComparison) and all(f.dtype == torch.int32 and f.shape == (24,) and f.is_cuda for f in r)
    assert not bool(r.shd.any()) and not bool(r.fp.any()) and not bool(r.fn.any()) and not bool(r.hamming.any())
    assert r.tp.cpu().tolist() == [cp.n_edges(row) for row in P]
    raw = compare_structures(y, x, equivalence=False)
    want = [1 if b in changed else 0 for b in range(len(P))]
    assert raw.shd.cpu().tolist() == want == raw.fp.cpu().tolist() == raw.fn.cpu().tolist() and not bool(raw.hamming.any())
    assert torch.equal(shd(y, x, equivalence=False), raw.shd)
    assert torch.equal(x, kept[0]) and torch.equal(y, kept[1])              # the caller's tensors are untouched
    # one target for the batch: [n] and [1, n] are the tiled target
    one = compare_structures(y, x[3])
    assert all(torch.equal(f, g) for f, g in zip(one, compare_structures(y, x[3:4].expand(24, -1).contiguous())))
    assert all(torch.equal(f, g) for f, g in zip(one, compare_structures(y, x[3:4])))
    assert int(one.shd[3]) == 0


@pytest.mark.parametrize("n", [4, 5])
def test_equivalence_classes_of_all_labelled_dags(n):
    import torch
    from dags_vae_search_amd import cpdag, equivalence_classes
    dags = cp.as_rows(cp.all_dags(n))
    class_of, reps = equivalence_classes(_t(dags))
    assert reps.shape == (cp.CLASS_COUNTS[n], n) and class_of.shape == (len(dags),) and class_of.dtype == torch.int64
    ref = [tuple(rows) for rows, _ in cp.ref_all(n)]
    got = [tuple(int(x) for x in row) for row in _rows(reps)]
    ids = class_of.cpu().tolist()
    assert all(got[ids[b]] == ref[b] for b in range(len(dags)))             # class_of agrees with cpdag_ref
    assert len(set(ref)) == cp.CLASS_COUNTS[n]
    assert _rows(cpdag(_t(dags))).tobytes() == cp.as_rows(ref).tobytes()


def test_hill_climb_result_against_the_known_asia_network():
    from dags_vae_search_amd import BNLearnWrapper, compare_structures, hill_climb
    case = hc.hc_case("asia")
    ev = BNLearnWrapper("asia", "bic", data=case.data)
    res = hill_climb(ev, batch=3, max_steps=case.max_steps, min_delta=case.min_delta)
    target = sc.masks_of(8, hc.ASIA_KNOWN)
    learned = _rows(res.parents)
    for eq in (True, False):
        got = compare_structures(res.parents, _t(target)[0], equivalence=eq)
        a = [cp.cpdag_ref(row)[0] for row in learned] if eq else learned
        t = cp.cpdag_ref(target[0])[0] if eq else target[0]
        want = [cp.compare_ref(row, t) for row in a]
        assert [tuple(int(f[b]) for f in got) for b in range(3)] == want
        print(f"\nasia, hill_climb from the empty graph, equivalence={eq}: shd, tp, fp, fn, hamming = {want[0]}")
    assert want[0][1] + want[0][3] == cp.n_edges(target[0]) == 9            # tp + fn: the arcs of the known network


def test_refusals_determinism_and_a_batch_is_its_rows():
    import torch
    from dags_vae_search_amd import compare_structures, cpdag, equivalence_classes
    P = cp.random_dags(17, 40, 0.5, seed=9)
    x = _t(P)
    bad = x.clone()
    bad[5] = 0
    bad[5, 0], bad[5, 1] = 1 << 1, 1 << 0                                   # 0 <-> 1
    bad[9, 3] |= 1 << 20                                                    # a parent bit >= n
    with pytest.raises(ValueError, match=r"cpdag: parents with a cycle: rows \[5\]; .* rows \[9\]"):
        cpdag(bad)
    with pytest.raises(ValueError, match=r"compare_structures: target with a cycle: rows \[5\]"):
        compare_structures(x, bad)
    compare_structures(x, bad, equivalence=False)                           # masks as given are not judged
    for fn in (cpdag, equivalence_classes, lambda t: compare_structures(t, t), lambda t: compare_structures(x, t)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(x.cpu())
    with pytest.raises(ValueError):
        compare_structures(x, x[:7])
    with pytest.raises(ValueError):
        cpdag(x.to(torch.int32))
    a, b = cpdag(x), cpdag(x)
    assert torch.equal(a, b) and torch.equal(cpdag(x[:7]), a[:7]) and torch.equal(cpdag(x[11:12]), a[11:12])
    r, s = compare_structures(x, x[2]), compare_structures(x, x[2])
    head = compare_structures(x[:7], x[2])
    assert all(torch.equal(f, g) for f, g in zip(r, s)) and all(torch.equal(f[:7], g) for f, g in zip(r, head))
