"""GPU: constraint-based structure learning (csrc/dvs_citest.h) through the raw calls with the cases, references and checks of
tests/pc_corpus.py — shared with the emulator twin tests/test_emu_pc.py — plus the Python surface
(dags_vae_search_amd/pc.py): ci_tests, ci_test, pc_stable, skeleton_blacklist."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import pc_corpus as pc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@functools.lru_cache(maxsize=None)
def evaluator(name, S):
    from dags_vae_search_amd import BNLearnWrapper
    return BNLearnWrapper(name, "bic", data=pc.e2e_data(name, S)[0])


def _rows(t):
    return [int(v) for v in t.cpu().numpy().view(U64)]


@pytest.mark.parametrize("typ", pc.TYPES)
@pytest.mark.parametrize("name", pc.CI_CASE_NAMES)
def test_ci_statistic_df_and_p_value(name, typ):
    pc.check_ci_case(backend(), name, typ)


def test_ci_max_cells_refuses_the_larger_tables_only():
    pc.check_ci_max_cells(backend())


def test_pc_expand_equals_sorted_combinations():
    assert pc.check_expand(backend()) > 1000


def test_pc_reduce_hand_made_levels():
    pc.check_reduce(backend())


@pytest.mark.parametrize("n", [3, 4, 5])
def test_pc_orient_with_a_dsep_oracle_gives_the_cpdag_of_every_dag(n):
    assert pc.check_orient_all_dags(backend(), n) == pc.cp.DAG_COUNTS[n]


def test_pc_orient_conflicts_cycle_and_illegal_rows():
    pc.check_orient_hand(backend())


def test_pc_stable_through_the_raw_calls():
    pc.check_e2e_raw(backend(), "asia", 5000, "mi")


@pytest.mark.parametrize("name,S,typ", pc.E2E_CASES)
def test_pc_stable_equals_the_restatement(name, S, typ):
    import torch
    from dags_vae_search_amd import PCResult, pc_stable
    ref = pc.check_guard(name, S, typ)
    r = pc_stable(evaluator(name, S), alpha=pc.ALPHA, test=typ)
    assert isinstance(r, PCResult) and r.pdag.is_cuda and r.skeleton.dtype == torch.int64 and r.sepsets.shape == (ref.sepset.shape)
    got = SimpleNamespace(adj=_rows(r.skeleton), sepset=r.sepsets.cpu().numpy().view(U64), tests_per_level=r.tests_per_level,
                          pdag=_rows(r.pdag), conflicts=r.conflicts, flag=r.flags)
    assert r.refused == 0
    pc.assert_same_result(got, ref, (name, S, typ))
    if (name, S, typ) == ("sachs", 5000, "mi"):
        small = pc_stable(evaluator(name, S), alpha=pc.ALPHA, test=typ, chunk=100)          # ragged chunks: the same bytes
        assert torch.equal(small.pdag, r.pdag) and torch.equal(small.sepsets, r.sepsets) and small.tests_per_level == r.tests_per_level
        capped = pc_stable(evaluator(name, S), alpha=pc.ALPHA, test=typ, max_cond=2)
        assert capped.tests_per_level == ref.tests_per_level[:3]


def test_ci_tests_surface_equals_the_raw_call():
    import torch
    from dags_vae_search_amd import ci_test, ci_tests
    case = pc.ci_case("sixS1000")
    from dags_vae_search_amd import BNLearnWrapper
    ev = BNLearnWrapper("six", "bic", data=case.data)
    card = (case.data.max(0) + 1).astype(np.uint8)                  # the evaluator's own level counts
    be = backend()
    tests = pc.SIX_TESTS[:8] + [(2, 2, ())]
    for typ in ("mi", "x2-adf"):
        _, raw, status = pc.run_ci(be, be.put(sc.pack(case.data)), be.put(card), 6, 1000, tests, typ, pc.MAX_CELLS)
        pairs = torch.tensor([[x, y] for x, y, _ in tests], dtype=torch.int32, device="cuda")
        cond = torch.tensor([pc.mask_of(z) for _, _, z in tests], dtype=torch.int64, device="cuda")
        out, st = ci_tests(ev, pairs, cond, typ, return_status=True)
        assert out.is_cuda and out.dtype == torch.float64 and int(st[0]) == status == 16
        assert out.cpu().numpy().tobytes() == raw.tobytes()
        assert ci_tests(ev, pairs, cond, typ, chunk=4).cpu().numpy().tobytes() == raw.tobytes()
        one = ci_test(ev, 3, 0, (1, 2, 5), typ)
        assert one.shape == (3,) and one.cpu().numpy().tobytes() == raw[6].tobytes()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ci_tests(ev, pairs.cpu(), cond, "mi")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ci_tests(ev, pairs, cond.cpu(), "mi")
    with pytest.raises(ValueError, match="test must be one of"):
        ci_tests(ev, pairs, cond, "g2")
    with pytest.raises(ValueError):
        ci_tests(ev, pairs.to(torch.int64), cond, "mi")


def test_skeleton_blacklist_restricts_hill_climb():
    import torch
    from dags_vae_search_amd import hill_climb, pc_stable, skeleton_blacklist
    case = hc.hc_case("asia")
    ev = evaluator("asia", 5000)
    n = ev.n_vars
    r = pc_stable(ev, alpha=pc.ALPHA, test="mi")
    forb = skeleton_blacklist(r.skeleton)
    skel = _rows(r.skeleton)
    assert _rows(forb) == [((1 << n) - 1) & ~(1 << v) & ~skel[v] for v in range(n)]
    kw = dict(batch=1, max_steps=case.max_steps, min_delta=case.min_delta)
    inside = hill_climb(ev, forbidden=forb, **kw)
    rows = _rows(inside.parents[0])
    assert any(rows) and all(rows[v] & ~skel[v] == 0 for v in range(n))
    free = hill_climb(ev, **kw)
    assert any(fr & ~sk for fr, sk in zip(_rows(free.parents[0]), skel))       # the restriction decided something
    complete = torch.tensor([((1 << n) - 1) & ~(1 << v) for v in range(n)], dtype=torch.int64, device="cuda")
    assert not skeleton_blacklist(complete).any()
    same = hill_climb(ev, forbidden=skeleton_blacklist(complete), **kw)
    assert torch.equal(same.parents, free.parents) and same.scores.cpu().numpy().tobytes() == free.scores.cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="no CPU path"):
        skeleton_blacklist(r.skeleton.cpu())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    pc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
