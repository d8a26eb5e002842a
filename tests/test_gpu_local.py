"""GPU: grouped CI tests and the MMPC round (csrc/dvs_local.h) through the raw calls with the cases, references and checks of
tests/local_corpus.py — shared with the emulator twin tests/test_emu_local.py — plus the Python surface
(dags_vae_search_amd/local.py): ci_tests_group, mmpc, rsmax2, mmhc."""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import local_corpus as lc
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
@pytest.mark.parametrize("S", pc.SAMPLE_COUNTS)
def test_grouped_cells_are_the_bytes_of_the_per_test_kernel(S, typ):
    assert lc.check_group_equal_bytes(backend(), S, typ) == 80


def test_grouped_refusals():
    lc.check_group_refusals(backend())


def test_grouped_wide_rows():
    assert lc.check_group_wide(backend()) == 6 * 47


def test_mmpc_update_hand_made_rounds():
    lc.check_update_hand(backend())


@pytest.mark.parametrize("n, seed", [(1, 2711), (7, 2712), (48, 2713), (48, 2714)])
def test_mmpc_update_seeded_rounds(n, seed):
    lc.check_update_seeded(backend(), n, seed)


@pytest.mark.parametrize("name, S, typ", lc.E2E_CASES)
def test_mmpc_end_to_end_through_the_raw_abi(name, S, typ):
    lc.check_e2e_raw(backend(), name, S, typ)


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    lc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def test_ci_tests_group_surface_equals_the_raw_call():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, ci_tests_group
    case = pc.ci_case("sixS1000")
    ev = BNLearnWrapper("six", "bic", data=case.data)
    card = (case.data.max(0) + 1).astype(np.uint8)                  # the evaluator's own level counts
    be = backend()
    groups = lc.six_groups()[:9] + [(2, (), 0b000101)]
    targets = torch.tensor([y for y, _, _ in groups], dtype=torch.int32, device="cuda")
    cond = torch.tensor([pc.mask_of(z) for _, z, _ in groups], dtype=torch.int64, device="cuda")
    cands = torch.tensor([c for _, _, c in groups], dtype=torch.int64, device="cuda")
    for typ, lds in (("mi", None), ("x2-adf", 3072)):
        _, raw, status = lc.run_group(be, be.put(sc.pack(case.data)), be.put(card), 6, 1000, groups, typ, lds or lc.MAX_CELLS)
        out, st = ci_tests_group(ev, targets, cond, cands, typ, lds_cells=lds, return_status=True)
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (len(groups), 6, 3) and int(st[0]) == status == 16
        assert out.cpu().numpy().tobytes() == raw.tobytes()
    assert ci_tests_group(ev, targets, cond, cands).cpu().numpy().tobytes() == ci_tests_group(ev, targets, cond, cands, "mi").cpu().numpy().tobytes()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ci_tests_group(ev, targets.cpu(), cond, cands)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ci_tests_group(ev, targets, cond, cands.cpu())
    with pytest.raises(TypeError, match="candidates must be a torch tensor"):
        ci_tests_group(ev, targets, cond, [1, 2])
    with pytest.raises(ValueError, match="test must be one of"):
        ci_tests_group(ev, targets, cond, cands, "g2")
    with pytest.raises(ValueError, match=r"targets must be int32 \[G >= 1\]"):
        ci_tests_group(ev, targets.to(torch.int64), cond, cands)
    with pytest.raises(ValueError, match=r"cond must be int64 \[10\] bit masks"):
        ci_tests_group(ev, targets, cond[:3], cands)
    with pytest.raises(ValueError, match=r"lds_cells must be in \[1, 36864\]"):
        ci_tests_group(ev, targets, cond, cands, lds_cells=0)


def test_mmpc_on_asia_equals_the_raw_driver():
    import torch
    from dags_vae_search_amd import MMPCResult, mmpc
    data, card = pc.e2e_data("asia", 5000)
    ev = evaluator("asia", 5000)
    raw = lc.mmpc_raw(backend(), data, card, "mi")
    r = mmpc(ev, alpha=pc.ALPHA, test="mi")
    assert isinstance(r, MMPCResult) and r.skeleton.is_cuda and r.skeleton.dtype == torch.int64 and r.sepsets.shape == (8, 8)
    got = SimpleNamespace(forward=_rows(r.forward), cpc=_rows(r.cpc), skeleton=_rows(r.skeleton), sepset=r.sepsets.cpu().numpy().view(U64),
                             groups_per_round=r.groups_per_round, refused=r.refused, asymmetric=r.asymmetric)
    lc.assert_same_mmpc(got, raw, "mmpc")
    assert r.groups_per_round == [8, 7, 10, 4, 29] and got.skeleton == [0, 24, 32, 34, 130, 12, 0, 16]
    for cap in (0, 1):
        capped = mmpc(ev, max_cond=cap)
        want = lc.mmpc_raw(backend(), data, card, "mi", max_cond=cap)
        assert (_rows(capped.cpc), _rows(capped.skeleton), capped.groups_per_round) == (want.cpc, want.skeleton, want.groups_per_round)
    some = mmpc(ev, targets=[1, 3, 4])
    assert _rows(some.cpc)[1] == got.cpc[1] and _rows(some.cpc)[0] == 0 and _rows(some.skeleton)[1] == got.skeleton[1] & 0b11010
    with pytest.raises(ValueError, match=r"alpha must be in \[0, 1\]"):
        mmpc(ev, alpha=1.5)
    with pytest.raises(ValueError, match="max_cond must be >= 0"):
        mmpc(ev, max_cond=-1)
    with pytest.raises(ValueError, match="test must be one of"):
        mmpc(ev, test="g2")
    with pytest.raises(ValueError, match=r"targets must name variables in \[0, 8\)"):
        mmpc(ev, targets=[8])


def test_mmhc_is_mmpc_then_a_hill_climb_inside_the_skeleton():
    import torch
    from dags_vae_search_amd import RSMAX2Result, hill_climb, mmhc, mmpc, skeleton_blacklist
    case = hc.hc_case("asia")
    ev = evaluator("asia", 5000)
    kw = dict(max_steps=case.max_steps, min_delta=case.min_delta)
    r = mmhc(ev, maximize_args=kw)
    restricted = mmpc(ev)
    by_hand = hill_climb(ev, batch=1, forbidden=skeleton_blacklist(restricted.skeleton), **kw)
    assert isinstance(r, RSMAX2Result) and torch.equal(r.skeleton, restricted.skeleton) and torch.equal(r.restrict.cpc, restricted.cpc)
    assert torch.equal(r.search.parents, by_hand.parents) and r.search.scores.cpu().numpy().tobytes() == by_hand.scores.cpu().numpy().tobytes()
    assert torch.equal(r.search.steps, by_hand.steps)
    rows, skel = _rows(r.search.parents[0]), _rows(r.skeleton)
    assert any(rows) and all(rows[v] & ~skel[v] == 0 for v in range(ev.n_vars))


def test_rsmax2_with_pc_stable_and_tabu_is_its_hand_composition():
    import torch
    from dags_vae_search_amd import pc_stable, rsmax2, skeleton_blacklist, tabu_search
    case = hc.hc_case("asia")
    ev = evaluator("asia", 5000)
    kw = dict(max_steps=case.max_steps, tabu=5)
    r = rsmax2(ev, restrict="pc.stable", maximize="tabu", restrict_args=dict(test="x2", max_cond=2), maximize_args=kw)
    restricted = pc_stable(ev, test="x2", max_cond=2)
    by_hand = tabu_search(ev, batch=1, forbidden=skeleton_blacklist(restricted.skeleton), **kw)
    assert torch.equal(r.skeleton, restricted.skeleton) and torch.equal(r.restrict.pdag, restricted.pdag)
    assert torch.equal(r.search.parents, by_hand.parents) and r.search.scores.cpu().numpy().tobytes() == by_hand.scores.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match="restrict must be one of"):
        rsmax2(ev, restrict="iamb")
    with pytest.raises(ValueError, match="maximize must be one of"):
        rsmax2(ev, maximize="sa")
    with pytest.raises(ValueError, match="forbidden is the learned skeleton's blacklist"):
        rsmax2(ev, maximize_args=dict(forbidden=None))
