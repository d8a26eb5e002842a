"""GPU: the Monte Carlo permutation CI tests (csrc/dvs_permtest.h) through the raw calls with the cases, restatement and checks
of tests/permtest_corpus.py — shared with the emulator twin tests/test_emu_permtest.py — plus the Python surface
(dags_vae_search_amd/pc.py: ci_tests, ci_test, pc_stable; local.py: what refuses them, rsmax2 through pc_stable)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pc_corpus as pc
from tests import permtest_corpus as pt
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _rows(t):
    return [int(v) for v in t.cpu().numpy().view(U64)]


@pytest.mark.parametrize("typ", pt.TYPES)
@pytest.mark.parametrize("S, B", pt.SHAPES)
def test_kernel_is_the_restatement(S, B, typ):
    worst = pt.check_kernel_is_restatement(backend(), S, B, typ, pc.P_RTOL)
    print(f"S {S} B {B} {typ}: worst relative sp p error {worst:.3e} (allowed {pc.P_RTOL:.1e})")


def test_klnk_table_and_log_paths_give_equal_bytes():
    pt.check_klnk_paths(backend())


def test_smc_stops():
    pt.check_smc_stops(backend())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    pt.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def test_ci_tests_surface_equals_the_raw_call():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, ci_test, ci_tests
    S, B = 300, 600
    data, _ = pt.perm_case(S)
    ev = BNLearnWrapper("ten", "bic", data=data)
    card = (data.max(0) + 1).astype(np.uint8)                       # the evaluator's own level counts
    be = backend()
    tests = pt.TESTS + pt.BAD[1:]
    pairs = torch.tensor([[x, y] for x, y, _ in tests], dtype=torch.int32, device="cuda")
    cond = torch.tensor(np.array([pc.mask_of(z) for _, _, z in tests], U64).view(np.int64), device="cuda")
    dh, ch = be.put(sc.pack(data)), be.put(card)
    for typ in pt.TYPES:
        raw = pt.run_perm(be, dh, ch, data.shape[1], S, tests, typ, B, alpha=0.1, seed=5, offset=3, max_cells=pc.MAX_CELLS)
        out, st, used = ci_tests(ev, pairs, cond, typ, B=B, seed=5, alpha=0.1, test_offset=3, return_status=True, return_used=True)
        assert out.is_cuda and out.dtype == torch.float64 and out.shape == (len(tests), 3) and int(st[0]) == raw.status == 16
        assert used.dtype == torch.int32 and used.cpu().numpy().tobytes() == raw.used.tobytes()
        assert out.cpu().numpy().tobytes() == raw.out.tobytes(), typ
        cut = ci_tests(ev, pairs, cond, typ, B=B, seed=5, alpha=0.1, test_offset=3, chunk=7)          # ragged chunks
        assert cut.cpu().numpy().tobytes() == raw.out.tobytes(), typ
        one, n_used = ci_test(ev, 6, 8, (7,), typ, B=B, seed=5, alpha=0.1, test_offset=3 + tests.index((6, 8, (7,))), return_used=True)
        assert one.cpu().numpy().tobytes() == raw.out[tests.index((6, 8, (7,)))].tobytes() and int(n_used) == raw.used[tests.index((6, 8, (7,)))]
    # the four asymptotic names: what they gave, down to the bytes, and no permutation keyword is read
    for typ in pc.TYPES:
        _, want, _ = pc.run_ci(be, dh, ch, data.shape[1], S, tests, typ, pc.MAX_CELLS)
        assert ci_tests(ev, pairs, cond, typ).cpu().numpy().tobytes() == want.tobytes()
        assert ci_tests(ev, pairs, cond, typ, B=7, seed=9).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="test must be one of"):
        ci_tests(ev, pairs, cond, "mc-g2")
    with pytest.raises(ValueError, match=r"B must be in \[1, 2\^20\]"):
        ci_tests(ev, pairs, cond, "mc-mi", B=0)
    with pytest.raises(ValueError, match=r"alpha must be in \(0, 1\) for smc-x2"):
        ci_tests(ev, pairs, cond, "smc-x2", alpha=1.0)
    with pytest.raises(ValueError, match="return_used goes with a permutation test"):
        ci_tests(ev, pairs, cond, "mi", return_used=True)
    assert ci_test(ev, 0, 1, (), "mi", B=3).cpu().numpy().tobytes() == ci_test(ev, 0, 1).cpu().numpy().tobytes()


def test_grouped_callers_refuse_permutation_tests():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, ci_tests_group, mmpc
    ev = BNLearnWrapper("asia", "bic", data=pc.e2e_data("asia", 300)[0])
    one = lambda v, dt: torch.tensor([v], dtype=dt, device="cuda")
    for typ in pt.TYPES:
        with pytest.raises(ValueError, match="mmpc: permutation tests are not built for the grouped kernel"):
            mmpc(ev, test=typ)
        with pytest.raises(ValueError, match="ci_tests_group: permutation tests are not built for the grouped kernel"):
            ci_tests_group(ev, one(0, torch.int32), one(0, torch.int64), one(6, torch.int64), typ)


def test_pc_stable_with_mc_mi_on_asia_equals_pc_over_the_restatement():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, pc_stable, rsmax2
    S, B, seed = 300, 256, 2821
    ev = BNLearnWrapper("asia", "bic", data=pc.e2e_data("asia", S)[0])
    ref = pt.pc_reference("asia", S, "mc-mi", B, seed, pc.ALPHA)
    r = pc_stable(ev, alpha=pc.ALPHA, test="mc-mi", B=B, seed=seed)
    print(f"asia S {S} mc-mi B {B}: tests per level {r.tests_per_level}, edges {sum(bin(a).count('1') for a in ref.adj) // 2}")
    assert r.tests_per_level == ref.tests_per_level and len(ref.tests_per_level) >= 2 and r.refused == 0
    assert _rows(r.skeleton) == ref.adj
    assert r.sepsets.cpu().numpy().view(U64).tobytes() == ref.sepset.tobytes()
    small = pc_stable(ev, alpha=pc.ALPHA, test="mc-mi", B=B, seed=seed, chunk=5)          # a function of the seed, not of the cut
    assert torch.equal(small.skeleton, r.skeleton) and torch.equal(small.sepsets, r.sepsets) and torch.equal(small.pdag, r.pdag)
    hybrid = rsmax2(ev, restrict="pc.stable", restrict_args=dict(test="mc-mi", B=B, seed=seed), maximize_args=dict(max_steps=20))
    assert torch.equal(hybrid.skeleton, r.skeleton)
    smc = pc_stable(ev, alpha=pc.ALPHA, test="smc-mi", B=B, seed=seed)      # the same draws, the same decisions: p > alpha <=> count >= E
    assert torch.equal(smc.skeleton, r.skeleton) and smc.tests_per_level == r.tests_per_level
    with pytest.raises(ValueError, match=r"alpha must be in \(0, 1\) for smc-mi"):
        pc_stable(ev, alpha=1.0, test="smc-mi")
