"""GPU: the Gaussian CI tests (csrc/dvs_gaussian_ci.h) through the raw calls with the cases, references and checks of
tests/gaussian_ci_corpus.py — shared with the emulator twin tests/test_emu_gaussian_ci.py — plus the Python surface: ci_tests,
ci_test, ci_tests_group, pc_stable, mmpc, rsmax2 and mmhc on a GaussianEvaluator, and the ValueErrors in both directions."""
import ctypes
import functools

import numpy as np
import pytest

from tests import gaussian_ci_corpus as gi
from tests import gaussian_corpus as gc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _masks(t):
    return [int(v) for v in t.cpu().numpy().view(U64).ravel()]


def _evaluator(n, S, metric="bic-g"):
    from dags_vae_search_amd import GaussianEvaluator
    return GaussianEvaluator(f"syn{n}", metric, data=gc.gauss_data(n, S))


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("T", gi.T_VALUES)
@pytest.mark.parametrize("n, S", gi.DATA_SHAPES)
def test_tests_against_mpmath(n, S, T):
    ws, wp = gi.check_against_mpmath(backend(), n, S, T)
    print(f"n {n} S {S} T {T}: worst statistic error / bound {ws:.3e}, worst p error / bound {wp:.3e}")


def test_four_rows_leave_cor_one_degree_of_freedom_and_zf_none():
    gi.check_short_set(backend())


def test_refusals_between_sentinels():
    gi.check_refusals(backend())


@pytest.mark.parametrize("n, S", gi.DATA_SHAPES)
def test_grouped_cells_are_the_per_test_bytes(n, S):
    cells = gi.check_group_equal_bytes(backend(), n, S)
    print(f"n {n}: {cells} grouped cells equal to dvs_gbn_ci_tests as bytes")


def test_row_sets_are_the_gathered_rows_bytes():
    gi.check_row_sets(backend())


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_pc_stable_raw_equals_the_restatement(n, S, typ):
    got = gi.check_pc_raw(backend(), n, S, typ)
    assert sum(got.tests_per_level) == {5: 30, 8: 72, 17: 949}[n]


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_mmpc_raw_equals_the_restatement(n, S, typ):
    gi.check_mmpc_raw(backend(), n, S, typ)


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    gi.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def _tensors(torch, tests):
    pairs = torch.tensor([[t[0], t[1]] for t in tests], dtype=torch.int32, device="cuda")
    cond = torch.from_numpy(np.asarray([gc.mask_of(t[2]) for t in tests], U64).view(np.int64)).cuda()
    return pairs, cond


@pytest.mark.parametrize("typ", gi.TYPES)
def test_ci_tests_and_ci_tests_group_equal_the_raw_calls(typ):
    import torch
    from dags_vae_search_amd import ci_test, ci_tests, ci_tests_group
    n, S = 17, 389
    be, ev = backend(), _evaluator(n, S)
    mom = gc.run_moments(be, gc.gauss_data(n, S))
    tests = gi.cycled(gi.pool(n), 65) + [(3, 3, ())]
    pairs, cond = _tensors(torch, tests)
    want, want_status = gi.run_ci(be, mom, n, tests, typ)
    got, status = ci_tests(ev, pairs, cond, typ, return_status=True)
    assert got.cpu().numpy().tobytes() == want.tobytes() and int(status[0]) == want_status == 16
    assert ci_tests(ev, pairs, cond, typ, chunk=7).cpu().numpy().tobytes() == want.tobytes()
    x, y, Z = tests[7]
    assert ci_test(ev, x, y, Z, test=typ).cpu().numpy().tobytes() == want[7].tobytes()
    assert ci_test(ev, 0, 1, (2,), test=typ).cpu().numpy().tobytes() == gi.run_ci(be, mom, n, [(0, 1, (2,))], typ)[0][0].tobytes()
    groups = gi.group_cases(n)
    gwant, gstatus = gi.run_group(be, mom, n, groups, typ)
    targets = torch.tensor([g[0] for g in groups], dtype=torch.int32, device="cuda")
    gcond = torch.from_numpy(np.asarray([gc.mask_of(g[1]) for g in groups], U64).view(np.int64)).cuda()
    cand = torch.from_numpy(np.asarray([g[2] for g in groups], U64).view(np.int64)).cuda()
    ggot, gst = ci_tests_group(ev, targets, gcond, cand, typ, return_status=True)
    assert ggot.cpu().numpy().tobytes() == gwant.tobytes() and int(gst[0]) == gstatus
    # a row-set view: test t on set t, or on set_of[t]
    rows = gc.row_sets(S, 150, n_sets=len(tests))
    sets = gc.run_moments(be, gc.gauss_data(n, S), rows)
    view = ev.with_rows(torch.from_numpy(rows).cuda())
    assert ci_tests(view, pairs, cond, typ).cpu().numpy().tobytes() == gi.run_ci(be, sets, n, tests, typ, set_of=np.arange(len(tests)))[0].tobytes()
    set_of = (np.arange(len(tests), dtype=np.int32) * 5) % 3
    view = ev.with_rows(torch.from_numpy(rows[:3]).cuda(), torch.from_numpy(set_of))
    assert ci_tests(view, pairs, cond, typ).cpu().numpy().tobytes() == gi.run_ci(be, sets[:3], n, tests, typ, set_of=set_of)[0].tobytes()
    with pytest.raises(ValueError, match="structures but 3 row sets"):
        ci_tests(ev.with_rows(torch.from_numpy(rows[:3]).cuda()), pairs, cond, typ)


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_pc_stable_equals_the_restatement(n, S, typ):
    from dags_vae_search_amd import pc_stable
    ref = gi.check_pc_guard(n, S, typ)
    res = pc_stable(_evaluator(n, S), test=typ, chunk=97)
    assert res.tests_per_level == ref.tests_per_level and res.refused == 0
    assert _masks(res.skeleton) == ref.adj and res.sepsets.cpu().numpy().view(U64).tobytes() == ref.sepset.tobytes()
    assert (_masks(res.pdag), res.conflicts, res.flags) == (ref.pdag, ref.conflicts, ref.flag)


@pytest.mark.parametrize("typ", gi.TYPES)
@pytest.mark.parametrize("n, S", gi.E2E_SHAPES)
def test_mmpc_equals_the_restatement(n, S, typ):
    from dags_vae_search_amd import mmpc
    ref = gi.check_mmpc_guard(n, S, typ)
    res = mmpc(_evaluator(n, S), test=typ)
    assert res.groups_per_round == ref.groups_per_round and (res.refused, res.asymmetric) == (ref.refused, ref.asymmetric)
    assert _masks(res.forward) == ref.forward and _masks(res.cpc) == ref.cpc and _masks(res.skeleton) == ref.skeleton
    assert res.sepsets.cpu().numpy().view(U64).tobytes() == ref.sepset.tobytes()


def test_conditioning_sets_beyond_the_cap_are_refused_and_counted():
    """alpha = 1 removes nothing, so PC-stable on 13 variables reaches level 11, one above DVS_GCI_MAX_COND: its 2 * 78 tests
    come back refused, are counted, and no edge leaves on their account"""
    import torch
    from dags_vae_search_amd import ci_tests_group, pc_stable
    from dags_vae_search_amd import _lib as dl
    n = 13
    ev = _evaluator(n, 389)
    res = pc_stable(ev, alpha=1.0, test="zf", max_cond=dl.GCI_MAX_COND + 2)
    assert len(res.tests_per_level) == 12 and res.tests_per_level[11] == 156 and res.refused == 156
    assert _masks(res.skeleton) == [((1 << n) - 1) & ~(1 << v) for v in range(n)]
    out, status = ci_tests_group(ev, torch.tensor([12], dtype=torch.int32, device="cuda"),
                                 torch.tensor([(1 << 11) - 1], dtype=torch.int64, device="cuda"),
                                 torch.tensor([1 << 11], dtype=torch.int64, device="cuda"), "cor", return_status=True)
    assert int(status[0]) == 16 and bool(torch.isnan(out).all())


def test_restrict_then_maximise_on_real_data_is_the_blacklisted_climb():
    from dags_vae_search_amd import hill_climb, mmhc, mmpc, pc_stable, rsmax2, skeleton_blacklist
    n, S = 8, 389
    ev = _evaluator(n, S, "bic-g")
    for got, skeleton in ((rsmax2(ev, restrict="pc.stable", restrict_args={"test": "zf"}), pc_stable(ev, test="zf").skeleton),
                          (mmhc(ev, restrict_args={"test": "cor"}), mmpc(ev, test="cor").skeleton)):
        assert got.skeleton.cpu().numpy().tobytes() == skeleton.cpu().numpy().tobytes() and got.restrict.refused == 0
        want = hill_climb(ev, forbidden=skeleton_blacklist(skeleton), max_steps=max(16, n * n), batch=1)
        assert got.search.parents.cpu().numpy().tobytes() == want.parents.cpu().numpy().tobytes()
        assert got.search.scores.cpu().numpy().tobytes() == want.scores.cpu().numpy().tobytes()
        assert int(want.steps[0]) > 0
        adj = _masks(skeleton)
        assert all(not (m & ~adj[v]) for v, m in enumerate(_masks(got.search.parents)))       # every arc lies in the skeleton


def test_value_errors_in_both_directions():
    import torch
    from dags_vae_search_amd import BNLearnWrapper, ci_test, ci_tests, ci_tests_group, mmhc, mmpc, pc_stable, rsmax2
    n, S = 5, 129
    ev = _evaluator(n, S)
    rng = np.random.default_rng(3)
    disc = BNLearnWrapper("disc5", "bic", data=rng.integers(0, 3, (200, n)))
    pairs, cond = _tensors(torch, [(0, 1, ())])
    one = lambda v, dt: torch.tensor([v], dtype=dt, device="cuda")
    group = lambda e, t: ci_tests_group(e, one(0, torch.int32), one(0, torch.int64), one(6, torch.int64), t)
    # a discrete or permutation test name on a Gaussian evaluator: need_discrete's message, now naming the Gaussian tests
    for name in ("mi", "x2-adf", "mc-mi", "smc-x2"):
        calls = {"ci_tests": lambda: ci_tests(ev, pairs, cond, name), "ci_test": lambda: ci_test(ev, 0, 1, (), name),
                 "pc_stable": lambda: pc_stable(ev, test=name), "mmpc": lambda: mmpc(ev, test=name),
                 "ci_tests_group": lambda: group(ev, name)}
        if name.startswith(("mc-", "smc-")):
            calls = {k: calls[k] for k in ("ci_tests", "ci_test", "pc_stable")}          # the grouped kernel refuses them first
        for what, fn in calls.items():
            with pytest.raises(ValueError, match=f"{what}: the evaluator holds real-valued data .*\"cor\", \"zf\" and \"mi-g\".* Gaussian "
                                                 f"counterpart is not built"):
                fn()
    with pytest.raises(ValueError, match="mmpc: the evaluator holds real-valued data"):
        mmhc(ev)
    with pytest.raises(ValueError, match="pc_stable: the evaluator holds real-valued data"):
        rsmax2(ev, restrict="pc.stable")
    # a Gaussian test name on a discrete evaluator
    for name in gi.TYPES:
        for what, fn in {"ci_tests": lambda: ci_tests(disc, pairs, cond, name), "ci_test": lambda: ci_test(disc, 0, 1, (), name),
                         "pc_stable": lambda: pc_stable(disc, test=name), "mmpc": lambda: mmpc(disc, test=name),
                         "ci_tests_group": lambda: group(disc, name),
                         "mmpc ": lambda: mmhc(disc, restrict_args={"test": name})}.items():
            with pytest.raises(ValueError, match=f"{what.strip()}: test '{name}' reads real-valued data and the evaluator holds discrete levels"):
                fn()
    # an unknown name, on either evaluator: the old wording, the Gaussian names in the list
    for e in (ev, disc):
        for fn in (lambda: ci_tests(e, pairs, cond, "fisher"), lambda: pc_stable(e, test="fisher"), lambda: mmpc(e, test="fisher"),
                   lambda: group(e, "fisher")):
            with pytest.raises(ValueError, match=r"test must be one of \[.*'mi'.*'mc-mi'.*'cor', 'mi-g', 'zf'\] \(got 'fisher'\)"):
                fn()
    with pytest.raises(ValueError, match="return_used goes with a permutation test"):
        ci_tests(ev, pairs, cond, "zf", return_used=True)
    # a view of several row sets has no one data set to learn a structure from; a view of one set is that set's evaluator
    rows = gc.row_sets(S, 100, n_sets=2)
    view = ev.with_rows(torch.from_numpy(rows).cuda())
    for what, fn in (("pc_stable", lambda: pc_stable(view, test="zf")), ("mmpc", lambda: mmpc(view, test="zf"))):
        with pytest.raises(ValueError, match=f"{what}: the evaluator is a view of 2 row sets"):
            fn()
    from dags_vae_search_amd import GaussianEvaluator
    single = ev.with_rows(torch.from_numpy(rows[:1]).cuda())
    gathered = GaussianEvaluator("gathered", "bic-g", data=np.ascontiguousarray(gc.gauss_data(n, S)[rows[0]]))
    a, b = pc_stable(single, test="zf"), pc_stable(gathered, test="zf")
    assert a.tests_per_level == b.tests_per_level and _masks(a.pdag) == _masks(b.pdag) and _masks(a.sepsets) == _masks(b.sepsets)
    assert _masks(mmpc(single, test="cor").skeleton) == _masks(mmpc(gathered, test="cor").skeleton)
