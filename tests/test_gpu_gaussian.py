"""GPU: Gaussian networks (csrc/dvs_gaussian.h) through the raw calls with the cases, references and checks of
tests/gaussian_corpus.py — shared with the emulator twin tests/test_emu_gaussian.py — plus the Python surface
(dags_vae_search_amd/gaussian.py) under the searches that take an evaluator: hill_climb, tabu_search, exact_search,
boot_strength, and the guards of the entry points that read discrete levels."""
import ctypes
import functools

import numpy as np
import pytest

from dags_vae_search_amd import gaussian  # noqa: F401  (the module under test: its absence fails every test of this file)
from tests import gaussian_corpus as gc
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc
from tests import tabu_corpus as tb

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


def _masks(t):
    return t.cpu().numpy().view(U64)


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("S", gc.S_VALUES)
@pytest.mark.parametrize("n", gc.N_VALUES)
def test_moments(n, S):
    worst = gc.check_moments(backend(), n, S)
    print(f"n {n} S {S}: worst moment error / bound {worst:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
def test_scores_against_mpmath(n, S):
    worst = gc.check_scores(backend(), n, S)
    print(f"n {n} S {S}: worst score error / bound {worst:.3e}")


@pytest.mark.parametrize("n, S", gc.SCORE_SHAPES)
def test_fit_against_mpmath(n, S):
    worst = gc.check_fit(backend(), n, S)
    print(f"n {n} S {S}: worst coefficient / intercept / sd error / bound {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e}")


def test_refusals_between_sentinels():
    gc.check_refusals(backend())


@pytest.mark.parametrize("n", (5, 17, 48))
def test_toggle_cells_are_the_scorer_bytes(n):
    gc.check_toggles(backend(), n, variants=gc.SCORE_VARIANTS if n == 5 else (("bic-g", None, None), ("bge", None, None)))


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    gc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_evaluator_surface_equals_the_raw_calls(tmp_path):
    import torch
    from dags_vae_search_amd import GaussianEvaluator, gaussian_fit
    n, S = 5, gc.CHUNK + 1
    x = gc.gauss_data(n, S)
    be = backend()
    mom = gc.run_moments(be, x)
    P = gc.random_dags(n, 6, 3, seed=1)
    Pt = torch.from_numpy(P.view(np.int64)).cuda()
    path = tmp_path / "real.csv"
    path.write_text("\n".join([",".join(f"v{i}" for i in range(n))] + [",".join(repr(float(v)) for v in row) for row in x]) + "\n")
    for typ, a1, a2 in (gc.variant_args(n, v) for v in gc.SCORE_VARIANTS):
        kw = dict(iss_mu=a1, iss_w=a2) if typ == "bge" else dict(k=a1) if typ != "loglik-g" else {}
        ev = GaussianEvaluator("syn5", typ, data=x, **kw)
        assert (ev.n_vars, ev.n_samples, ev.metric_name, ev.device.type) == (n, S, typ, "cuda")
        assert ev.moments.cpu().numpy().tobytes() == mom.tobytes()
        local, out, status = gc.run_scores(be, mom, n, P, typ, a1, a2)
        assert status == 0
        got, got_local = ev.score_masks(Pt, local=True)
        assert got.cpu().numpy().tobytes() == out.tobytes() and got_local.cpu().numpy().tobytes() == local.tobytes()
        L, T, _ = gc.run_toggle(be, mom, n, P, typ, a1, a2)
        gl, gt, st = ev.toggle_scores(Pt, return_status=True)
        assert gl.cpu().numpy().tobytes() == L.tobytes() and gt.cpu().numpy().tobytes() == T.tobytes() and int(st[0]) == 0
        for other in (GaussianEvaluator("csv", typ, data=str(path), **kw),
                      GaussianEvaluator.from_device("dev", typ, torch.from_numpy(np.array(x)).cuda(), **kw)):
            assert other.moments.cpu().numpy().tobytes() == mom.tobytes()
            assert other.score_masks(Pt).cpu().numpy().tobytes() == out.tobytes()
    ev = GaussianEvaluator("syn5", data=x.astype(np.float32))               # float32 is converted once; bic-g is the default
    assert ev.metric_name == "bic-g" and ev.x.dtype == torch.float64
    assert ev.moments.cpu().numpy().tobytes() == gc.run_moments(be, x.astype(np.float32).astype(np.float64)).tobytes()
    ev = GaussianEvaluator("syn5", "bic-g", data=x)
    coef, icpt, sd, _ = gc.run_fit(be, mom, n, P)
    fit = gaussian_fit(ev, Pt)
    assert fit.coef.cpu().numpy().tobytes() == coef.tobytes() and fit.intercept.cpu().numpy().tobytes() == icpt.tobytes()
    assert fit.sd.cpu().numpy().tobytes() == sd.tobytes() and gaussian_fit(ev, Pt[0]).sd.cpu().numpy().tobytes() == sd[:1].tobytes()
    # row sets: one moments call over the sets, structure b on set b or on set_of[b]
    rows = gc.row_sets(S, 70, n_sets=6)
    view = ev.with_rows(torch.from_numpy(rows).cuda())
    assert view.n_samples == 70 and view.moments.cpu().numpy().tobytes() == gc.run_moments(be, x, rows).tobytes()
    local, out, _ = gc.run_scores(be, gc.run_moments(be, x, rows), n, P, "bic-g", set_of=np.arange(6))
    assert view.score_masks(Pt).cpu().numpy().tobytes() == out.tobytes()
    set_of = np.asarray([5, 0, 0, 3, 2, 1], np.int32)
    _, out, _ = gc.run_scores(be, gc.run_moments(be, x, rows), n, P, "bic-g", set_of=set_of)
    assert ev.with_rows(torch.from_numpy(rows).cuda(), torch.from_numpy(set_of)).score_masks(Pt).cpu().numpy().tobytes() == out.tobytes()
    with pytest.raises(ValueError, match=r"rows must lie in \[0, 129\)"):
        ev.with_rows(torch.tensor([[0, 129]], dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="built Gaussian scores"):
        GaussianEvaluator("syn5", "bic", data=x)
    with pytest.raises(ValueError, match="k is the argument of"):
        GaussianEvaluator("syn5", "bge", data=x, k=1.0)
    with pytest.raises(ValueError, match="iss_w must be finite and > n_vars"):
        GaussianEvaluator("syn5", "bge", data=x, iss_w=6.0)
    with pytest.raises(ValueError, match="a family was refused"):
        GaussianEvaluator("deg", "bic-g", data=gc.degenerate_data()).score_masks(torch.tensor([[0, 0, 0, 2, 0]], dtype=torch.int64))
    with pytest.raises(ValueError, match="gaussian_fit: refused families"):
        gaussian_fit(GaussianEvaluator("deg", "bic-g", data=gc.degenerate_data()), torch.tensor([[0, 0, 0, 2, 0]], dtype=torch.int64))


def _search_setup(typ):
    import torch
    from dags_vae_search_amd import GaussianEvaluator
    n, S = gc.SEARCH_N, gc.SEARCH_S
    ev = GaussianEvaluator("syn6", typ, data=gc.gauss_data(n, S))
    starts = np.concatenate([np.zeros((1, n), U64), gc.random_dags(n, 2, 2, seed=5)])
    starts[1:] = [[int(m) & ~gc.mask_of(range(v + 1, n)) for v, m in enumerate(row)] for row in starts[1:]]      # inside the order
    tol = 4 * gc.family_table(n, S, typ)[1]                  # a delta reads up to four local scores
    return torch, ev, n, starts, tol


def _tables(torch, ev, P):
    L, T = ev.toggle_scores(torch.tensor([[int(x) for x in P]], dtype=torch.int64).cuda())
    return L[0].cpu().numpy(), T[0].cpu().numpy()


@pytest.mark.parametrize("typ", ("bic-g", "bge"))
@pytest.mark.parametrize("ordered", (True, False), ids=("ordered", "free"))
def test_hill_climb_equals_a_greedy_loop_over_the_device_tables(typ, ordered):
    """the trace of hill_climb against select_ref (tests/hillclimb_corpus.py) applied to the evaluator's own toggle tables.
    Under the fixed order every selection's gap to the runner-up is asserted to exceed the tolerance first; without it
    score-equivalent moves tie in exact arithmetic, so the free climb is held to the tables' bytes and the tie rule alone."""
    from dags_vae_search_amd import hill_climb
    torch, ev, n, starts, tol = _search_setup(typ)
    forb = gc.ordered_forbidden(n) if ordered else None
    res = hill_climb(ev, torch.from_numpy(starts.view(np.int64)), max_steps=40, min_delta=hc.MIN_DELTA, forbidden=forb, trace=True)
    codes, deltas = res.trace[0].cpu().numpy(), res.trace[1].cpu().numpy()
    assert res.converged.cpu().numpy().all() and not res.flags.cpu().numpy().any()
    for b in range(len(starts)):
        P, k = [int(x) for x in starts[b]], 0
        while True:
            L, T = _tables(torch, ev, P)
            moves = [(c, hc.move_delta(op, v, u, L, T)) for c, op, v, u in hc.legal_moves(P, None, forb)]
            moves = [(c, d) for c, d in moves if not np.isnan(d)]
            pick = hc.select_ref(P, L, T, None, forb, hc.MIN_DELTA)
            if pick is None:
                break
            if ordered:
                assert gc.selection_gap(moves) > tol, (typ, b, k, gc.selection_gap(moves), tol)
            assert int(codes[b, k]) == pick[0] and deltas[b, k].tobytes() == np.float64(pick[1]).tobytes(), (typ, b, k)
            P, k = hc.apply_move(P, pick[0])[0], k + 1
        assert k == int(res.steps[b]) and k > 0 and [int(x) for x in _masks(res.parents)[b]] == P
    assert res.scores.cpu().numpy().tobytes() == ev.score_masks(res.parents).cpu().numpy().tobytes()


@pytest.mark.parametrize("typ", ("bic-g", "bge"))
def test_tabu_search_equals_the_restated_walk_over_the_device_tables(typ):
    from dags_vae_search_amd import tabu_search
    torch, ev, n, starts, tol = _search_setup(typ)
    forb, tabu_len, max_steps = gc.ordered_forbidden(n), 4, 25
    res = tabu_search(ev, torch.from_numpy(starts.view(np.int64)), max_steps=max_steps, tabu=tabu_len, min_delta=hc.MIN_DELTA,
                      forbidden=forb, trace=True)
    codes, deltas = res.trace[0].cpu().numpy(), res.trace[1].cpu().numpy()
    for b in range(len(starts)):
        P, st = [int(x) for x in starts[b]], tb.TabuState(n, tabu_len)
        while not st.converged and st.steps < max_steps:
            L, T = _tables(torch, ev, P)
            seen = [[int(x) for x in st.ring[e]] for e in range(min(st.visited, tabu_len))] + [P]
            moves = [(c, hc.move_delta(op, v, u, L, T)) for c, op, v, u in hc.legal_moves(P, None, forb)
                     if hc.apply_move(P, c)[0] not in seen]
            moves = [(c, d) for c, d in moves if not np.isnan(d)]
            k = st.steps
            pick = tb.tabu_select_ref(P, L, T, st, tabu_len, None, forb, hc.MIN_DELTA)
            if pick is None:
                break
            assert gc.selection_gap(moves) > tol, (typ, b, k, gc.selection_gap(moves), tol)
            assert int(codes[b, k]) == pick[0] and deltas[b, k].tobytes() == np.float64(pick[1]).tobytes(), (typ, b, k)
            P = pick[2]
        assert st.steps == int(res.steps[b]) and st.steps > 0
        assert [int(x) for x in _masks(res.last_parents)[b]] == P
        assert _masks(res.parents)[b].tobytes() == st.best_parents.tobytes()


def test_exact_search_with_bge_is_the_brute_force_optimum_and_its_class():
    import torch
    from dags_vae_search_amd import GaussianEvaluator, exact_search
    n, S = 5, 300
    ev = GaussianEvaluator("syn5", "bge", data=gc.gauss_data(n, S))
    table, bound = gc.family_table(n, S, "bge")
    dags = gc.all_dags(n)
    assert len(dags) == 29281
    totals = sum(table[v, dags[:, v]] for v in range(n))
    tol = 2 * n * bound
    best = totals.max()
    optima = {tuple(int(x) for x in P) for P in dags[totals >= best - tol]}
    assert totals[totals < best - tol].max() < best - 10 * tol            # the optima stand clear of everything else
    res = exact_search(ev)
    found = tuple(int(x) for x in _masks(res.parents)[0])
    assert found in optima
    assert abs(float(res.scores[0]) - best) <= tol and abs(float(res.rescored[0]) - best) <= tol
    edges = sum(bin(m).count("1") for m in found)
    same_size = dags[np.asarray([sum(bin(int(m)).count("1") for m in P) == edges for P in dags])]
    key = gc.cpdag_key(found)
    cls = {tuple(int(x) for x in P) for P in same_size if gc.cpdag_key(P) == key}
    assert cls == optima and len(cls) >= 1
    print(f"bge optimum {best:.6f}: {len(cls)} DAGs in its equivalence class, tolerance {tol:.3e}")


def test_boot_strength_replicates_are_plain_climbs_on_the_gathered_rows():
    import torch
    from dags_vae_search_amd import GaussianEvaluator, boot_strength, bootstrap_rows, hill_climb
    n, S, R, seed = 5, 300, 4, 11
    ev = GaussianEvaluator("syn5", "bic-g", data=gc.gauss_data(n, S))
    args = dict(max_steps=40, min_delta=hc.MIN_DELTA)
    res = boot_strength(ev, replicates=R, algorithm_args=args, seed=seed, return_networks=True)
    assert res.n_networks == R and res.exhausted == 0 and res.networks.shape == (R, n)
    for r in range(R):
        rows = bootstrap_rows(1, S, S, seed=seed, set_offset=r)
        one = GaussianEvaluator.from_device("replicate", "bic-g", ev.x[rows[0].long()])
        plain = hill_climb(one, batch=1, **args)
        assert plain.parents.cpu().numpy().tobytes() == res.networks[r:r + 1].cpu().numpy().tobytes(), r
        assert int(plain.steps[0]) > 0
    assert int(res.any.sum()) > 0


def test_discrete_entry_points_refuse_a_gaussian_evaluator():
    import torch
    from dags_vae_search_amd import (GaussianEvaluator, bn_fit, ci_test, ci_tests, ci_tests_group, cross_validate, mmpc, pc_stable)
    ev = GaussianEvaluator("syn5", "bic-g", data=gc.gauss_data(5, gc.CHUNK + 1))
    one = lambda v, dt: torch.tensor([v], dtype=dt, device="cuda")
    P = torch.zeros(1, 5, dtype=torch.int64, device="cuda")
    calls = {
        "ci_tests": lambda: ci_tests(ev, torch.tensor([[0, 1]], dtype=torch.int32, device="cuda"), one(0, torch.int64)),
        "ci_test": lambda: ci_test(ev, 0, 1),
        "pc_stable": lambda: pc_stable(ev),
        "mmpc": lambda: mmpc(ev),
        "ci_tests_group": lambda: ci_tests_group(ev, one(0, torch.int32), one(0, torch.int64), one(6, torch.int64)),
        "bn_fit": lambda: bn_fit(ev, P),
        "cross_validate": lambda: cross_validate(ev, P, folds=2),
        "available_case": lambda: ev.available_case(torch.zeros(ev.n_samples, dtype=torch.int64, device="cuda")),
    }
    for what, fn in calls.items():
        with pytest.raises(ValueError, match=f"{what}: the evaluator holds real-valued data .* Gaussian counterpart is not built"):
            fn()
