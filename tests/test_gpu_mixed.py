"""GPU: conditional Gaussian networks on mixed data (csrc/dvs_mixed.h) through the raw calls with the cases, references and
checks of tests/mixed_corpus.py — shared with the emulator twin tests/test_emu_mixed.py — plus the Python surface
(dags_vae_search_amd/mixed.py): the table cache, hill_climb and tabu_search on a MixedEvaluator, cg_fit, and the guards of the
entry points that are not built on mixed data."""
import functools

import numpy as np
import pytest

from dags_vae_search_amd import mixed  # noqa: F401  (the module under test: its absence fails every test of this file)
from tests import gaussian_corpus as gc
from tests import mixed_corpus as mc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("S", mc.PARTITION_S)
def test_partition_is_the_stable_sort(S):
    mc.check_partition(backend(), S)


def test_partition_one_factor_in_each_packed_word():
    mc.check_partition_wide(backend())


def test_partition_cut_into_spans():
    mc.check_partition_spans(backend())


def test_partition_refusals():
    mc.check_partition_refusals(backend())


@pytest.mark.parametrize("nc", (1, 5, 17))
def test_ragged_moments(nc):
    worst = mc.check_moments(backend(), nc)
    print(f"n_c {nc}: worst moment error / bound {worst:.3e}")


def test_scores_against_mpmath():
    worst = mc.check_scores(backend())
    print(f"worst score error / bound {worst:.3e}")


def test_byte_identities():
    mc.check_identities(backend())


def test_refusals_between_sentinels():
    mc.check_refusals(backend())


@pytest.mark.parametrize("n", (5, 17, 48))
def test_toggle_cells_are_the_scorer_bytes(n):
    mc.check_toggles(backend(), n, variants=(("bic-cg", None), ("aic-cg", 0.3)) if n == 5 else (("bic-cg", None),))


def test_fit_against_mpmath():
    worst = mc.check_fit(backend())
    print(f"worst coefficient / intercept / sd error / bound {worst[0]:.3e} {worst[1]:.3e} {worst[2]:.3e}")


# ---- the Python surface ------------------------------------------------------------------------------------------------
CARD7 = [2, 0, 3, 0, 2, 0, 0]                # n = 7: factors 0, 2, 4 (2, 3, 2 levels) and four real columns


@functools.lru_cache(maxsize=None)
def network_data():
    """600 rows drawn with numpy from a fixed mixed network: 0 -> 2 -> 4 among the factors; 1 | 0; 3 | 2, 1; 5 | 3; 6 | 4, 5"""
    rng = np.random.default_rng(3700)
    S = 600
    a = np.zeros((S, 7))
    a[:, 0] = rng.integers(0, 2, S)
    a[:, 2] = np.where(rng.random(S) < 0.7, (a[:, 0] + 1) % 3, rng.integers(0, 3, S))
    a[:, 4] = np.where(rng.random(S) < 0.8, a[:, 2] % 2, rng.integers(0, 2, S))
    a[:, 1] = 1.5 * a[:, 0] + rng.normal(0, 1.0, S)
    a[:, 3] = np.asarray([-1.0, 0.5, 2.0])[a[:, 2].astype(int)] + np.asarray([0.8, -0.6, 0.3])[a[:, 2].astype(int)] * a[:, 1] + rng.normal(0, 0.5, S)
    a[:, 5] = 0.7 * a[:, 3] + rng.normal(0, 1.0, S)
    a[:, 6] = 2.0 * a[:, 4] - 0.5 * a[:, 5] + rng.normal(0, 0.7, S)
    return a


@functools.lru_cache(maxsize=None)
def evaluator(metric="bic-cg"):
    from dags_vae_search_amd import MixedEvaluator
    return MixedEvaluator("fixed-mixed", metric, data=network_data(), discrete=CARD7)


def _starts():
    import torch
    P = np.zeros((4, 7), U64)
    P[1, 1], P[1, 3] = U64(1 << 0), U64((1 << 2) | (1 << 1))
    P[2, 6], P[2, 4], P[2, 5] = U64((1 << 4) | (1 << 5)), U64(1 << 2), U64(1 << 1)
    P[3, 2], P[3, 6] = U64(1 << 0), U64(1 << 0)
    return torch.from_numpy(P.view(np.int64)).cuda()


def test_surface_and_cache():
    import torch
    ev = evaluator()
    assert ev.kind == ["discrete" if c else "continuous" for c in CARD7] and ev.card.cpu().tolist() == CARD7
    cont = sum(1 << v for v in range(7) if not CARD7[v])
    assert ev.illegal.cpu().tolist() == [cont if c else 0 for c in CARD7]
    P = _starts()
    ev.clear_cache()
    cold = ev.toggle_scores(P)
    before = dict(ev.cache_stats)
    warm = ev.toggle_scores(P)
    assert ev.cache_stats["misses"] == before["misses"] and ev.cache_stats["hits"] > before["hits"]
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(cold, warm)), "a cold and a warm cache give equal bytes"
    # a budget that holds the pass but not the cache's history: the same bytes again
    small = type(ev).from_device("fixed-mixed", "bic-cg", ev.packed, ev.x, CARD7, table_bytes=64 * 1024)
    tiny = small.toggle_scores(P)
    small.score_masks(P)
    again = small.toggle_scores(P)
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes() for a, b, c in zip(cold, tiny, again))
    scores, local = ev.score_masks(P, local=True)
    assert local.cpu().numpy().tobytes() == cold[0].cpu().numpy().tobytes()
    bad = P.clone()
    bad[0, 0] = 1 << 1                                            # a continuous parent of a factor
    with pytest.raises(ValueError, match=r"refused families \(structure, variable\): \[\[0, 0\]\]"):
        ev.score_masks(bad)
    with pytest.raises(ValueError, match="table_bytes"):
        type(ev).from_device("fixed-mixed", "bic-cg", ev.packed, ev.x, CARD7, table_bytes=64).score_masks(P)
    # the discrete cells are BNLearnWrapper's, the D = {} cells GaussianEvaluator's
    from dags_vae_search_amd import BNLearnWrapper, GaussianEvaluator
    zero = torch.zeros(1, 7, dtype=torch.int64, device="cuda")
    l0 = ev.score_masks(zero, local=True)[1].cpu().numpy()
    dis = BNLearnWrapper.from_packed("d", "bic", ev.packed, [c or 1 for c in CARD7]).score_masks(zero, local=True)[1].cpu().numpy()
    gau = GaussianEvaluator.from_device("g", "bic-g", ev.x).score_masks(torch.zeros(1, 4, dtype=torch.int64, device="cuda"), local=True)[1].cpu().numpy()
    assert l0[0, [0, 2, 4]].tobytes() == dis[0, [0, 2, 4]].tobytes() and l0[0, [1, 3, 5, 6]].tobytes() == gau[0].tobytes()


@pytest.mark.parametrize("algorithm", ("hill_climb", "tabu_search"))
def test_search_on_mixed_data(algorithm):
    import torch
    import dags_vae_search_amd as pkg
    from dags_vae_search_amd.hillclimb import decode_move
    ev = evaluator()
    search = getattr(pkg, algorithm)
    args = dict(max_steps=40, trace=True)
    res = search(ev, _starts(), **args)
    assert res.scores.cpu().numpy().tobytes() == ev.score_masks(res.parents).cpu().numpy().tobytes()
    codes, deltas = (t.cpu().numpy() for t in res.trace)
    steps = res.steps.cpu().numpy()
    disc = [v for v in range(7) if CARD7[v]]
    cont = sum(1 << v for v in range(7) if not CARD7[v])
    start = _starts().cpu().numpy().view(U64)
    worst = 0.0
    for b in range(4):
        P = start[b].copy()
        prev = float(ev.score_masks(torch.from_numpy(P.view(np.int64))[None].cuda())[0])
        visited = {P.tobytes(): prev}
        for t in range(int(steps[b])):
            op, u, v = decode_move(int(codes[b, t]), 7)
            if op == "reverse":
                P[v] ^= U64(1 << u)
                P[u] ^= U64(1 << v)
            else:
                P[v] ^= U64(1 << u)
            assert not any(int(P[d]) & cont for d in disc), (b, t, "a continuous -> discrete arc")
            now = float(ev.score_masks(torch.from_numpy(P.view(np.int64))[None].cuda())[0])
            ulp = np.spacing(max(abs(now), abs(prev)))
            assert abs((now - prev) - float(deltas[b, t])) <= 64 * ulp, (b, t, op, u, v, now - prev, float(deltas[b, t]))
            worst = max(worst, abs((now - prev) - float(deltas[b, t])) / ulp)
            prev = now
            visited[P.tobytes()] = now
        if algorithm == "hill_climb":
            assert P.tobytes() == res.parents[b].cpu().numpy().tobytes()
        else:
            # the walk may go downhill: the result is the best structure it stood on (best by the walk's own running sum of
            # deltas, each within 64 ulp of the rescored difference)
            assert P.tobytes() == res.last_parents[b].cpu().numpy().tobytes()
            best = res.parents[b].cpu().numpy().tobytes()
            top = max(visited.values())
            assert best in visited and visited[best] >= top - 64 * max(1, int(steps[b])) * np.spacing(abs(top))
    print(f"{algorithm}: worst traced delta error {worst:.1f} ulp")
    twice = search(ev, _starts(), **args)
    barred = search(ev, _starts(), forbidden=ev.illegal, **args)
    for other in (twice, barred):
        assert other.parents.cpu().numpy().tobytes() == res.parents.cpu().numpy().tobytes()
        assert other.scores.cpu().numpy().tobytes() == res.scores.cpu().numpy().tobytes()
        assert other.trace[1].cpu().numpy().tobytes() == res.trace[1].cpu().numpy().tobytes()
    if algorithm == "hill_climb":
        restarted = search(ev, _starts(), max_steps=40, restarts=2, perturb=2, seed=5)
        assert (restarted.scores >= res.scores).all()
        assert not any(int(m) & cont for row in restarted.parents[:, disc].cpu().tolist() for m in row)
        from dags_vae_search_amd import cg_fit
        for b in range(4):
            fit = cg_fit(ev, res.parents[b])
            for v in range(7):
                if CARD7[v]:
                    assert fit.coef[v] is None
                    continue
                live = (fit.count[v] > 0).cpu().numpy()
                assert live.any() and int(fit.count[v].sum()) == 600
                assert np.isfinite(fit.coef[v].cpu().numpy()[live]).all() and np.isfinite(fit.intercept[v].cpu().numpy()[live]).all()
                assert (fit.sd[v].cpu().numpy()[live] > 0).all()
            assert fit.discrete is not None and fit.discrete_vars == disc


def test_cg_fit_recovers_the_network():
    import torch
    from dags_vae_search_amd import cg_fit
    ev = evaluator()
    P = np.zeros(7, U64)
    P[2], P[4], P[1], P[3], P[5], P[6] = U64(1), U64(1 << 2), U64(1), U64((1 << 2) | (1 << 1)), U64(1 << 3), U64((1 << 4) | (1 << 5))
    fit = cg_fit(ev, torch.from_numpy(P.view(np.int64)).cuda())
    a = network_data()
    for z in range(3):
        rows = a[a[:, 2] == z]
        coef, icpt, sd = gc.lstsq_fit(rows[:, [1, 3]], 1, [0])
        assert abs(float(fit.coef[3][z, 1]) - coef[0]) < 1e-9 and abs(float(fit.intercept[3][z]) - icpt) < 1e-9
        assert abs(float(fit.sd[3][z]) - sd) < 1e-9 and float(fit.count[3][z]) == len(rows)
    assert fit.coef[3].shape == (3, 7) and fit.coef[6].shape == (2, 7) and fit.coef[5].shape == (1, 7)
    bad = P.copy()
    bad[0] = U64(1 << 1)
    with pytest.raises(ValueError, match="discrete variable 0 has a continuous parent"):
        cg_fit(ev, torch.from_numpy(bad.view(np.int64)).cuda())


def test_entry_points_that_are_not_built_on_mixed_data_say_so():
    import torch
    import dags_vae_search_amd as pkg
    ev = evaluator()
    zero = torch.zeros(7, dtype=torch.int64, device="cuda")
    calls = {
        "with_rows / boot_strength": lambda: ev.with_rows(torch.zeros(1, 4, dtype=torch.int32, device="cuda")),
        "boot_strength": lambda: pkg.boot_strength(ev, replicates=2, algorithm_args=dict(max_steps=2)),
        "exact_search": lambda: pkg.exact_search(ev),
        "arc_posterior": lambda: pkg.arc_posterior(ev),
        "order_mcmc": lambda: pkg.order_mcmc(ev, steps=10),
        "bn_fit": lambda: pkg.bn_fit(ev, zero),
        "gaussian_fit": lambda: pkg.gaussian_fit(ev, zero),
        "ci_tests": lambda: pkg.ci_tests(ev, torch.zeros(1, 2, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")),
        "pc_stable": lambda: pkg.pc_stable(ev),
        "mmpc": lambda: pkg.mmpc(ev),
        "mmhc": lambda: pkg.mmhc(ev),
        "cross_validate": lambda: pkg.cross_validate(ev, zero),
        "gaussian_cross_validate": lambda: pkg.gaussian_cross_validate(ev, zero),
        "available_case": lambda: ev.available_case(),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match=f"{name}: the evaluator holds mixed data .* mixed data is not built for {name}"):
            call()
    for test in ("cor", "zf", "mi-g", "mc-mi"):
        with pytest.raises(ValueError, match="mixed data is not built for"):
            pkg.pc_stable(ev, test=test)
