"""GPU: available-case scoring on incomplete data (csrc/dvs_available.h) through the raw calls with the cases, references and
checks of tests/available_corpus.py — shared with the emulator twin tests/test_emu_available.py — plus the Python surface: the
view ``BNLearnWrapper.available_case`` under ``hill_climb`` and ``tabu_search``, and ``structural_em``."""
import functools

import numpy as np
import pytest

from tests import available_corpus as av
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def driver():
    from dags_vae_search_amd import _lib as dl
    return av.AvailDriver(sc.GpuBackend(dl.load()))


@pytest.mark.parametrize("kind", av.MASK_SETS)
@pytest.mark.parametrize("name", av.DATASETS)
def test_scores_are_the_formula_over_the_plain_scorer_on_the_rows_that_count(name, kind):
    print(f"\n{name} {kind}: {dict(av.check_scores(driver(), name, kind))}")


@pytest.mark.parametrize("name", av.DATASETS)
def test_everything_observed_is_the_plain_scorer_over_n_samples(name):
    av.check_everything_observed(driver(), name)


@pytest.mark.parametrize("kind", ("light", "heavy"))
@pytest.mark.parametrize("name", av.DATASETS)
def test_toggle_cells_are_the_scorer_on_the_flipped_structure(name, kind):
    av.check_toggles(driver(), name, kind)


def test_kernels_against_the_restatement():
    av.check_kernels_against_restatement(driver())


def test_hand_cases_in_closed_form():
    av.check_hand_cases(driver())


def test_refusals_leave_the_outputs_untouched():
    av.check_refusals_leave_outputs_untouched(driver())


# ---------------------------------------------------------------------------------------------------------------------
# The Python surface
# ---------------------------------------------------------------------------------------------------------------------
CARD = [2, 3, 2, 3, 2, 2]
DAG = {1: [0], 2: [0], 3: [1, 2], 4: [3], 5: [4]}


@functools.lru_cache(maxsize=None)
def hand_network():
    """six variables, 0 -> 1, 0 -> 2, {1, 2} -> 3 -> 4 -> 5; every table row puts 0.8 on one level, which moves with the
    configuration, and spreads the rest"""
    import dags_vae_search_amd as dvs
    masks = [int(m) for m in sc.masks_of(6, DAG)[0]]
    tables = []
    for v, r in enumerate(CARD):
        q = int(np.prod([CARD[u] for u in DAG.get(v, [])]))
        t = np.full((q, r), 0.2 / (r - 1))
        for j in range(q):
            t[j, (j + v) % r] = 0.8
        tables.append(t)
    return dvs.FittedBN.from_tables(masks, CARD, tables), masks


@functools.lru_cache(maxsize=None)
def sampled(n_rows, rate, seed):
    """(levels with -1 for missing [R, 6], (rows, observed) on the device): rows of the hand network, missing completely at random"""
    import dags_vae_search_amd as dvs
    fitted, _ = hand_network()
    packed = dvs.sample(fitted, n_rows, seed=seed).cpu().numpy().view(U64)
    levels = np.stack([(packed[:, 0] >> U64(4 * v)) & U64(15) for v in range(6)], 1).astype(np.int64)
    if rate:
        levels[np.random.default_rng(seed + 1).random(levels.shape) < rate] = -1
        levels[0], levels[1] = np.abs(levels[0]), -1                                   # one row whole, one row empty
        levels[2, 1:] = -1
    return levels, dvs.incomplete_rows(levels)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _replay(view, result, n, greedy=True):
    """every accepted move against a fresh full toggle pass on the structure it left and the scorer on the one it reached"""
    import torch
    from dags_vae_search_amd.hillclimb import decode_move
    codes, deltas = result.trace
    steps = int(result.steps[0])
    parents = torch.zeros(1, n, dtype=torch.int64, device="cuda")
    for t in range(steps):
        L, T = view.toggle_scores(parents)
        op, u, v = decode_move(int(codes[0, t]), n)
        d = T[0, v, u] - L[0, v]
        if op == "reverse":
            d = d + (T[0, u, v] - L[0, u])
        assert _bytes(d) == _bytes(deltas[0, t]) and (float(d) > 0.0 or not greedy), (t, op, u, v)
        parents[0, v] ^= 1 << u
        if op == "reverse":
            parents[0, u] |= 1 << v
        total, local = view.score_masks(parents, local=True)
        assert _bytes(local[0, v]) == _bytes(T[0, v, u]), (t, op, u, v)                  # the step's score is the scorer's
        if op == "reverse":
            assert _bytes(local[0, u]) == _bytes(T[0, u, v])
    assert _bytes(parents) == _bytes(result.parents if greedy else result.last_parents)
    assert _bytes(result.scores) == _bytes(view.score_masks(result.parents))
    return steps


@pytest.mark.parametrize("search", ("hill_climb", "tabu_search"))
def test_the_searches_take_the_view(search):
    import dags_vae_search_amd as dvs
    levels, data = sampled(2000, 0.3, 611)
    default = dvs.available_case_evaluator(data, CARD)
    assert isinstance(default, dvs.AvailableCaseEvaluator) and default.metric_name == "pnal" and default.penalty == 2000 ** -0.25
    view = dvs.available_case_evaluator(data, CARD, "pnal", k=0.02)          # the default penalty admits a single arc here
    assert view.penalty == 0.02 and view.n_samples == 2000
    used = view.used(view.base.packed.new_zeros(1, 6))
    assert used.dtype.is_floating_point is False and used.tolist() == [[int((levels[:, v] >= 0).sum()) for v in range(6)]]
    if search == "hill_climb":
        result = dvs.hill_climb(view, batch=1, max_steps=40, trace=True)
        assert int(result.converged[0]) == 1
        assert _replay(view, result, 6) >= 4
    else:
        result = dvs.tabu_search(view, batch=1, max_steps=40, tabu=5, trace=True)
        assert _replay(view, result, 6, greedy=False) >= 4
        climb = dvs.hill_climb(view, batch=1, max_steps=40)
        assert float(result.scores[0]) >= float(climb.scores[0])                       # tabu keeps the best it stood on
    with pytest.raises(NotImplementedError):
        view.with_rows(None)


def test_nal_on_complete_data_takes_the_moves_of_the_plain_loglik_climb():
    """Dividing every local score by the same S keeps the order of the deltas unless two candidates are closer than the
    roundings: a nal local score L / S carries an error of at most ulp(L / S), so a delta of two of them 2 ulp(L / S), which is
    2 ulp(L / S) S on the plain scale; two deltas 4 ulp(L / S) S.  Adds in both directions have the same likelihood gain (the
    mutual information), so `forbidden` bars u -> v for u > v: the candidates are then the adds u < v under the parent cap and
    the deletes, and they are asserted to lie further apart than that at every step of the plain run."""
    import torch
    import dags_vae_search_amd as dvs
    levels, (rows, observed) = sampled(2000, 0.0, 611)
    S, n = 2000, 6
    plain = dvs.BNLearnWrapper.from_packed("six", "loglik", rows, CARD)
    view = plain.available_case(observed, "nal")
    forbidden = [sum(1 << u for u in range(n) if u > v) for v in range(n)]
    kw = dict(batch=1, max_steps=40, max_parents=2, forbidden=forbidden, trace=True)
    a, b = dvs.hill_climb(plain, **kw), dvs.hill_climb(view, **kw)
    steps = int(a.steps[0])
    assert steps >= 5 and steps == int(b.steps[0])
    assert a.trace[0][0, :steps].tolist() == b.trace[0][0, :steps].tolist() and _bytes(a.parents) == _bytes(b.parents)
    from dags_vae_search_amd.hillclimb import decode_move
    parents = torch.zeros(1, n, dtype=torch.int64, device="cuda")
    for t in range(steps):
        L, T = (x.cpu().numpy()[0] for x in plain.toggle_scores(parents))
        rowsP = [int(m) for m in parents[0].tolist()]
        cand = [T[v, u] - L[v] for v in range(n) for u in range(v)
                if (rowsP[v] >> u) & 1 or bin(rowsP[v]).count("1") < 2]
        gap = 4 * np.spacing(np.abs(L).max() / S) * S
        cand = np.sort(np.asarray(cand))
        assert len(cand) >= 2 and np.diff(cand).min() > gap, (t, np.diff(cand).min(), gap)
        op, u, v = decode_move(int(a.trace[0][0, t]), n)
        parents[0, v] ^= 1 << u


# ---- structural_em: 6 variables, 500 rows, max_parents = 2 ---------------------------------------------------------------
def _hand_composition(data, iterations, refit="completed"):
    """impute -> from_packed -> hill_climb -> bn_fit, as structural_em documents it -> [(parents, score, left out, fitted)]"""
    import torch
    import dags_vae_search_amd as dvs
    fitted = dvs.em_fit([0] * 6, CARD, data, method="bayes").fitted
    current, out = [0] * 6, []
    for _ in range(iterations):
        rows, seen = dvs.impute(fitted, data)
        whole = (seen & 63) == 63
        ev = dvs.BNLearnWrapper.from_packed("completed", "bic", rows[whole].contiguous(), CARD)
        found = dvs.hill_climb(ev, torch.tensor([current], dtype=torch.int64, device="cuda"), max_steps=36, max_parents=2)
        current = [int(m) for m in found.parents[0].tolist()]
        fitted = dvs.bn_fit(ev, found.parents[0], method="bayes", unobserved="uniform")
        out.append((current, float(found.scores[0]), int((~whole).sum()), fitted))
    return out


@functools.lru_cache(maxsize=None)
def _em_run():
    import dags_vae_search_amd as dvs
    levels, data = sampled(500, 0.2, 711)
    return data, dvs.structural_em(data, CARD, max_parents=2)


def test_structural_em_is_the_hand_composition_iteration_by_iteration():
    import dags_vae_search_amd as dvs
    data, result = _em_run()
    assert 1 <= result.iterations <= 5 and len(result.trace) == result.iterations
    hand = _hand_composition(data, result.iterations)
    for t, (parents, score, left_out, fitted) in enumerate(hand):
        entry = result.trace[t]
        assert entry["parents"] == parents and entry["left_out"] == left_out, (t, entry, parents)
        assert np.float64(entry["score"]).tobytes() == np.float64(score).tobytes()
        assert entry["log_likelihood"] == float(dvs.expected_counts(fitted, data).log_likelihood.item())
        upto = result if t + 1 == result.iterations else dvs.structural_em(data, CARD, max_parents=2, max_iter=t + 1)
        assert _bytes(upto.fitted.cpt) == _bytes(fitted.cpt) and upto.parents.tolist() == parents, t
    assert result.converged == (result.iterations >= 2 and hand[-1][0] == hand[-2][0])
    assert max(bin(m).count("1") for m in result.parents.tolist()) <= 2


def test_structural_em_on_complete_data_is_hill_climb_and_bn_fit():
    import dags_vae_search_amd as dvs
    levels, data = sampled(500, 0.0, 711)
    result = dvs.structural_em(data, CARD, max_parents=2)
    ev = dvs.BNLearnWrapper.from_packed("completed", "bic", data[0], CARD)
    climb = dvs.hill_climb(ev, batch=1, max_steps=36, max_parents=2)
    assert (result.iterations, result.converged) == (2, True)
    assert _bytes(result.parents) == _bytes(climb.parents[0]) and int(climb.steps[0]) >= 4
    assert _bytes(result.fitted.cpt) == _bytes(dvs.bn_fit(ev, climb.parents[0], method="bayes", unobserved="uniform").cpt)
    assert [e["left_out"] for e in result.trace] == [0, 0]


def test_structural_em_stops_at_max_iter_unconverged():
    import dags_vae_search_amd as dvs
    levels, data = sampled(500, 0.2, 711)
    result = dvs.structural_em(data, CARD, max_parents=2, max_iter=1)
    assert (result.iterations, result.converged, len(result.trace)) == (1, False, 1)


def test_structural_em_refit_em_gives_the_tables_of_em_fit():
    import dags_vae_search_amd as dvs
    levels, data = sampled(500, 0.2, 711)
    result = dvs.structural_em(data, CARD, max_parents=2, max_iter=2, refit="em", maximize="tabu", maximize_args=dict(max_steps=20, tabu=4))
    want = dvs.em_fit(result.parents.tolist(), CARD, data, method="bayes").fitted
    assert _bytes(result.fitted.cpt) == _bytes(want.cpt) and _bytes(result.fitted.parents) == _bytes(want.parents)


def test_structural_em_names_the_iteration_when_the_plans_exceed_the_cap():
    import torch
    import dags_vae_search_amd as dvs
    from tests import incomplete_corpus as nc
    net = nc.network("full4")                                                          # its last family fills the cap alone
    data = (torch.zeros(4, 1, dtype=torch.int64, device="cuda"), torch.full((4,), 0b0111, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match=r"structural_em: iteration 0: .*need 17472 cells; the cap is 16384"):
        dvs.structural_em(data, net.card, start=[int(m) for m in net.masks])


def test_a_variable_no_row_observes_is_a_value_error_that_names_it():
    import torch
    import dags_vae_search_amd as dvs
    levels, (rows, observed) = sampled(500, 0.2, 711)
    with pytest.raises(ValueError, match=r"no row observes variable\(s\) \[4\]"):
        dvs.available_case_evaluator((rows, observed & ~16), CARD, "nal")
    with pytest.raises(ValueError, match="k is the argument of pnal"):
        dvs.available_case_evaluator((rows, observed), CARD, "nal", k=0.1)
