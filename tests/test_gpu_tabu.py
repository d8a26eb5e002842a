"""GPU: tabu search and random restarts (csrc/dvs_tabu.h) through tabu_search / hill_climb and the raw calls, with the cases,
references, tolerances and checks of tests/tabu_corpus.py — shared with the emulator twin tests/test_emu_tabu.py — plus the
Python surface: restarts, flagged starts, the caller's masks."""
import ctypes
import functools

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import tabu_corpus as tb

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def make_driver(name, typ, arg):
    from dags_vae_search_amd import _lib as dl
    return tb.GpuTabuDriver(tb.sc.GpuBackend(dl.load()), tb.hc_case(name), typ, arg)


@pytest.mark.parametrize("name", tb.TABU_CASES)
def test_tabu_trace_replays_exactly(name):
    """Layer 1 on the raw launch sequence; the driver asserts that tabu_search returns the same bytes."""
    drv, r = tb._tabu_cached(make_driver, name)
    downhill = tb.check_tabu_replay(drv, tb.tabu_case(name), r)
    print(f"\ndevice {name}: steps {r.steps.tolist()}, moves that lowered the score {downhill}")
    if not tb.tabu_case(name).cut:
        assert downhill > 0


def test_tabu_hand_made_cases():
    tb.check_tabu_hand_made(make_driver("single", "bic", None))


@pytest.mark.parametrize("name", sorted(tb.ESCAPE))
def test_tabu_leaves_the_optimum_greedy_stops_at(name):
    """Layer 3.  Worst margin used / tau on an MI355X: DESIGN.md §15."""
    tc = tb.tabu_case(name)
    ref = tb.reference_tabu(name)
    drv, r = tb._tabu_cached(make_driver, name)
    g = drv.climb(tc.starts, tc.max_steps, tc.hc.max_parents, tc.hc.forbidden, tc.hc.min_delta)
    assert g.converged.all()
    worst = tb.check_tabu_against_oracle(tc, r, g.scores)
    print(f"\ndevice {name}: worst margin / tau = {worst:.3g}, gains {[float(r.best_score[b] - g.scores[b]) for b in ref]}")


@pytest.mark.parametrize("name", ["asia", "syn17", "syn48"])
def test_perturb_takes_the_drawn_legal_move_and_the_incremental_pass_follows(name):
    taken = tb.check_perturb_case(make_driver(name, "bic", None), name)
    if name == "asia":                                   # 33 structures: two draw indices differ somewhere
        assert taken[7, 1] != taken[7, 0xFFFFFFFF]


def test_perturb_hand_made_cases():
    tb.check_perturb_hand_made(make_driver("single", "bic", None))


def test_two_tabu_runs_are_bytewise_equal_and_a_batch_is_its_rows():
    drv, r = tb._tabu_cached(make_driver, "asia_bde")
    tb.check_tabu_deterministic(drv, tb.tabu_case("asia_bde"), r)


def _fields(r):
    return [x.cpu().numpy().tobytes() for x in (r.parents, r.scores, r.steps, r.converged, r.flags)]


def test_tabu_search_restarts_and_surface():
    import torch
    from dags_vae_search_amd import TabuResult, tabu_search
    tc = tb.tabu_case("asia_bic")
    drv, r0 = tb._tabu_cached(make_driver, "asia_bic")
    ev, starts = drv.ev, drv._t(tc.starts)
    kept = starts.clone()
    kw = dict(max_steps=tc.max_steps, tabu=tc.tabu, min_delta=tc.hc.min_delta)
    plain = tabu_search(ev, starts, **kw)                                    # max_tabu=None means tabu
    assert isinstance(plain, TabuResult) and plain.trace is None and plain.rounds == 0
    assert plain.parents.cpu().numpy().view(np.uint64).tobytes() == r0.best_parents.tobytes()
    res = tabu_search(ev, starts, restarts=2, perturb=3, seed=5, **kw)
    again = tabu_search(ev, starts, restarts=2, perturb=3, seed=5, **kw)
    assert _fields(res) == _fields(again) and torch.equal(res.last_parents, again.last_parents)
    head = tabu_search(ev, starts[:5], restarts=2, perturb=3, seed=5, **kw)  # the draw is keyed by the row
    assert torch.equal(head.parents, res.parents[:5]) and torch.equal(head.scores, res.scores[:5])
    assert torch.equal(head.last_parents, res.last_parents[:5]) and torch.equal(head.steps, res.steps[:5])
    assert res.rounds == 2 and bool((res.scores >= plain.scores).all()) and not bool(res.flags.any())
    assert torch.equal(res.scores, ev.score_masks(res.parents))
    masks = lambda t: t.cpu().numpy().view(np.uint64)
    assert not any(hc.has_cycle(row) for row in masks(res.parents)) and not any(hc.has_cycle(row) for row in masks(res.last_parents))
    other = tabu_search(ev, starts, restarts=2, perturb=3, seed=6, **kw)
    assert not torch.equal(other.last_parents, res.last_parents)              # another seed, another walk
    assert torch.equal(starts, kept)                                         # the caller's masks are not searched in place
    empty = tabu_search(ev, batch=2, **kw)
    assert torch.equal(empty.parents[0], plain.parents[0]) and torch.equal(empty.parents[1], plain.parents[0])
    bad = starts.clone()
    bad[5, 0] |= 1 << 1
    bad[5, 1] |= 1 << 0                                   # 0 <-> 1
    with pytest.raises(ValueError, match=r"tabu_search: starts with a cycle: rows \[5\]"):
        tabu_search(ev, bad, max_steps=4)
    bad = starts.clone()
    bad[2, 3] |= 1 << 20                                  # a parent bit >= n_vars
    with pytest.raises(ValueError, match=r"rows \[2\]"):
        tabu_search(ev, bad, max_steps=4)
    for wrong in (dict(tabu=0), dict(max_tabu=0), dict(restarts=-1), dict(perturb=0)):
        with pytest.raises(ValueError):
            tabu_search(ev, starts, **{**kw, **wrong})


def test_hill_climb_restarts():
    import torch
    from dags_vae_search_amd import hill_climb
    case = hc.hc_case("asia")
    drv = make_driver("asia", "bic", None)
    cached = drv.climb(case.starts, case.max_steps, case.max_parents, case.forbidden, case.min_delta)
    ev, starts = drv.ev, drv._t(case.starts)
    kept = starts.clone()
    kw = dict(max_steps=case.max_steps, min_delta=case.min_delta)
    plain = hill_climb(ev, starts, restarts=0, trace=True, **kw)
    c = lambda x: x.cpu().numpy()
    assert c(plain.parents).view(np.uint64).tobytes() == cached.parents.tobytes() and c(plain.scores).tobytes() == cached.scores.tobytes()
    assert c(plain.steps).tobytes() == cached.steps.tobytes() and c(plain.converged).tobytes() == cached.converged.tobytes()
    assert c(plain.trace[0]).tobytes() == cached.codes.tobytes() and c(plain.trace[1]).tobytes() == cached.deltas.tobytes()
    res = hill_climb(ev, starts, restarts=2, perturb=3, seed=5, **kw)
    again = hill_climb(ev, starts, restarts=2, perturb=3, seed=5, **kw)
    assert _fields(res) == _fields(again)
    head = hill_climb(ev, starts[:5], restarts=2, perturb=3, seed=5, **kw)
    assert torch.equal(head.parents, res.parents[:5]) and torch.equal(head.scores, res.scores[:5])
    assert bool((res.scores >= plain.scores).all())
    assert torch.equal(res.scores, ev.score_masks(res.parents)) and bool(res.converged.all())
    assert not any(hc.has_cycle(row) for row in c(res.parents).view(np.uint64))
    assert torch.equal(starts, kept)
    bad = starts.clone()
    bad[5, 0] |= 1 << 1
    bad[5, 1] |= 1 << 0
    with pytest.raises(ValueError, match=r"hill_climb: starts with a cycle: rows \[5\]"):
        hill_climb(ev, bad, max_steps=4, restarts=1)


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    tb.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
