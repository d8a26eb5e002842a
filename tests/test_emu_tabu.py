"""Tabu search and random perturbation (csrc/dvs_tabu.h: dvs_tabu_step, dvs_hc_perturb) on the host emulator: every case,
reference, tolerance and check comes from tests/tabu_corpus.py, which tests/test_gpu_tabu.py runs unchanged on the device."""
import ctypes
import functools

import pytest

from tests import tabu_corpus as tb


@functools.lru_cache(maxsize=None)
def make_driver(name, typ, arg):
    from tests.emu.harness import emu
    return tb.TabuDriver(tb.sc.EmuBackend(emu()), tb.hc_case(name), typ, arg)


@pytest.mark.parametrize("name", tb.TABU_CASES)
def test_emu_tabu_trace_replays_exactly(name):
    """Layer 1: every traced (code, delta bits), the ring, stall / visited and the best against tabu_select_ref."""
    drv, r = tb._tabu_cached(make_driver, name)
    downhill = tb.check_tabu_replay(drv, tb.tabu_case(name), r)
    print(f"\nemulator {name}: steps {r.steps.tolist()}, moves that lowered the score {downhill}")
    if not tb.tabu_case(name).cut:
        assert downhill > 0


def test_emu_tabu_hand_made_cases():
    tb.check_tabu_hand_made(make_driver("single", "bic", None))


@pytest.mark.parametrize("name", sorted(tb.ESCAPE))
def test_emu_tabu_leaves_the_optimum_greedy_stops_at(name):
    """Layer 3.  Worst margin used / tau on the emulator build: DESIGN.md §15."""
    tc = tb.tabu_case(name)
    ref = tb.reference_tabu(name)
    print(f"\nreference {name}: gain of the tabu best over the greedy final {[(b, g) for b, (_, _, g) in ref.items()]}")
    drv, r = tb._tabu_cached(make_driver, name)
    g = drv.climb(tc.starts, tc.max_steps, tc.hc.max_parents, tc.hc.forbidden, tc.hc.min_delta)
    assert g.converged.all()
    worst = tb.check_tabu_against_oracle(tc, r, g.scores)
    print(f"emulator {name}: worst margin / tau = {worst:.3g}, gains {[float(r.best_score[b] - g.scores[b]) for b in ref]}")


@pytest.mark.parametrize("name", ["asia", "syn17", "syn48"])
def test_emu_perturb_takes_the_drawn_legal_move_and_the_incremental_pass_follows(name):
    taken = tb.check_perturb_case(make_driver(name, "bic", None), name)
    if name == "asia":                                   # 33 structures: two draw indices differ somewhere
        assert taken[7, 1] != taken[7, 0xFFFFFFFF]


def test_emu_perturb_hand_made_cases():
    tb.check_perturb_hand_made(make_driver("single", "bic", None))


def test_emu_two_tabu_runs_are_bytewise_equal_and_a_batch_is_its_rows():
    drv, r = tb._tabu_cached(make_driver, "asia_bde")
    tb.check_tabu_deterministic(drv, tb.tabu_case("asia_bde"), r)


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    tb.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    tb.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
