"""The greedy hill climb (csrc/dvs_hillclimb.h: dvs_bn_toggle_scores, dvs_hc_step) on the host emulator: every case,
reference, tolerance and check comes from tests/hillclimb_corpus.py, which tests/test_gpu_hillclimb.py runs unchanged on the
device through BNLearnWrapper.toggle_scores and hill_climb."""
import ctypes
import functools

import pytest

from tests import hillclimb_corpus as hc

CASES = [(name, typ, arg) for name in hc.CASE_NAMES for typ, arg in hc.case_types(name)]


@functools.lru_cache(maxsize=None)
def make_driver(name, typ, arg):
    from tests.emu.harness import emu
    return hc.Driver(hc.sc.EmuBackend(emu()), hc.any_case(name), typ, arg)


@pytest.mark.parametrize("name", hc.TOGGLE_CASES)
@pytest.mark.parametrize("typ,arg", hc.TOGGLE_VARIANTS)
def test_emu_toggle_table_is_dvs_bn_scores_bit_for_bit(name, typ, arg):
    hc.check_toggle_exact(make_driver(name, typ, arg), hc.toggle_masks(name))


def test_emu_refused_family_is_nan_in_its_cell_alone_and_never_taken():
    hc.check_toggle_refusal(make_driver("keybits", "bic", None))


@pytest.mark.parametrize("name,typ,arg", [("asia", "bic", None), ("asia", "bde", 10.0), ("sachs", "bic", None),
                                          ("syn17", "bic", None), ("syn48", "bic", None)])
def test_emu_incremental_pass_equals_full_pass(name, typ, arg):
    case = hc.hc_case(name)
    assert hc.check_incremental_equals_full(make_driver(name, typ, arg), case.starts, case.max_parents) >= len(case.starts)


def test_emu_hand_made_legality_cases():
    hc.check_hand_made(make_driver("single", "bic", None))


@pytest.mark.parametrize("name,typ,arg", CASES)
def test_emu_trace_replays_exactly_and_is_greedy_for_the_oracle(name, typ, arg):
    """Layers 2 and 3 on one climb per case.  Worst margin used / tau on the emulator build: DESIGN.md §14."""
    case = hc.hc_case(name)
    hc.reference_climb(name, typ, arg)                   # max_steps is enough for the reference alone; the case shows its point
    drv, r = hc._climb_cached(make_driver, name, typ, arg)
    assert not r.flags.any() and r.converged.all()
    hc.check_replay(drv, case, r)
    worst = hc.check_against_oracle(case, typ, arg, r)
    print(f"\nemulator {name} {typ}: steps {r.steps.tolist()}, worst margin / tau = {worst:.3g}")
    if name == "asia":
        known, T = hc.asia_known_score(typ, arg)
        print(f"asia {typ}: from the empty graph {r.scores[0]!r}, the reference's asia DAG {known!r}")
        if typ == "bic":
            assert r.scores[0] >= known - hc.TAU_RTOL * T


def test_emu_two_climbs_are_bytewise_equal_and_a_batch_is_its_rows():
    case = hc.hc_case("asia")
    drv, r = hc._climb_cached(make_driver, "asia", "bic", None)
    again = drv.climb(case.starts, case.max_steps, case.max_parents, case.forbidden, case.min_delta)
    for a, b in zip(r[:7], again[:7]):
        assert a.tobytes() == b.tobytes()
    head = drv.climb(case.starts[:5], case.max_steps, min_delta=case.min_delta)
    assert head.parents.tobytes() == r.parents[:5].tobytes() and head.scores.tobytes() == r.scores[:5].tobytes()
    assert head.steps.tobytes() == r.steps[:5].tobytes() and head.codes.tobytes() == r.codes[:5].tobytes()
    assert head.deltas.tobytes() == r.deltas[:5].tobytes()


def test_emu_max_steps_stops_a_climb_without_marking_it_converged():
    case = hc.hc_case("asia")
    drv, r = hc._climb_cached(make_driver, "asia", "bic", None)
    short = drv.climb(case.starts[:5], 2, min_delta=case.min_delta)
    for b in range(5):
        k = min(2, int(r.steps[b]))
        assert short.steps[b] == k and short.codes[b, :k].tolist() == r.codes[b, :k].tolist()
        assert short.converged[b] == (1 if r.steps[b] < 2 else 0)


def test_emu_argument_refusals():
    from tests.emu.harness import emu
    hc.check_argument_refusals(emu(), ctypes.c_void_p(4096))


def test_device_library_argument_refusals_without_a_device():
    from dags_vae_search_amd import _lib as dl
    hc.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))
