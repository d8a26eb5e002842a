"""dvs_decode's probabilities on the host emulator, pinned by threshold-bracketing draws against the float64 trace of
oracle/decode.py: cases, tolerance and checks are those of tests/decode_corpus.py, which tests/test_gpu_decode_margins.py
runs unchanged on the device.  The conditions that only need the reference (tau within its cap, no forced side, row roles
reached, a counter seed that leaves no row out) are asserted here, for the emulator's and the device's batch alike."""
import numpy as np
import pytest

from oracle import rng as orng
from tests import decode_corpus as dc
from tests import scoring_corpus as sc


@pytest.fixture(scope="module")
def be():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_reference_conditions_hold_at_both_batches(name):
    """From the reference alone: tau = max(32 * d32, 1e-6) stays at or below 2e-5 on every random-init case, no decision there
    is forced to a side, every grower row reaches nv == N (even rows finished by `output` at the last step, odd rows not) and
    every b % 4 == 3 row finishes early at its seeded step.  asia only reports its forced share."""
    for B in dict.fromkeys(dc.CASES[name][3:5]):
        c = dc.case(name, B)
        print("\n" + dc.report_line(c))
        dc.check_reference_conditions(c)
        assert c.decisions > 0 and c.U.dtype == np.float32 and (c.U >= 0).all() and (c.U < 1).all()
    if name == "asia":
        assert 0 < c.forced < c.decisions


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_emu_decode_equals_float64_reference_under_bracketing_draws(be, name):
    """Every dvs_decode_state byte of every row (nv, labels, all 48 parent words, finished, zero tails) equals the float64
    reference with every uniform tau from the reference's threshold; the shapes of at most two tiles are decoded twice for
    equal bytes.  A failure names row, step and candidate."""
    c = dc.case(name, dc.CASES[name][3])
    dc.check_case(be, c, twice=c.cfg.N <= 17)


@pytest.mark.parametrize("name", dc.COUNTER_CASES)
def test_emu_counter_draws_equal_the_restated_stream(be, name):
    """uniforms = NULL: graphs equal the reference under oracle.rng.decode_uniforms, and dag_offset continues the stream.
    The seed must leave no row out: asserted here on all COUNTER_ROWS rows, so that a change of seed cannot empty the test."""
    margin = dc.counter_reference(name)[4]
    assert len(margin) == dc.COUNTER_ROWS and (margin > dc.TAU_CAP).all(), (name, margin)
    assert dc.case(name, dc.CASES[name][4]).tau <= dc.TAU_CAP
    dc.check_counter_draws(be, name, 4, 1)


def test_decode_uniforms_offsets_and_range():
    """The restated stream: row b at dag_offset k is row b + k at offset 0; 24-bit values in [0, 1); another seed, other draws."""
    a = orng.decode_uniforms(dc.COUNTER_SEED, 8, 17, 0)
    assert a.dtype == np.float32 and a.shape == (8, 17, 17) and (a >= 0).all() and (a < 1).all()
    assert np.array_equal(a * np.float32(16777216.0), np.floor(a * np.float32(16777216.0)))
    assert np.array_equal(orng.decode_uniforms(dc.COUNTER_SEED, 5, 17, 3), a[3:])
    assert not np.array_equal(orng.decode_uniforms(dc.COUNTER_SEED + 1, 8, 17, 0), a)
    assert abs(float(a.mean()) - 0.5) < 0.02


def test_report_last_step_threshold_error(be):
    """Report only: the smallest tau of the ladder at which every LAST-step decision of the emulator agrees with the float64
    reference (its implied threshold error).  Asserts only that agreement is monotone in tau."""
    for name in ("n12c12", "asia"):
        rungs, first = dc.last_step_ladder(be, name, 2)       # rows 0 and 1: both arms of the last step
        print(f"\ndecode {name}: last-step decisions agree from tau = {first} on   {rungs}")
