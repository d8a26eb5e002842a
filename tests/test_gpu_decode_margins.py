"""GPU: dvs_decode's probabilities through the raw C ABI, pinned by threshold-bracketing draws against the float64 trace
of oracle/decode.py.  Cases, tolerance and the check functions are those of tests/decode_corpus.py, shared with the emulator
twin tests/test_emu_decode_margins.py (which also asserts the conditions that need the reference alone)."""
import numpy as np
import pytest
import torch

from tests import decode_corpus as dc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_decode_equals_float64_reference_under_bracketing_draws(be, name):
    """Every dvs_decode_state byte of every row (nv, labels, all 48 parent words, finished, zero tails) equals the float64
    reference with every uniform tau(case) = max(32 * d32, 1e-6) from the reference's threshold; a second call gives the same
    bytes.  A failure names row, step and candidate."""
    c = dc.case(name, dc.CASES[name][4])
    print("\n" + dc.report_line(c))
    dc.check_case(be, c)


def test_bracketing_draws_past_one_pass_of_the_persistent_grid(be):
    """n12c12 at B = 4 * CUs + 5: k_decode_step's grid is capped at the CU count with four DAGs per workgroup, so the last
    five rows are decoded in a second trip of the workgroups' loop; the stack kernels switch to 8 waves per workgroup."""
    B = 4 * int(be.lib.dvs_device_cus()) + 5
    c = dc.case(dc.GRID_CASE, B)
    print("\n" + dc.report_line(c))
    assert c.forced == 0 and dc.TAU_FLOOR <= c.tau <= dc.TAU_CAP
    dc.check_case(be, c)


@pytest.mark.parametrize("name", dc.COUNTER_CASES)
def test_counter_draws_equal_the_restated_stream(be, name):
    """uniforms = NULL, seed S: the device's graphs equal the float64 reference under oracle.rng.decode_uniforms(S, B, N, 0);
    rows [3:] decoded alone at dag_offset 3 equal rows [3:] of the offset-0 call."""
    dc.check_counter_draws(be, name, dc.COUNTER_ROWS, 3)


def test_report_last_step_threshold_error(be):
    """Report only: the smallest tau of the ladder at which every LAST-step decision of the device agrees with the float64
    reference (its implied threshold error).  Asserts only that agreement is monotone in tau."""
    for name in dc.LADDER_CASES:
        rungs, first = dc.last_step_ladder(be, name, dc.CASES[name][4])
        print(f"\ndecode {name}: last-step decisions agree from tau = {first} on   {rungs}")
