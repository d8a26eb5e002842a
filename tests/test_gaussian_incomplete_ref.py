"""CPU: the eleventh companion header (include/dvs_gaussian_incomplete.h) as the binding reads it, and the Python restatement of
its definitions (tests/gaussian_incomplete_corpus.py) against mpmath at 60 digits, which conditions the joint by a solve on the
observed block and shares no formula with the header.  The emulator and GPU twins run the same corpus through the C ABI.

Apart from the header binding, the tests here check the oracle, not the library: they would pass without the kernel.  The tests
that fail without the feature are the header binding here and everything in the emulator and GPU files."""
import math

import mpmath as mp
import numpy as np
import pytest

from dags_vae_search_amd import _lib as dl
from tests import gaussian_corpus as gc
from tests import gaussian_incomplete_corpus as gi
from tests import gaussian_params_corpus as gp


def test_header_binding():
    assert list(dl.GINC_SIGNATURES) == ["dvs_gbn_condition_workspace_bytes", "dvs_gbn_condition"]
    others = (dl.SIGNATURES, dl.EXT_SIGNATURES, dl.INC_SIGNATURES, dl.AVAIL_SIGNATURES, dl.LOCAL_SIGNATURES, dl.PERM_SIGNATURES,
              dl.GAUSS_SIGNATURES, dl.GCI_SIGNATURES, dl.GPAR_SIGNATURES, dl.MIXED_SIGNATURES, dl.MPAR_SIGNATURES)
    assert all(not set(dl.GINC_SIGNATURES) & set(t) for t in others)
    assert [len(t) for t in others] == [64, 1, 5, 2, 2, 2, 5, 2, 6, 8, 6] and dl.ABI_VERSION == 202
    assert dl.signature("dvs_gbn_condition") is dl.GINC_SIGNATURES["dvs_gbn_condition"]
    assert [k for k, _ in dl.GINC_SIGNATURES["dvs_gbn_condition"][1]] == [
        "n_vars", "n_rows", "mean", "cov", "x", "observed", "order", "completed", "cvar", "quad", "logp", "loglik", "ccov", "counts",
        "workspace", "workspace_bytes", "status", "stream"]
    assert [k for k, _ in dl.GINC_SIGNATURES["dvs_gbn_condition_workspace_bytes"][1]] == ["n_vars", "n_rows"]
    with pytest.raises(KeyError, match=r"dvs_mixed_params\.h, nor in include/dvs_gaussian_incomplete\.h'$"):
        dl.signature("dvs_gbn_nothing")


def test_a_missing_header_is_an_error_that_gives_its_path(tmp_path):
    with pytest.raises(RuntimeError, match="include/dvs_gaussian_incomplete.h not found at"):
        dl._read_header(str(tmp_path / "dvs_gaussian_incomplete.h"))


def _cases(n):
    """(x [S, n], masks [S]): all observed, none, one observed, one missing, the whole Markov blanket of three targets (nothing
    else), then seeded masks"""
    net = gp.NETS[gi.NET_KEYS[n]]
    S = 24 if n < 48 else 10
    x = gp.rows_for(n, S)
    masks = gi.masks_for(n, S, "mixed", seed=1)
    targets = gp.sinks_and_sources(net) if n >= 5 else ()
    for i, t in enumerate(targets):
        masks[4 + i] = gi.blanket_mask(net, t)
    return net, x, masks, targets


@pytest.mark.parametrize("n", gi.N_VALUES)
def test_restatement_against_mpmath(n):
    net, x, masks, targets = _cases(n)
    if n == 48:
        assert len(net.pa(n // 2 - 1)) == 47
    res = gi.restated(n, x, masks)
    assert not res.refused.any()
    worst = gi.assert_rows_against_reference(n, x, masks, res, range(len(x)))
    gi.assert_sums_against_reference(n, x, masks, res)
    gi.assert_sums_against_reference(n, x, masks, gi.restated(n, x, masks, gi.sorted_order(masks)), gi.sorted_order(masks))
    low = (1 << n) - 1
    assert int(masks[0]) == low and int(masks[1]) == 0
    assert np.float64(res.logp[1]).tobytes() == np.float64(-0.0).tobytes() and gi.same(res.completed[1], gi.joint_of(n)[0])
    print(f"n {n}: largest error / bound {worst:.3e}, kappa_F up to "
          f"{max(gi.pattern_reference(n, int(m)).kappa_F for m in masks):.3e}")


@pytest.mark.parametrize("n", (5, 17, 48))
def test_the_whole_blanket_observed_meets_the_exact_prediction(n):
    """conditioning on the Markov blanket alone is conditioning on every other variable: gaussian_predict(method="exact")'s
    restatement and this one meet within the sum of their bounds"""
    net, x, masks, targets = _cases(n)
    res = gi.restated(n, x, masks)
    for i, t in enumerate(targets):
        r = 4 + i
        assert not (int(masks[r]) >> t) & 1
        pred, var = gp.restated_predict(net, t, 1, x[r:r + 1])
        bound, rel = gp.predict_bound(net, t, x[r])
        b = gi.row_reference(n, int(masks[r]), x[r])[3]
        ref = gi.pattern_reference(n, int(masks[r]))
        assert abs(float(pred[0]) - float(res.completed[r, t])) <= bound + b.mean + gc.U * abs(float(pred[0])), (n, t)
        assert abs(var - float(res.cvar[r, t])) <= rel * var + ref.T_bound, (n, t)


@pytest.mark.parametrize("n", gi.N_VALUES)
def test_every_variable_observed_meets_the_network_log_likelihood(n):
    S = 12 if n < 48 else 6
    net, x = gp.NETS[gi.NET_KEYS[n]], gp.rows_for(n, S)
    masks = np.full(S, (1 << n) - 1, np.uint64)
    res = gi.restated(n, x, masks)
    rest = gp.restated_loglik_rows(net, x)
    for i in range(S):
        _, other = gp.exact_loglik_row(net, x[i])
        mine = gi.row_reference(n, int(masks[i]), x[i])[3].logp
        assert abs(float(rest[i]) - float(res.logp[i])) <= other + mine, (n, i, rest[i], res.logp[i], other, mine)


def test_vectorised_restatement_equals_the_scalar_one_as_bytes():
    for n in (1, 5, 17):
        mean, cov = gi.joint_of(n)
        x, masks = gp.rows_for(n, 40), gi.masks_for(n, 40, "mixed", seed=2)
        res = gi.restated(n, x, masks)
        for r in range(40):
            completed, cvar, q, logp, T = gi.restated_row(mean, cov, x[r], masks[r])
            assert gi.same(res.completed[r], np.asarray(completed)) and gi.same(res.cvar[r], np.asarray(cvar)), (n, r)
            assert np.float64(q).tobytes() == res.quad[r].tobytes() and np.float64(logp).tobytes() == res.logp[r].tobytes(), (n, r)
            mis = np.asarray([not (int(masks[r]) >> v) & 1 for v in range(n)])
            assert gi.same(np.where(np.outer(mis, mis), res.factors[int(masks[r])][6], 0.0), np.asarray(T).reshape(n, n))


def test_refusals_in_the_restatement():
    n = 5
    mean, _ = gi.joint_of(n)
    x = np.array(gp.rows_for(n, 4), copy=True)
    dup = gi.duplicated_cov(n, 1, 3)
    assert gi.restated_row(mean, dup, x[0], 0b01010) is None and gi.restated_row(mean, dup, x[0], 0b11111) is None
    assert gi.restated_row(mean, dup, x[0], 0b00010) is not None and gi.restated_row(mean, dup, x[0], 0b10101) is not None
    assert gi.restated_row(mean, gi.joint_of(n)[1], x[0], 1 << n) is None
    x[1, 2] = math.nan
    assert gi.restated_row(mean, gi.joint_of(n)[1], x[1], 0b00100) is None
    assert gi.restated_row(mean, gi.joint_of(n)[1], x[1], 0b11011) is not None
    res = gi.restated(n, x, np.asarray([0b01010, 0b00100, 1 << n, 0b10101], np.uint64), cov=dup)
    assert list(res.refused) == [True, True, True, False] and res.counts == 3 and res.status == 16


def test_a_run_across_a_chunk_boundary_is_two_runs():
    """13 rows of one mask at positions 250 .. 262: ccov adds 6 T and 7 T in two chunks, and the two-level sum of those"""
    n, S = 5, 300
    masks = gi.straddle_masks(n, S)
    x = gp.rows_for(n, S)
    res = gi.restated(n, x, masks)
    T = {m: np.where(np.outer(*(2 * [np.asarray([not (m >> v) & 1 for v in range(n)])])), res.factors[m][6], 0.0) for m in (0b00101, 0b01001, 0b11010)}
    c0 = (0.0 + 250.0 * T[0b00101]) + 6.0 * T[0b01001]
    c1 = (0.0 + 7.0 * T[0b01001]) + 37.0 * T[0b11010]
    assert gi.same(res.ccov, c0 + c1)


def test_restated_em_meets_the_closed_form_at_the_recorded_settings():
    """the settings the GPU test uses (CLOSED_ITERATIONS, CLOSED_RTOL) are chosen here: the restatement alone is inside the
    tolerance, the cross-products are as well conditioned as its derivation says, and the linear rate is the missing fraction"""
    x, masks = gi.closed_form_case()
    assert 0.3 < np.mean(masks == 1) < 0.37
    xc = x - x.mean(0)
    assert np.linalg.cond(xc.T @ xc) < 20
    net = gi.start_net(gi.CLOSED_NET.parents, x, masks)
    slope = gi.closed_form(x, masks)[1]
    errs, trace = [], []
    for _ in range(gi.CLOSED_ITERATIONS):
        net, ll, _ = gi.restated_em_step(net, x, masks)
        errs.append(abs(net.coef[1, 0] - slope))
        trace.append(ll)
    assert all(0.2 < errs[t + 1] / errs[t] < 0.45 for t in range(2, 10)), errs[:12]
    assert all(b >= a - 1e-9 for a, b in zip(trace, trace[1:]))
    part = gi.assert_meets_closed_form(net.coef, net.intercept, net.sd, x, masks, "restatement")
    print(f"restated EM after {gi.CLOSED_ITERATIONS} steps: distance to the closed form / tolerance {part:.3e}")


def test_restated_em_trace_is_monotone_under_the_true_m_step():
    n = 5
    x = gp.restated_sample(("loop", 5), 600, gi.EM_SEED)[0]
    masks = gi.em_masks(600, n, 0.2, gi.EM_MASK_SEED)
    net = gi.start_net(gp.LOOP_NET.parents, x, masks)
    trace = []
    for _ in range(6):
        net, ll, res = gi.restated_em_step(net, x, masks, "mle")
        trace.append(ll)
    assert all(b >= a for a, b in zip(trace, trace[1:])) and trace[-1] - trace[0] > 1.0, trace


def test_the_loop_closes_on_the_restatement_with_a_tenth_of_the_cells_missing():
    """the setting of the GPU test (2000 rows, the recorded mask seed, 12 EM steps under the complete DAG, bge): the restatement
    alone finds the generator's equivalence class among all 29 281 DAGs, with a gap far above any difference between builds"""
    ref = gi.missing_loop_reference()
    assert 0.08 < ref.missing < 0.12
    assert ref.best_key == ref.truth and ref.gap > 1.0, ref.gap
    print(f"closed loop with {ref.missing:.3f} of the cells missing: gap to the best other class {ref.gap:.3f}")
