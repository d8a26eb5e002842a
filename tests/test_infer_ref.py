"""CPU only: the restatements of tests/infer_corpus.py themselves.  The exact-posterior restatement equals brute-force
enumeration of the joint in exact rationals to a tolerance derived from the number of factors, and the likelihood-weighting
restatement lies within 5 standard errors of the exact posterior on a fixed list of seeded evidence sets (the standard error
from the enumeration, not from the sample); the byte-equality cases of test_emu_infer.py / test_gpu_infer.py carry both over to
the kernels."""
import math

import numpy as np
import pytest

from tests import infer_corpus as ic
from tests import params_corpus as pm


def test_vectorised_thresholds_equal_the_sampler_restatement():
    for name in ("zeroone", "small", "hand"):
        for t in pm.network(name).tables:
            assert np.array_equal(ic.thresholds_fast(t), pm.thresholds(t)), name


@pytest.mark.parametrize("M", (1, 255, 256, 257, 1000, 70000))
def test_ordered_sum_is_the_documented_tree(M):
    x = np.random.default_rng(M).random(M)
    chunks = (M + 255) // 256
    padded = np.zeros(chunks * 256)
    padded[:M] = x
    part = []
    for c in range(chunks):                                  # the tree, slot by slot
        y = padded[c * 256:(c + 1) * 256].copy()
        s = 128
        while s:
            for i in range(s):
                y[i] += y[i + s]
            s >>= 1
        part.append(y[0])
    slots = [0.0] * 256
    for c, v in enumerate(part):
        slots[c % 256] += v
    s = 128
    while s:
        for i in range(s):
            slots[i] += slots[i + s]
        s >>= 1
    got = ic.ordered_sum(x)
    assert got == slots[0] and abs(got - math.fsum(x)) <= 64 * 2.0 ** -53 * math.fsum(x)
    assert ic.ordered_sum(np.stack([x, 2 * x]))[1] == 2 * got               # batched along the leading axes


@pytest.mark.parametrize("name", ("hand", "handfour", "asia"))
def test_blanket_restatement_equals_enumeration_of_the_joint(name):
    """every joint state (asia: 256) as the row, every target, use_children = 1: the restated posterior against exact rationals
    of the same fp64 tables, within (factors + levels) * BLANKET_ULPS_PER_FACTOR; use_children = 0 against the target's own
    table row"""
    net = ic.stat_network(name)
    states = ic.enumerate_states(net.card)
    worst = 0.0
    for target in range(len(net.card)):
        post, pred = ic.blanket_ref(states, net.card, net.masks, net.tables, target, 1)
        tol = ic.blanket_tolerance(net, target)
        for s, row in enumerate(states):
            exact = ic.exact_blanket(net, row, target)
            if exact is None:
                assert np.isnan(post[s]).all() and pred[s] == 255
                continue
            for k, e in enumerate(exact):
                err = abs(float(post[s, k]) - float(e)) / float(e) if e else abs(float(post[s, k]))
                assert err <= tol, (name, target, s, k, err, tol)
                worst = max(worst, err / tol)
            top = max(exact)
            assert exact[pred[s]] == top or abs(float(exact[pred[s]] - top)) <= tol * float(top)
        parents_only, _ = ic.blanket_ref(states, net.card, net.masks, net.tables, target, 0)
        ps, _, r = pm.family_shape(net.card, net.masks[target], target)
        rows = net.tables[target][pm.config_keys(states, net.card, ps)]
        assert np.allclose(parents_only, rows / rows.sum(1, keepdims=True), rtol=(1 + r) * ic.BLANKET_ULPS_PER_FACTOR, atol=0)
    print(f"{name}: worst error / tolerance {worst:.3f}")
    assert worst > 0.0 or name == "hand"


@pytest.mark.parametrize("case", ic.STAT_CASES, ids=lambda c: f"{c.network}-{sorted(c.evidence.items())}")
def test_restated_likelihood_weighting_lies_within_five_standard_errors(case):
    worst = ic.stat_check(case)
    print(f"{case}: worst deviation {worst:.2f} standard errors (allowed {ic.STAT_SIGMAS})")


@pytest.mark.parametrize("case", ic.STAT_BLANKET_CASES, ids=lambda c: f"{c.network}-target{c.targets.bit_length() - 1}")
def test_restated_likelihood_weighting_agrees_with_the_exact_blanket_posterior(case):
    worst = ic.stat_check_blanket(case)
    print(f"{case}: worst deviation {worst:.2f} standard errors (allowed {ic.STAT_SIGMAS})")


def test_the_preconditions_do_reject_a_bad_case():
    with pytest.raises(AssertionError, match="cell out of range"):               # P(rain | sprinkler) leaves [0.05, 0.95]
        ic.stat_preconditions(ic.StatCase("hand", {1: 1}, None, 0b101, 0))
    with pytest.raises(AssertionError, match="cell out of range"):               # an event of posterior probability 1
        ic.stat_preconditions(ic.StatCase("hand", {2: 1}, {2: [1]}, 0b011, 0))
    with pytest.raises(AssertionError, match="effective sample size"):           # a good case with too few particles: 233
        ic.stat_preconditions(ic.STAT_CASES[0], M=450)
    assert ic.stat_preconditions(ic.STAT_CASES[0]).ess_ratio * ic.STAT_PARTICLES >= ic.STAT_MIN_ESS


def test_restated_weights_of_the_extreme_masks():
    net = pm.network("hand")
    rows = pm.sample_ref(net, 2, seed=1)
    ref = ic.lw_ref(net, rows, [0, 0b111], 500, 4, 0, None, 0b111)
    assert (ref.weights[0] == 1.0).all() and ref.sums[0, 0] == 500.0 == ref.sums[0, 1]
    assert (ref.levels[1] == rows[1]).all() and ref.marginals[1, 0, int(rows[1, 0])] == ref.sums[1, 0]
    # nothing observed: the particles are a fair sample of the joint (each variable's marginal within 5 binomial sigmas)
    big = ic.lw_ref(net, rows[:1], [0], 20000, 4, 0, None, 0b111)
    exact = ic.lw_exact(net, rows[0], 0, None, 0b111, 20000)
    dev = np.abs(big.marginals[0, :, :2] / 20000 - exact.marginal[:, :2]) / exact.marginal_se[:, :2]
    assert (dev <= 5.0).all(), dev


def test_vectorised_predict_restatement_equals_the_general_one():
    net = ic.asia_network()
    data = pm.sample_ref(net, 6, seed=3)
    for target in (1, 4, 7):
        post, pred = ic.predict_lw_ref(net, data, target, 300, 11, query_offset=40)
        observed = [0xFF & ~(1 << target)] * 6
        ref = ic.lw_ref(net, data, observed, 300, 11, 40, None, 1 << target)
        assert (ref.marginals[:, 0, :2] / ref.sums[:, :1]).tobytes() == post.tobytes()
        assert pred.tolist() == np.argmax(post, 1).tolist()
