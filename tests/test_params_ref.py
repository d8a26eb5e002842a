"""CPU only: the restatements of tests/params_corpus.py themselves.  The sampler's restatement is a fair sampler of its tables
(a G-test per table row); the byte-equality cases of test_emu_params.py / test_gpu_params.py carry that over to the kernels."""
import math

import mpmath
import numpy as np
import pytest

from tests import params_corpus as pm
from tests import scoring_corpus as sc


def g_test_network():
    card = np.asarray([2, 3, 4, 2, 16], np.uint8)
    masks = sc.masks_of(5, {1: [0], 2: [0, 1], 3: [2], 4: [1, 3]})[0]
    return pm.Network("gtest", card, masks, pm.random_tables(card, masks, 301))


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_restated_sampler_passes_a_g_test_on_every_table_row(seed):
    """200 000 rows; every (variable, configuration) row seen at least 1 000 times: G = 2 sum O log(O / E) against chi-square
    with r - 1 degrees of freedom, at an overall level of 1e-3 shared by the rows tested (Bonferroni)."""
    net = g_test_network()
    levels = pm.sample_ref(net, 200000, seed)
    tests = []
    for v in range(5):
        ps, q, r = pm.family_shape(net.card, net.masks[v], v)
        counts = np.bincount(pm.config_keys(levels, net.card, ps) * r + levels[:, v], minlength=q * r).reshape(q, r)
        for j in range(q):
            nj = int(counts[j].sum())
            if nj < 1000:
                continue
            g = 2.0 * math.fsum(int(o) * math.log(int(o) / (nj * float(t))) for o, t in zip(counts[j], net.tables[v][j]) if o)
            tests.append((v, j, nj, float(mpmath.gammainc((r - 1) / 2.0, max(g, 0.0) / 2.0, mpmath.inf, regularized=True))))
    assert len(tests) >= 15, len(tests)
    worst = min(tests, key=lambda t: t[3])
    print(f"seed {seed}: {len(tests)} rows tested, smallest p {worst[3]:.3e} at variable {worst[0]} configuration {worst[1]}")
    assert worst[3] >= 1e-3 / len(tests), worst


def test_thresholds_never_admit_a_zero_probability_level():
    net = pm.network("zeroone")
    for v, t in enumerate(net.tables):
        T = pm.thresholds(t)
        assert (np.diff(T.astype(np.int64), axis=1) >= 0).all() and (T[:, -1] == 1 << 31).all()
        lower = np.concatenate([np.zeros((len(T), 1), np.int64), T[:, :-1].astype(np.int64)], 1)
        width = np.minimum(T.astype(np.int64), 1 << 31) - lower          # draws that give level k
        assert ((width == 0) == (t == 0.0)).all(), v
        assert (np.abs(width / 2.0 ** 31 - t) <= 2.0 ** -30).all()


def test_fit_reference_rows_are_probability_vectors():
    case = pm.fit_case("sixS255")
    counts = pm.family_counts(case.data, case.card, case.masks[0, 3], 3)
    assert counts.sum() == 255 and (counts.sum(1) == 0).any()
    mle = pm.fit_reference(counts, 0, None, 0)
    assert np.isnan(mle[counts.sum(1) == 0]).all() and np.allclose(mle[counts.sum(1) > 0].sum(1), 1.0)
    assert (pm.fit_reference(counts, 0, None, 1)[counts.sum(1) == 0] == 0.5).all()
    for iss in pm.ISS_VALUES:
        assert np.allclose(pm.fit_reference(counts, 1, iss, 0).sum(1), 1.0, rtol=0, atol=1e-15)


def test_offsets_and_topological_order():
    case = pm.fit_case("sixS1")
    off = pm.offsets_of(case.card, case.masks)
    assert off[0] == 0 and len(off) == 19 and (np.diff(off) > 0).all()
    assert len({int(off[b * 6 + 6] - off[b * 6]) for b in range(3)}) == 3       # the structures' sizes differ
    net = pm.network("chain48")
    assert pm.topological_order(net.masks)[0] == 47
