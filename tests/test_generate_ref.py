"""CPU: the SPECIFICATION of the device graph generator, on its numpy restatement alone (tests/generate_corpus.py): every
accepted graph is a connected DAG with m edges, the accepted graphs are uniform over the connected graphs, slots and labels
are uniform, and encoder_dag_train_schema gives the reference's values.  Seeds are fixed, so every statistic below is one
deterministic number; the bounds are the 99.9 % quantiles of the chi-square distribution the statistic has under the
specification (15: 37.70, 221: 291.7 — the issue's "about 290" is used —, 27: 55.48, 7: 24.32, 4: 18.47)."""
import collections
import json
import os

import numpy as np
import pytest

from dags_vae_search_amd.generate import encoder_dag_train_schema
from tests import generate_corpus as gc

HERE = os.path.dirname(os.path.abspath(__file__))


def _components(n, edges):
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for u, v in edges:
        parent[find(u)] = find(v)
    return len({find(v) for v in range(n)})


@pytest.mark.parametrize("name", ["n5_m5", "n12_mixed", "n14_m20", "n45_m90"])
def test_accepted_graphs_are_connected_dags_with_m_edges(name):
    c = gc.CASES[name]
    labels, preds, attempts = gc.reference(name)
    m = gc.edge_counts(c)
    ok = attempts > 0
    assert ok.sum() >= 0.9 * len(m)
    assert (gc.popcount(preds).sum(1)[ok] == m[ok]).all()
    for v in range(c["n"]):                                    # a DAG in vertex order: row v holds vertices below v only
        assert (preds.astype(np.uint64) >> np.uint64(v) == 0)[:, v].all()
    for b in np.nonzero(ok)[0][:300]:
        assert _components(c["n"], gc.edge_sets(preds[b:b + 1])[0]) == 1
    assert (preds[~ok] == 0).all() and (labels[~ok] == 0).all()


@pytest.mark.parametrize("n,m,seed,draws,graphs,bound", [(4, 3, 7, 16000, 16, 37.7), (5, 5, 11, 22200, 222, 290.0)])
def test_accepted_graphs_are_uniform_over_the_connected_graphs(n, m, seed, draws, graphs, bound):
    _, preds, attempts = gc.generate(n, n, m, draws, seed=seed)
    assert (attempts > 0).all()
    hist = collections.Counter(gc.edge_sets(preds))
    assert len(hist) == graphs                                 # 16 spanning trees of K4; 222 connected 5-edge graphs on 5 vertices
    exp = draws / graphs
    chi2 = sum((k - exp) ** 2 / exp for k in hist.values())
    print(f"n = {n}, m = {m}: chi2 = {chi2:.1f} on {graphs - 1} d.o.f.")
    assert chi2 < bound


def test_prototype_figures():
    """The figures the specification's prototype gave (mean attempts, failures) are those of this restatement."""
    _, _, a = gc.generate(12, 12, 11, 2000, seed=3)
    assert (a == 0).sum() == 6 and abs(a[a > 0].mean() - 16.7) < 0.1
    _, _, a = gc.generate(12, 12, 26, 2000, seed=3)
    assert abs(a.mean() - 1.03) < 0.005
    assert abs(gc.reference("n45_m90")[2].mean() - 1.9) < 0.05
    assert (gc.reference("n45_m198")[2] == 1).all()


def test_shared_cases_cover_what_they_are_for():
    a = gc.reference("n8_m7_try2")[2]
    assert (a == 0).sum() >= 64 and (a > 0).sum() >= 16
    a = gc.reference("n12_mixed")[2]
    assert a.max() > 64 and (a == 0).sum() == 1               # a 64-lane group needs a second round; one DAG fails
    assert gc.reference("n45_m90")[2].max() > 1
    assert (gc.reference("n45_m198")[1][:, 44] >> np.uint64(43)).any()    # the highest bit there is: edge 43 -> 44
    a = gc.reference("n8_m_out_of_range")[2]
    assert (a.reshape(-1, 4)[:, [0, 3]] == -1).all() and (a.reshape(-1, 4)[:, [1, 2]] > 0).all()
    # accept_isolates accepts graphs the default rejects
    c = gc.CASES["n8_isolates"]
    strict = gc.generate(8, 8, 7, c["B"], seed=c["seed"])[2]
    assert (gc.reference("n8_isolates")[2] <= strict).all() and (gc.reference("n8_isolates")[2] < strict).any()


def test_slot_inclusion_is_uniform():
    """Without the connectivity test every slot is taken with probability m / P.  The counts X_t of N draws are exchangeable
    with a fixed sum, so sum (X_t - N p)^2 / (N p (1 - p)) * (P - 1) / P is chi-square with P - 1 = 27 d.o.f."""
    n, m, N = 8, 10, 20000
    P = n * (n - 1) // 2
    _, preds, attempts = gc.generate(n, n, m, N, seed=17, flags=gc.ACCEPT_NO_CONNECTIVITY)
    assert (attempts == 1).all()
    counts = np.asarray([((preds[:, v] >> np.uint16(u)) & 1).sum() for v in range(1, n) for u in range(v)], np.float64)
    assert counts.sum() == N * m
    p = m / P
    chi2 = ((counts - N * p) ** 2 / (N * p * (1 - p))).sum() * (P - 1) / P
    print(f"slot inclusion: chi2 = {chi2:.1f} on {P - 1} d.o.f.")
    assert chi2 < 55.48


def test_labels():
    N, n, card = 20000, 8, 8
    key = gc.rng.site_key(29, gc.SITE_LABELS, np.arange(N, dtype=np.uint64))
    lab = gc.draw_labels(key, n, card, choice=False)
    assert (np.sort(lab, axis=1) == np.arange(card)).all()     # card == n: a permutation, so injective
    wide = gc.draw_labels(key, n, 45, choice=False)
    assert all(len(set(r)) == n for r in wide[:2000].tolist()) and wide.max() == 44 and wide.min() == 0
    for v in range(n):                                         # every value equally frequent at every position
        chi2 = ((np.bincount(lab[:, v], minlength=card) - N / card) ** 2 / (N / card)).sum()
        assert chi2 < 24.32, (v, chi2)
    ch = gc.draw_labels(key, n, 5, choice=True)
    chi2 = ((np.bincount(ch.reshape(-1), minlength=5) - N * n / 5) ** 2 / (N * n / 5)).sum()
    assert chi2 < 18.47 and ch.max() == 4
    assert (gc.draw_labels(key[:50], n, 1, choice=True) == 0).all()


def test_schema_equals_the_reference():
    with open(os.path.join(HERE, "golden", "encoder_schema.json")) as f:
        golden = json.load(f)
    assert [(g["num_vertices"], g["density_limit"], g["steps_limit"]) for g in golden] == \
        [(12, 0.4, 20), (8, 0.6, 20), (37, 0.2, 20), (45, 0.4, 7), (5, 1.0, 3)]
    for g in golden:
        got = encoder_dag_train_schema(g["num_vertices"], g["density_limit"], g["steps_limit"])
        assert [list(e) for e in got] == g["schema"]
        assert all(isinstance(m, int) and isinstance(k, int) for m, k in got)


@pytest.mark.parametrize("args,word", [((0, 0.4, 20), "num_vertices"), ((12, 0.0, 20), "density_limit"),
                                       ((12, 1.5, 20), "density_limit"), ((12, 0.4, 0), "steps_limit"),
                                       ((12, 0.1, 20), "max_edges_density")])
def test_schema_value_errors(args, word):
    with pytest.raises(ValueError, match=word):
        encoder_dag_train_schema(*args)


def test_python_entry_refusals_need_no_device():
    from dags_vae_search_amd import generate_dags
    with pytest.raises(AssertionError, match="Expected at least 11 edges"):
        generate_dags(12, 12, 10, 4, seed=0)
    with pytest.raises(ValueError, match="label_random_method"):
        generate_dags(12, 12, 11, 4, seed=0, label_random_method="shuffle")
    with pytest.raises(RuntimeError, match="no CPU path"):
        generate_dags(12, 12, 11, 4, seed=0, device="cpu")
