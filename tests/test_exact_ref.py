"""CPU pins of the references of tests/exact_corpus.py, before any kernel is trusted against them: ref_dp's vectorised
best-parents sweep against direct subset enumeration (ref_best_brute), and the whole of ref_dp against the maximum over every
labelled DAG (ref_all_dags)."""
import numpy as np
import pytest

from tests import exact_corpus as ex


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("kind", ["random", "ties", "nan"])
def test_ref_dp_best_parents_equal_subset_enumeration(n, kind):
    table = ex.make_tables(kind, 1, n, seed=n)[0]
    if kind == "nan" and n > 1:
        table[0, n - 1] = np.nan                                           # one column with no empty parent set
    rng = np.random.default_rng(n)
    for cap, forb in ((None, None), (1, None), (2, ex.random_forbidden(rng, n))):
        best, arg = ex.ref_best_brute(table, cap, forb)
        ref = ex.ref_dp(table, cap, forb)
        free = ex.free_cells(n)
        assert ref.best[free].tobytes() == best[free].tobytes()
        assert ref.arg[free].astype(np.int64).tobytes() == arg[free].tobytes()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_ref_dp_is_the_maximum_over_all_labelled_dags(n):
    assert len(ex.dag_rows(n)) == {1: 1, 2: 3, 3: 25, 4: 543, 5: 29281}[n]
    tables = ex.make_tables("integers", 6, n, seed=n)
    rng = np.random.default_rng(n)
    for cap, forb in ((None, None), (1, None), (2, ex.random_forbidden(rng, n))):
        for table in tables:
            ref = ex.ref_dp(table, cap, forb)
            assert ref.score == ex.ref_all_dags(table, cap, forb) and not ref.flag
            assert sum(table[int(ref.parents[v]), v] for v in range(n)) == ref.score
