"""GPU: exact structure search (csrc/dvs_exact.h) through the raw calls with the cases, references and checks of
tests/exact_corpus.py — shared with the emulator twin tests/test_emu_exact.py — plus the Python surface
(dags_vae_search_amd/exact.py): local_score_table, exact_from_tables, exact_search."""
import ctypes
import functools

import numpy as np
import pytest

from tests import exact_corpus as ex
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def driver():
    from dags_vae_search_amd import _lib as dl
    return ex.Driver(sc.GpuBackend(dl.load()))


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, U64).view(np.int64).copy()).cuda()


class GpuReal:
    """the package itself: local_score_table, score_masks, exact_search / exact_from_tables, hill_climb, tabu_search"""

    def __init__(self, name, typ, arg):
        from dags_vae_search_amd import BNLearnWrapper
        self.case, self.typ, self.arg = hc.hc_case(name), typ, arg
        self.ev = BNLearnWrapper(name, typ, data=self.case.data, **({} if arg is None else {"iss": arg}))
        self.n = self.ev.n_vars

    def local(self, masks):
        out, loc = self.ev.score_masks(_t(masks), local=True)
        return out.cpu().numpy(), loc.cpu().numpy()

    def table(self, cap):
        from dags_vae_search_amd import local_score_table
        t = local_score_table(self.ev, max_parents=cap)
        small = local_score_table(self.ev, max_parents=cap, chunk=37)      # ragged chunks give the same bytes
        assert t.shape == (1 << self.n, self.n) and t.cpu().numpy().tobytes() == small.cpu().numpy().tobytes()
        return t.cpu().numpy()

    def search(self, table, cap, forbidden):
        import torch
        from dags_vae_search_amd import exact_from_tables, exact_search
        forb = None if forbidden is None else _t(forbidden)
        r = exact_search(self.ev, max_parents=cap, forbidden=forb)
        again = exact_from_tables(torch.from_numpy(table).cuda()[None], max_parents=cap, forbidden=forb)
        assert torch.equal(r.parents, again.parents) and torch.equal(r.scores, again.scores) and torch.equal(r.order, again.order)
        assert r.parents.shape == (1, self.n) and r.parents.dtype == torch.int64 and r.order.dtype == torch.int32
        assert r.scores.dtype == torch.float64 and not bool(r.flags.any()) and again.rescored is None
        return r.parents.cpu().numpy().view(U64)[0], float(r.scores[0]), float(r.rescored[0]), r.order.cpu().numpy()[0]

    def heuristics(self, cap, forbidden):
        from dags_vae_search_amd import hill_climb, tabu_search
        forb = None if forbidden is None else _t(forbidden)
        kw = dict(batch=1, max_parents=cap, forbidden=forb, min_delta=self.case.min_delta)
        g = hill_climb(self.ev, max_steps=self.case.max_steps, **kw)
        t = tabu_search(self.ev, max_steps=ex.TABU_STEPS, tabu=ex.TABU_LEN, **kw)
        return float(g.scores[0]), float(t.scores[0])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_exact_score_is_the_maximum_over_all_labelled_dags(n):
    assert ex.check_optimal(driver(), n) == 6


@pytest.mark.parametrize("kind", ex.KINDS)
@pytest.mark.parametrize("n", ex.BYTES_SIZES)
def test_exact_every_stage_equals_ref_dp(n, kind):
    if n >= ex.BIG and kind != "random":
        return                                                             # the three-pass size runs the plain table only
    ex.check_bytes(driver(), n, kind)


@pytest.mark.parametrize("n", [1, 5, 9])
def test_exact_flag_for_a_table_without_any_dag(n):
    ex.check_flags(driver(), n)


@pytest.mark.parametrize("typ,arg", ex.REAL_TYPES)
@pytest.mark.parametrize("name", ["asia", "sachs"])
def test_exact_on_real_data(name, typ, arg):
    ex.check_real(GpuReal(name, typ, arg), name)


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    ex.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def test_python_surface_refusals_and_flag_rows():
    import torch
    from dags_vae_search_amd import ExactResult, exact_from_tables
    tables = ex.make_tables("random", 4, 5, seed=1)
    good = exact_from_tables(torch.from_numpy(tables).cuda(), max_parents=2)
    assert isinstance(good, ExactResult) and good.parents.is_cuda and good.scores.shape == (4,)
    raw = driver().search(tables, 2)
    assert good.parents.cpu().numpy().view(U64).tobytes() == raw.parents.tobytes()
    assert good.scores.cpu().numpy().tobytes() == raw.score.tobytes() and good.order.cpu().numpy().tobytes() == raw.order.tobytes()
    tables[1, :, 0] = np.nan
    tables[3, :, 4] = np.nan
    with pytest.raises(ValueError, match=r"no admissible DAG .*rows \[1, 3\]"):
        exact_from_tables(torch.from_numpy(tables).cuda())
    with pytest.raises(RuntimeError, match="no CPU path"):
        exact_from_tables(torch.from_numpy(tables))
    with pytest.raises(ValueError, match=r"n_vars = 21 > 20.*2\^n \* n cells"):
        exact_from_tables(torch.empty(1, 4, 21, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        exact_from_tables(torch.empty(1, 31, 5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        exact_from_tables(torch.empty(1, 32, 5, dtype=torch.float32, device="cuda"))
