"""GPU: the exact arc posterior (csrc/dvs_posterior.h) through the raw calls with the cases, references and checks of
tests/posterior_corpus.py — shared with the emulator twin tests/test_emu_posterior.py — plus the Python surface
(dags_vae_search_amd/posterior.py): arc_posterior_from_tables, arc_posterior, ArcPosterior.to_arc_strength."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import hillclimb_corpus as hc
from tests import posterior_corpus as po
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def driver():
    from dags_vae_search_amd import _lib as dl
    return po.Driver(sc.GpuBackend(dl.load()))


class GpuReal:
    """the package itself: local_score_table for the table, exact_search for the optimum"""

    def __init__(self, name, typ, arg):
        from dags_vae_search_amd import BNLearnWrapper
        self.case, self.typ, self.arg = hc.hc_case(name), typ, arg
        self.ev = BNLearnWrapper(name, typ, data=self.case.data, **({} if arg is None else {"iss": arg}))
        self.n = self.ev.n_vars

    def table(self, cap):
        from dags_vae_search_amd import local_score_table
        return local_score_table(self.ev, max_parents=cap).cpu().numpy()

    def search(self, table, cap, forbidden):
        from dags_vae_search_amd import exact_search
        r = exact_search(self.ev, max_parents=cap)
        return r.parents.cpu().numpy().view(U64)[0], float(r.scores[0])


@pytest.mark.parametrize("kind", po.KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_posterior_equals_brute_force_over_all_dags(n, kind):
    print("\nworst errors (log, linear):", po.check_brute(driver(), n, kind))


@pytest.mark.parametrize("kind", po.KINDS)
@pytest.mark.parametrize("n", po.STAGE_SIZES)
def test_posterior_every_stage_matches_ref_dp(n, kind):
    if n >= po.BIG and kind != "random":
        return                                                             # the three-pass size runs the plain table only
    print("\nworst errors (log, linear):", po.check_stages(driver(), n, kind))


@pytest.mark.parametrize("n,cap", [(2, None), (2, 1), (9, None), (9, 2), (10, None), (10, 3), (17, None), (17, 4)])
def test_posterior_closed_form_on_the_all_zero_table(n, cap):
    print("\nerrors (log_z, prob):", po.check_closed_form(driver(), n, cap))


@pytest.mark.parametrize("n", [6, 9])
@pytest.mark.parametrize("which", ["offsets", "dominated"])
def test_posterior_on_tables_whose_exp_underflows(which, n):
    print("\nworst errors (log, linear):", po.check_range(driver(), which, n))


@pytest.mark.parametrize("n", [1, 5, 9])
def test_posterior_flag_for_a_table_without_any_dag(n):
    po.check_flags(driver(), n)


def test_posterior_two_calls_give_equal_bytes():
    po.check_determinism(driver())


@pytest.mark.parametrize("typ,arg", [("bic", None), ("bde", 10.0)])
def test_posterior_on_asia(typ, arg):
    po.check_real_asia(GpuReal("asia", typ, arg), driver())


def test_posterior_on_sachs_capped():
    print("\nworst errors (log, linear):", po.check_real_capped(GpuReal("sachs", "bde", 10.0), driver(), 3))


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    po.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


def _same(t, a):
    return t.cpu().numpy().tobytes() == np.ascontiguousarray(a).tobytes()


def test_python_surface_equals_the_raw_call():
    import torch
    from dags_vae_search_amd import ArcPosterior, arc_posterior_from_tables
    n = 6
    tables = po.make_tables("nan", 3, n, seed=2)
    forb = np.zeros(n, U64)
    forb[2] = U64(0b1001)
    raw = driver().posterior(tables, 3, forb)
    dev = torch.from_numpy(tables).cuda()
    post = arc_posterior_from_tables(dev, max_parents=3, forbidden=torch.from_numpy(forb.view(np.int64).copy()).cuda(), families=True)
    assert isinstance(post, ArcPosterior) and post.prob.is_cuda and post.prob.shape == (3, n, n) and post.prob.dtype == torch.float64
    assert post.log_z.shape == (3,) and post.families.shape == (3, 1 << n, n) and not bool(post.flags.any())
    assert _same(post.prob, raw.prob) and _same(post.log_z, raw.log_z) and _same(post.log_z_back, raw.log_z_back)
    assert _same(post.families, raw.family)
    lean = arc_posterior_from_tables(dev, max_parents=3, forbidden=forb)
    assert lean.families is None and torch.equal(lean.prob, post.prob) and torch.equal(lean.log_z, post.log_z)
    s = post.strength
    assert torch.equal(s, post.prob + post.prob.transpose(1, 2))
    d = post.direction
    assert torch.equal(d[s > 0], (post.prob / s)[s > 0]) and not bool(d[s == 0].any()) and bool((s == 0).any())
    assert float(post.prob[:, 0, 2].abs().max()) == 0.0 and float(post.prob[:, 3, 2].abs().max()) == 0.0     # the forbidden arcs
    # parent_prior: "koivisto" is the explicit tensor -log C(n - 1, k); both equal the raw call with that size_prior
    prior = np.array([-math.log(math.comb(n - 1, k)) for k in range(n)])
    a = arc_posterior_from_tables(dev, parent_prior="koivisto")
    b = arc_posterior_from_tables(dev, parent_prior=torch.from_numpy(prior).cuda())
    raw = driver().posterior(tables, None, None, prior)
    assert torch.equal(a.prob, b.prob) and torch.equal(a.log_z, b.log_z) and _same(a.prob, raw.prob) and _same(a.log_z, raw.log_z)
    assert not torch.equal(a.prob, lean.prob)


def test_python_surface_on_an_evaluator():
    import torch
    from dags_vae_search_amd import arc_posterior, arc_posterior_from_tables, local_score_table
    real = GpuReal("asia", "bde", 10.0)
    post = arc_posterior(real.ev, max_parents=3, families=True)
    again = arc_posterior_from_tables(local_score_table(real.ev, max_parents=3)[None], max_parents=3, families=True)
    for f in ("prob", "log_z", "log_z_back", "families", "flags"):
        assert torch.equal(getattr(post, f), getattr(again, f)), f
    assert post.prob.shape == (1, 8, 8)


def test_python_surface_refusals_and_flag_rows():
    import torch
    from dags_vae_search_amd import arc_posterior_from_tables
    tables = po.make_tables("random", 4, 5, seed=1)
    tables[1, :, 0] = np.nan
    tables[3, :, 4] = np.nan
    with pytest.raises(ValueError, match=r"no admissible DAG .*rows \[1, 3\]"):
        arc_posterior_from_tables(torch.from_numpy(tables).cuda())
    with pytest.raises(RuntimeError, match="no CPU path"):
        arc_posterior_from_tables(torch.from_numpy(tables))
    with pytest.raises(TypeError, match="must be a torch tensor"):
        arc_posterior_from_tables(tables)
    with pytest.raises(ValueError, match=r"n_vars = 21 > 20.*2\^n \* n cells"):
        arc_posterior_from_tables(torch.empty(1, 4, 21, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"float64 \[B, 2\^n, n\] \(got 31 rows for n = 5\)"):
        arc_posterior_from_tables(torch.empty(1, 31, 5, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"tables must be float64 \[B >= 1, 2\^n, n\]"):
        arc_posterior_from_tables(torch.empty(1, 32, 5, dtype=torch.float32, device="cuda"))
    good = torch.zeros(1, 32, 5, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError, match="parent_prior must be None, 'koivisto' or a float64"):
        arc_posterior_from_tables(good, parent_prior="uniform")
    with pytest.raises(ValueError, match=r"parent_prior must be None, 'koivisto' or a float64 \[5\] tensor"):
        arc_posterior_from_tables(good, parent_prior=torch.zeros(4, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match=r"parent_prior must be None, 'koivisto' or a float64 \[5\] tensor"):
        arc_posterior_from_tables(good, parent_prior=torch.zeros(5, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="parent_prior must be finite"):
        arc_posterior_from_tables(good, parent_prior=torch.full((5,), float("nan"), dtype=torch.float64, device="cuda"))


def test_to_arc_strength_feeds_the_averaged_network():
    import torch
    from dags_vae_search_amd import ArcStrength, arc_posterior_from_tables, averaged_network, inclusion_threshold
    n = 6
    tables = np.concatenate([po.make_tables("random", 1, n, seed=4, scale=1.0), po.dominated(n)[0]])
    post = arc_posterior_from_tables(torch.from_numpy(tables).cuda())
    for b, R in ((0, 1_000_000), (0, 1000), (1, 1_000_000)):
        st = post.to_arc_strength(b, resolution=R)
        assert isinstance(st, ArcStrength) and st.n_networks == R and st.any.dtype == torch.int32 and st.dir2.dtype == torch.int32
        assert torch.equal(st.dir2 + st.dir2.t(), 2 * st.any) and int(st.any.max()) <= R and int(st.any.min()) >= 0
        assert float((st.any.to(torch.float64) / R - post.strength[b]).abs().max()) <= 2.0 / R
        assert 0.0 <= inclusion_threshold(st) <= 1.0
    assert post.to_arc_strength().n_networks == 1_000_000
    # the dominated table: every arc of the DAG that carries the mass has probability 1, the averaged network is that DAG
    want = po.dominated(n)[1]
    net = averaged_network(post.to_arc_strength(1), threshold=0.5)
    assert net.parents.cpu().numpy().view(U64).tobytes() == want.tobytes() and net.dropped == 0 and net.ties == 0
    assert net.placed == sum(bin(int(p)).count("1") for p in want)
