"""GPU: model averaging (csrc/dvs_strength.h) through the raw calls with the cases, references and checks of
tests/strength_corpus.py — shared with the emulator twin tests/test_emu_strength.py — plus the Python surface
(dags_vae_search_amd/strength.py, BNLearnWrapper.with_rows) and boot_strength end to end on asia."""
import ctypes
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import cpdag_corpus as cp
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc
from tests import strength_corpus as st

pytestmark = pytest.mark.gpu
U64 = np.uint64


@functools.lru_cache(maxsize=None)
def driver():
    from dags_vae_search_amd import _lib as dl
    return st.Driver(sc.GpuBackend(dl.load()))


def _rows(t):
    return t.cpu().numpy().view(U64)


# ---- the raw C ABI: the emulator's checks, unchanged -------------------------------------------------------------------
@pytest.mark.parametrize("set_size", st.SET_SIZES)
@pytest.mark.parametrize("name", st.ROW_DATASETS)
def test_scores_rows_equal_the_plain_scorer_on_gathered_rows(name, set_size):
    st.check_scores_rows(driver(), name, set_size)


@pytest.mark.parametrize("plan", st.toggle_plan(), ids=lambda p: f"{p[0]}-S{p[1]}-{p[2]}-{p[4]}")
def test_toggle_rows_equal_the_plain_toggle_pass_on_gathered_rows(plan):
    st.check_toggle_rows(driver(), *plan)


@pytest.mark.parametrize("name", st.ROW_DATASETS)
def test_identity_row_set_is_the_plain_call(name):
    st.check_identity_set(driver(), name)


def test_row_set_refusals_leave_the_outputs_untouched():
    st.check_rows_refusals(driver())


@pytest.mark.parametrize("set_size", st.BOOT_SET_SIZES)
def test_bootstrap_rows_bytes(set_size):
    st.check_bootstrap_bytes(driver(), set_size)


def test_bootstrap_rows_offsets_and_wrap():
    st.check_bootstrap_offsets(driver())


@pytest.mark.parametrize("n", st.ARC_SIZES)
def test_arc_strength_random_pdags(n):
    st.check_arc_random(driver(), n)


def test_arc_strength_empty_and_complete():
    st.check_arc_extremes(driver())


@pytest.mark.parametrize("n", [3, 8, 48])
def test_averaged_network_random_counts(n):
    st.check_averaged_random(driver(), n)


def test_averaged_network_hand_made():
    st.check_averaged_hand(driver())


def test_averaged_network_sweep_equals_single_calls():
    st.check_averaged_sweep(driver())


def test_library_argument_refusals():
    from dags_vae_search_amd import _lib as dl
    st.check_argument_refusals(dl.load(), ctypes.c_void_p(4096))


# ---- the Python surface ---------------------------------------------------------------------------------------------
def _asia(metric):
    from dags_vae_search_amd import BNLearnWrapper
    case = hc.hc_case("asia")
    return BNLearnWrapper("asia", metric, data=case.data, **({"iss": 10.0} if metric == "bde" else {}))


def test_bootstrap_rows_and_with_rows_validation():
    import torch
    from dags_vae_search_amd import bootstrap_rows
    ev = _asia("bic")
    rows = bootstrap_rows(6, 300, ev.n_samples, seed=st.BOOT_SEED, set_offset=3)
    assert rows.dtype == torch.int32 and rows.shape == (6, 300) and rows.is_cuda
    assert st.same_bytes(rows.cpu().numpy(), st.bootstrap_ref(6, 300, ev.n_samples, st.BOOT_SEED, 3))
    view = ev.with_rows(rows)
    assert (view.lib, view.device, view.n_vars, view.metric_name, view.n_samples) == (ev.lib, ev.device, 8, "bic", 300)
    P = torch.from_numpy(hc.hc_case("asia").starts[:6].view(np.int64).copy()).cuda()
    got = view.score_masks(P)
    for b in range(6):                                                     # structure b on set b = the gathered evaluator
        from dags_vae_search_amd import BNLearnWrapper
        one = BNLearnWrapper.from_packed("asia", "bic", ev.packed[rows[b].long()], ev.card_host)
        assert st.same_bytes(one.score_masks(P[b:b + 1]).cpu().numpy(), got[b:b + 1].cpu().numpy())
    with pytest.raises(ValueError, match="row sets"):
        view.score_masks(torch.cat([P, P]))
    with pytest.raises(ValueError, match="set_of names"):
        ev.with_rows(rows, set_of=torch.zeros(4, dtype=torch.int32)).toggle_scores(P)
    bad = rows.clone()
    bad[2, 7] = ev.n_samples
    with pytest.raises(ValueError, match=r"rows must lie in \[0, "):
        ev.with_rows(bad)
    bad[2, 7] = -1
    with pytest.raises(ValueError, match=r"rows must lie in \[0, "):
        ev.with_rows(bad)
    with pytest.raises(ValueError, match=r"set_of must lie in \[0, 6\)"):
        ev.with_rows(rows, set_of=torch.tensor([0, 6]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        bootstrap_rows(2, 3, 4, seed=0, device="cpu")


def test_arc_strength_fields_and_merge():
    import torch
    from dags_vae_search_amd import ArcStrength, arc_strength
    n = 17
    dags = cp.random_dags(n, 70, cp.SPARSE(n), seed=611)
    x = torch.from_numpy(dags.view(np.int64).copy()).cuda()
    s = arc_strength(x)
    want = st.arc_ref(cp.as_rows([cp.cpdag_ref(row)[0] for row in dags]), n)
    assert isinstance(s, ArcStrength) and s.n_networks == 70 and s.any.dtype == torch.int32 and s.any.shape == (n, n)
    assert st.same_bytes(s.any.cpu().numpy(), want[..., 0]) and st.same_bytes(s.dir2.cpu().numpy(), want[..., 1])
    raw = arc_strength(x, cpdag=False)
    want_raw = st.arc_ref(dags, n)
    assert st.same_bytes(raw.any.cpu().numpy(), want_raw[..., 0]) and st.same_bytes(raw.dir2.cpu().numpy(), want_raw[..., 1])
    assert np.array_equal(s.strength.cpu().numpy(), want[..., 0] / 70.0)
    d = s.direction.cpu().numpy()
    present = want[..., 0] > 0
    assert np.array_equal(d[present], want[..., 1][present] / (2.0 * want[..., 0][present])) and not d[~present].any()
    assert np.allclose((d + d.T)[present], 1.0, rtol=0, atol=1e-15)
    both = arc_strength(x[:30]) + arc_strength(x[30:])
    assert both.n_networks == 70 and torch.equal(both.any, s.any) and torch.equal(both.dir2, s.dir2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        arc_strength(x.cpu())


def test_inclusion_threshold_and_averaged_network_against_the_restatement():
    import torch
    from dags_vae_search_amd import ArcStrength, AveragedNetwork, averaged_network, inclusion_threshold
    n, R = 8, 40
    c = st.random_counts(n, R, seed=8800 + n)
    s = ArcStrength(torch.from_numpy(c[..., 0].copy()).cuda(), torch.from_numpy(c[..., 1].copy()).cuda(), R)
    T = st.threshold_ref([c[u, v, 0] for u, v in st.pairs_of(n)], R)
    assert inclusion_threshold(s) == T / R
    net = averaged_network(s)
    want_p, want_i = st.averaged_ref(c, R, -1)
    assert isinstance(net, AveragedNetwork) and net.parents.shape == (n,) and net.parents.dtype == torch.int64
    assert [int(x) for x in _rows(net.parents)] == want_p and st.is_acyclic(want_p)
    assert (net.threshold, net.placed, net.dropped, net.ties) == (T / R, want_i[1], want_i[2], want_i[3])
    ts = [0.0, 0.25, 0.5, 0.7, 0.85, 1.0]
    sweep = averaged_network(s, ts)
    assert sweep.parents.shape == (len(ts), n) and sweep.threshold == ts
    for g, t in enumerate(ts):
        m = math.floor(Fraction(t) * R) + 1
        want_p, want_i = st.averaged_ref(c, R, m)
        assert [int(x) for x in _rows(sweep.parents[g])] == want_p, t
        assert (sweep.placed[g], sweep.dropped[g], sweep.ties[g]) == want_i[1:], t
        one = averaged_network(s, t)
        assert torch.equal(one.parents, sweep.parents[g]) and one.placed == sweep.placed[g]
    assert sweep.placed[-1] == 0 and sweep.placed[0] >= sweep.placed[1] >= sweep.placed[2]
    with pytest.raises(ValueError):
        averaged_network(s, 1.5)


# ---- boot_strength end to end on asia ------------------------------------------------------------------------------------
def _plain_replicates(ev, metric, search, replicates, seed, **kw):
    """today's composition, one replicate at a time: gather the rows, an evaluator of their own, one search"""
    from dags_vae_search_amd import BNLearnWrapper, bootstrap_rows
    rows = bootstrap_rows(replicates, ev.n_samples, ev.n_samples, seed=seed)
    out = []
    for r in range(replicates):
        one = BNLearnWrapper.from_packed("asia", metric, ev.packed[rows[r].long()], ev.card_host, iss=ev.iss)
        out.append(search(one, batch=1, **kw).parents)
    return out


@pytest.mark.parametrize("metric", ["bic", "bde"])
def test_boot_strength_hc_is_one_plain_hill_climb_per_replicate(metric):
    import torch
    from dags_vae_search_amd import boot_strength, hill_climb
    ev = _asia(metric)
    args = dict(max_steps=40)
    res = boot_strength(ev, replicates=16, algorithm="hc", algorithm_args=args, seed=5, return_networks=True)
    assert res.n_networks == 16 and res.networks.shape == (16, 8) and res.exhausted == 0
    plain = _plain_replicates(ev, metric, hill_climb, 16, 5, **args)
    for r in range(16):
        assert torch.equal(res.networks[r:r + 1], plain[r]), (metric, r)
    nets = _rows(res.networks)
    assert len({row.tobytes() for row in nets}) > 1                         # the replicates do differ
    want = st.arc_ref(cp.as_rows([cp.cpdag_ref(row)[0] for row in nets]), 8)
    assert st.same_bytes(res.any.cpu().numpy(), want[..., 0]) and st.same_bytes(res.dir2.cpu().numpy(), want[..., 1])
    st.check_arc_identities(np.stack([res.any.cpu().numpy(), res.dir2.cpu().numpy()], -1))
    # the result does not depend on the chunking, and shards add up
    for chunk in (5, 16):
        again = boot_strength(ev, replicates=16, algorithm="hc", algorithm_args=args, seed=5, chunk=chunk, return_networks=True)
        assert torch.equal(again.any, res.any) and torch.equal(again.dir2, res.dir2) and torch.equal(again.networks, res.networks)
    lo = boot_strength(ev, replicates=8, algorithm="hc", algorithm_args=args, seed=5, set_offset=0)
    hi = boot_strength(ev, replicates=8, algorithm="hc", algorithm_args=args, seed=5, set_offset=8)
    both = lo + hi
    assert both.n_networks == 16 and torch.equal(both.any, res.any) and torch.equal(both.dir2, res.dir2)
    other = boot_strength(ev, replicates=16, algorithm="hc", algorithm_args=args, seed=6)
    assert not (torch.equal(other.any, res.any) and torch.equal(other.dir2, res.dir2))     # the seed matters
    print(f"\nasia {metric}: strength of the known arcs "
          f"{[round(float(res.strength[u, v]), 2) for v, ps in hc.ASIA_KNOWN.items() for u in ps]}")


@pytest.mark.parametrize("metric", ["bic", "bde"])
def test_boot_strength_tabu_is_one_plain_tabu_search_per_replicate(metric):
    import torch
    from dags_vae_search_amd import boot_strength, tabu_search
    ev = _asia(metric)
    args = dict(max_steps=40, tabu=5)
    res = boot_strength(ev, replicates=8, algorithm="tabu", algorithm_args=args, seed=9, return_networks=True)
    plain = _plain_replicates(ev, metric, tabu_search, 8, 9, **args)
    for r in range(8):
        assert torch.equal(res.networks[r:r + 1], plain[r]), (metric, r)
    want = st.arc_ref(cp.as_rows([cp.cpdag_ref(row)[0] for row in _rows(res.networks)]), 8)
    assert st.same_bytes(res.any.cpu().numpy(), want[..., 0]) and st.same_bytes(res.dir2.cpu().numpy(), want[..., 1])
    raw = boot_strength(ev, replicates=8, algorithm="tabu", algorithm_args=args, seed=9, cpdag=False)
    want_raw = st.arc_ref(_rows(res.networks), 8)
    assert st.same_bytes(raw.any.cpu().numpy(), want_raw[..., 0]) and st.same_bytes(raw.dir2.cpu().numpy(), want_raw[..., 1])


def test_boot_strength_argument_errors():
    from dags_vae_search_amd import boot_strength
    ev = _asia("bic")
    with pytest.raises(ValueError, match="algorithm must be"):
        boot_strength(ev, algorithm="pc", algorithm_args=dict(max_steps=3))
    with pytest.raises(ValueError, match="max_steps"):
        boot_strength(ev, algorithm="hc")
    with pytest.raises(ValueError, match="empty graphs"):
        boot_strength(ev, algorithm="hc", algorithm_args=dict(max_steps=3, batch=4))
    short = boot_strength(ev, replicates=4, m=50, algorithm="hc", algorithm_args=dict(max_steps=1))
    assert short.exhausted == 4 and short.n_networks == 4                   # one step is never enough on asia
