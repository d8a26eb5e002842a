"""GPU: the one evaluator surface (dags_vae_search_amd/evaluator.py) on each of the six evaluator classes, over
one tiny data set.  Expected values come from the raw C ABI (the drivers of tests/*_corpus.py), from numpy or from the other
public call; nothing here is a recording."""
import functools
import threading

import numpy as np
import pytest

from tests import bn_score_corpus as bn
from tests import gaussian_corpus as gc
from tests import mixed_corpus as mc
from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu
U64 = np.uint64
N, S, B = 5, 64, 3
CARD = [2, 3, 3, 2, 3]                     # the discrete data set
MIXED_CARD = [2, 0, 3, 0, 0]               # the mixed one: factors 0 and 2 of the discrete data set, real columns 1, 3, 4
KINDS = ("plain", "rows", "available", "gaussian", "gaussian-rows", "mixed")
DISCRETE_REFUSAL = ("a variable's parent set is too large for the on-chip counting paths (dense table: 36 864 cells; sorted "
                    "samples: 16 384 samples, 63 key bits)")
USED_REFUSAL = "used= is what an available-case view counts (BNLearnWrapper.available_case)"


@functools.lru_cache(maxsize=None)
def backend():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@functools.lru_cache(maxsize=None)
def data():
    """(levels uint8 [S, N], real f64 [S, N], rows int32 [3, 32], observed uint64 [S])"""
    rng = np.random.default_rng(4100)
    levels = np.stack([rng.integers(0, c, S) for c in CARD], 1).astype(np.uint8)
    rows = rng.integers(0, S, (3, 32)).astype(np.int32)
    real = rng.normal(size=(S, N))
    real[:, 3] += 0.8 * real[:, 1] + 0.5 * levels[:, 2]
    real[:, 4] += 0.6 * real[:, 3] - 0.4 * levels[:, 0]
    observed = np.full(S, (1 << N) - 1, U64)
    for r, v in ((0, 0), (3, 2), (3, 4), (17, 1), (40, 3), (63, 4)):
        observed[r] &= ~U64(1 << v)
    return levels, real, rows, observed


def structures():
    """B = 3 structures every kind can score: a factor has factors as parents only"""
    P = np.zeros((B, N), U64)
    P[1, 1], P[1, 2], P[1, 3] = 1 << 0, 1 << 0, 1 << 1
    P[2, 2], P[2, 4] = 1 << 0, (1 << 1) | (1 << 2) | (1 << 3)
    return P


def mixed_rows():
    levels, real, _, _ = data()
    arr = real.copy()
    arr[:, [0, 2]] = levels[:, [0, 2]]
    return arr


@functools.lru_cache(maxsize=None)
def evaluator(kind):
    import torch
    from dags_vae_search_amd import BNLearnWrapper, GaussianEvaluator, MixedEvaluator
    levels, real, rows, observed = data()
    if kind in ("plain", "rows", "available"):
        base = BNLearnWrapper("tiny", "bic", data=levels)
        assert base.card_host == CARD
        if kind == "rows":
            return base.with_rows(torch.from_numpy(rows).cuda())
        return base if kind == "plain" else base.available_case(torch.from_numpy(observed.view(np.int64)).cuda(), "pnal")
    if kind == "mixed":
        return MixedEvaluator("tiny", "bic-cg", data=mixed_rows(), discrete=MIXED_CARD)
    base = GaussianEvaluator("tiny", "bic-g", data=real)
    return base if kind == "gaussian" else base.with_rows(torch.from_numpy(rows))


def device_masks(P):
    import torch
    return torch.from_numpy(np.ascontiguousarray(P, U64).view(np.int64)).cuda()


def raw(t):
    return t.cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def tables(kind):
    """(L, T, status) of the allocating call on ``structures()``: computed once, read by several tests, never written"""
    return evaluator(kind).toggle_scores(device_masks(structures()), return_status=True)


def raw_local(kind):
    """the local scores of ``structures()`` from the raw ABI, f64 [B, N]; None where the other public call is the reference"""
    be, P = backend(), structures()
    levels, real, rows, _ = data()
    card = np.asarray(CARD, np.uint8)
    if kind == "plain":
        return bn.run_bn(be, levels, card, P, "bic")[1]
    if kind == "rows":                     # structure b on the gathered rows of set b
        return np.concatenate([bn.run_bn(be, np.ascontiguousarray(levels[rows[b]]), card, P[b:b + 1], "bic")[1] for b in range(B)])
    if kind == "gaussian":
        return gc.run_scores(be, gc.run_moments(be, real), N, P, "bic-g")[0]
    if kind == "gaussian-rows":
        return gc.run_scores(be, gc.run_moments(be, real, rows), N, P, "bic-g", set_of=np.arange(B))[0]
    if kind == "mixed":
        lev = np.where(np.asarray(MIXED_CARD) > 0, levels, 0).astype(np.uint8)
        return mc.run_scores(be, mc.Mixed(MIXED_CARD, lev, real[:, [1, 3, 4]]), P, "bic-cg")[0]
    return None


@pytest.mark.parametrize("kind", KINDS)
def test_toggle_local_scores_are_the_scorer_bytes(kind):
    from dags_vae_search_amd import Evaluator
    ev = evaluator(kind)
    assert isinstance(ev, Evaluator) and (ev.n_vars, ev.n_samples) == (N, 32 if kind.endswith("rows") else S)
    scores, local = ev.score_masks(device_masks(structures()), local=True)
    L, T, status = tables(kind)
    assert int(status.item()) & 16 == 0 or kind == "mixed"                  # a mixed table has its illegal cells
    assert raw(L) == raw(local) and tuple(T.shape) == (B, N, N) and not bool(L.isnan().any())
    want = raw_local(kind)
    if want is not None:
        assert want.tobytes() == raw(local), kind
    assert raw(scores) == raw(ev.score_masks(device_masks(structures())))


@pytest.mark.parametrize("kind", KINDS)
def test_out_and_worklist_passes(kind):
    import torch
    ev = evaluator(kind)
    L0, T0, _ = tables(kind)
    P = structures()
    L = torch.full_like(L0, -7.0)
    T = torch.full_like(T0, -7.0)
    got = ev.toggle_scores(device_masks(P), out=(L, T))
    assert got[0] is L and got[1] is T and raw(L) == raw(L0) and raw(T) == raw(T0)
    P[1, 3] |= U64(1 << 0)                                   # structure 1: 0 -> 3 joins 1 -> 3
    fresh_L, fresh_T = ev.toggle_scores(device_masks(P))
    worklist = torch.tensor([-1, -1, 3, -1, -1, -1], dtype=torch.int32).cuda()
    ev.toggle_scores(device_masks(P), worklist=worklist, out=(L, T))
    assert raw(fresh_L[1, 3]) != raw(L0[1, 3]) and raw(T[1, 3]) == raw(fresh_T[1, 3]) != raw(T0[1, 3])
    keep = torch.ones(B, N, dtype=torch.bool).cuda()         # the pass writes the named row of T; L is the climb's to update
    keep[1, 3] = False
    assert raw(L[keep]) == raw(L0[keep]) and raw(T[keep]) == raw(T0[keep])
    with pytest.raises(ValueError) as e:
        ev.toggle_scores(device_masks(P), worklist=worklist)
    assert str(e.value) == "an incremental pass (worklist=) updates a table in place: pass out=(L, T)"
    with pytest.raises(AssertionError) as e:
        ev.toggle_scores(device_masks(P[:, :4]))
    assert str(e.value) == "Expected 5 variables, but got 4"


@pytest.mark.parametrize("kind", KINDS)
def test_used_is_the_available_case_view_s(kind):
    import torch
    ev = evaluator(kind)
    P = device_masks(structures())
    scratch = torch.empty(B, N, dtype=torch.float64).cuda()
    out, status = torch.empty(B, dtype=torch.float64).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    used = torch.full((B, N), -7, dtype=torch.int32).cuda()
    if kind != "available":
        with pytest.raises(ValueError) as e:
            ev.launch_scores(P, scratch, out, status, used=used)
        assert str(e.value) == USED_REFUSAL and bool((used == -7).all())
        return
    ev.launch_scores(P, scratch, out, status, used=used)
    observed = data()[3]
    family = structures() | (U64(1) << np.arange(N, dtype=U64))[None, :]
    want = ((observed[None, None, :] & family[:, :, None]) == family[:, :, None]).sum(2)
    assert used.cpu().numpy().tolist() == want.tolist() == ev.used(P).cpu().numpy().tolist() and want.min() < S
    assert raw(scratch) == raw(tables(kind)[0]) and int(status.item()) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_compact_parent_masks(kind):
    import torch
    from dags_vae_search_amd import CompactBatch
    ev = evaluator(kind)
    labels = np.array([[0, 1, 2, 3, 4], [4, 2, 0, 3, 1]], np.uint8)
    preds = np.array([[0, 1, 1, 2, 14], [0, 0, 3, 4, 9]], np.int16)
    want = np.zeros((2, N), U64)
    for b in range(2):
        for v in range(N):
            for u in range(N):
                if (int(preds[b, v]) >> u) & 1:
                    want[b, labels[b, v]] |= U64(1 << int(labels[b, u]))
    batch = CompactBatch(torch.from_numpy(labels).cuda(), torch.from_numpy(preds).cuda())
    got = ev.compact_parent_masks(batch)
    assert got.dtype == torch.int64 and got.is_cuda and got.cpu().numpy().view(U64).tolist() == want.tolist()
    if hasattr(ev, "base"):
        assert torch.equal(got, ev.base.compact_parent_masks(batch))
    labels[1, 4] = 2                                         # label 2 twice, label 1 missing
    with pytest.raises(AssertionError) as e:
        ev.compact_parent_masks(CompactBatch(torch.from_numpy(labels).cuda(), torch.from_numpy(preds).cuda()))
    assert str(e.value) == "Expected graph labels from 0 to 4"


@pytest.mark.parametrize("kind", KINDS)
def test_a_refused_family_raises_the_kind_s_text(kind):
    import torch
    from dags_vae_search_amd import GaussianEvaluator
    from dags_vae_search_amd import _lib as dl
    ev, P, v = evaluator(kind), structures(), 0
    if kind.startswith("gaussian"):                          # a duplicated column (no family of ``structures()`` holds 0 and 4)
        real, rows, v = data()[1].copy(), data()[2], 1
        real[:, 0] = real[:, 4]
        ev = GaussianEvaluator("tiny", "bic-g", data=real)
        ev = ev if kind == "gaussian" else ev.with_rows(torch.from_numpy(rows))
        P[2, 1] = (1 << 0) | (1 << 4)
        want = (f"a family was refused: a Cholesky pivot within rounding of zero (a duplicated or collinear column), more than "
                f"{dl.GBN_MAX_PARENTS} parents, a parent bit >= 5, or fewer than p + 2 rows for a likelihood score")
    elif kind == "mixed":                                    # a continuous parent of a factor
        P[2, 0] = 1 << 1
        want = None
    else:                                                    # a parent bit >= n_vars
        P[2, 0] = 1 << N
        want = DISCRETE_REFUSAL
    with pytest.raises(ValueError) as e:
        ev.score_masks(device_masks(P))
    if want is None:
        assert str(e.value).startswith("refused families (structure, variable): [[2, 0]]: a continuous parent of a discrete variable, "
                                       f"more than {dl.CG_MAX_CONFIGS} configurations of the discrete parents, ")
        assert str(e.value).endswith("or a discrete family the counting paths cannot hold")
    else:
        assert str(e.value) == want
    L, _, status = ev.toggle_scores(device_masks(P), return_status=True)
    assert int(status.item()) & 16 and bool(L[2, v].isnan()) and int(L.isnan().sum()) == 1


@pytest.mark.parametrize("kind", KINDS)
def test_score_masks_from_another_thread_on_the_evaluator_s_device(kind):
    """one device here: the thread's current device is the evaluator's, which exercises the guard and nothing more"""
    import torch
    ev, P = evaluator(kind), device_masks(structures())
    want = raw(ev.score_masks(P))
    got = []

    def work():
        got.append(ev.score_masks(P))
        torch.cuda.synchronize()

    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert len(got) == 1 and raw(got[0]) == want
