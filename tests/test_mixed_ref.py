"""CPU only: the references of tests/mixed_corpus.py against each other (mpmath at 60 digits per configuration against
numpy.linalg.lstsq on the raw rows, under the bound the corpus derives, with every configuration's conditioning asserted on the
way), the ninth header's binding, and that the corpus holds the shapes it names."""
import mpmath as mp
import numpy as np
import pytest

from dags_vae_search_amd import mixed  # noqa: F401  (the module under test: its absence fails every test of this file)
from dags_vae_search_amd import _lib as dl
from tests import gaussian_corpus as gc
from tests import mixed_corpus as mc


def test_ninth_header_binding():
    assert list(dl.MIXED_SIGNATURES) == ["dvs_cg_partition", "dvs_cg_moments_workspace_bytes", "dvs_cg_moments",
                                         "dvs_cg_scores_workspace_bytes", "dvs_cg_scores", "dvs_cg_toggle_workspace_bytes",
                                         "dvs_cg_toggle_scores", "dvs_cg_fit"]
    others = (dl.SIGNATURES, dl.EXT_SIGNATURES, dl.INC_SIGNATURES, dl.AVAIL_SIGNATURES, dl.LOCAL_SIGNATURES, dl.PERM_SIGNATURES,
              dl.GAUSS_SIGNATURES, dl.GCI_SIGNATURES, dl.GPAR_SIGNATURES)
    assert all(not set(dl.MIXED_SIGNATURES) & set(t) for t in others)
    assert len(dl.SIGNATURES) == 64 and dl.ABI_VERSION == 202 and len(dl.GAUSS_SIGNATURES) == 5 and len(dl.GPAR_SIGNATURES) == 6
    assert dl.signature("dvs_cg_fit") is dl.MIXED_SIGNATURES["dvs_cg_fit"]
    assert dl.CG_MAX_CONFIGS == 4096 == 16 ** 3 and dl.CGSCORE_TYPES == {"loglik-cg": 0, "aic-cg": 1, "bic-cg": 2}
    assert [k for k, _ in dl.MIXED_SIGNATURES["dvs_cg_partition"][1]] == [
        "n_vars", "n_samples", "data", "card", "n_requests", "masks", "q_pitch", "count", "count_bytes", "start", "order", "order_bytes",
        "status", "stream"]
    with pytest.raises(KeyError, match="dvs_mixed.h"):
        dl.signature("dvs_cg_predict")


def test_corpus_holds_the_shapes_it_names():
    md = mc.partition_case(257)
    assert [int(md.card[v]) for v in md.dvars] == [3, 4, 16, 2, 1, 16] and md.nc == 3
    assert sorted(len(gc.bits_of(D)) for D in mc.partition_requests(md)) == [0, 1, 1, 1, 2, 2, 3, 3]
    w = mc.wide_case()
    assert w.dvars == [15, 16, 33] and w.n == 48
    m = mc.moments_case(5)
    assert [len(s) for s in m.segments(1)] == list(mc.LEVEL_COUNTS)
    pos = [np.nonzero(m.levels[:, 0] == z)[0] for z in range(6)]
    assert all(p.max() - p.min() >= len(p) for p in pos if len(p) > 1), "the levels are interleaved"
    s = mc.score_case()
    fams = mc.score_families()
    assert sorted({(s.q(D), len(G)) for _, D, G in fams}) == [(q, p) for q in (1, 2, 12) for p in (0, 2, mc.CAP)]
    for v, D, G in fams:
        assert min(len(seg) for seg in s.segments(D)) >= 4 * (len(G) + 2)
    for n in (5, 17, 48):
        t, P = mc.toggle_case(n)
        assert t.n == n and abs(len(t.dvars) - n / 2) <= 1
        assert not (P[:, t.dvars] & np.uint64(gc.mask_of(t.cvars))).any()
    r = mc.refusal_case()
    assert r.q(gc.mask_of([1, 2, 3])) == 4096 and r.q(gc.mask_of([1, 2, 3, 4])) == 16 ** 4
    assert sorted(len(seg) for seg in r.segments(1)) == [3, 197, 200]


@gc.at60
def test_lstsq_route_against_mpmath():
    """the two references of a mixed family agree within the corpus' bound; every configuration's kappa and eta are asserted
    by Reference.local before the comparison"""
    worst = 0.0
    for v, D, G in mc.score_families():
        for typ, k in mc.VARIANTS:
            want, bound = mc.reference_local(mc.score_case, v, D, G, typ, k)
            err = float(abs(mp.mpf(mc.lstsq_local(mc.score_case, v, D, G, typ, k)) - want))
            assert err <= bound, (v, D, G, typ, err, bound)
            worst = max(worst, err / bound)
    print(f"worst lstsq error / bound {worst:.3e}")


def test_one_configuration_is_the_gaussian_reference():
    """q = 1: the mixed reference is gaussian_corpus' own on all rows"""
    md = mc.score_case()
    ref = gc.Reference(gc.ExactMoments(md.x))
    for v, D, G in mc.score_families():
        if D == 0:
            for typ, k in mc.VARIANTS:
                want, _ = mc.reference_local(mc.score_case, v, D, G, typ, k)
                theirs, _ = ref.local(md.col[v], [md.col[u] for u in G], mc.GAUSS_OF[typ], k)
                with mp.workdps(gc.DPS):
                    assert abs(want - theirs) < mp.mpf(10) ** -45
