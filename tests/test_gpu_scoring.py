"""GPU: the fp64 scoring kernels (csrc/k_bic.hip) and the clip + Adam norm (csrc/k_optim.hip) over the whole range
include/dvs.h promises, through the raw C ABI and BNLearnWrapper.score_masks.  Cases, references, tolerances and the check
functions are those of tests/scoring_corpus.py, shared with the emulator twin tests/test_emu_scoring.py.  Every case is
deterministic; the refusal cases are handled paths that come back through `status`.  Cases are built on first use."""
import math

import numpy as np
import pytest

from tests import scoring_corpus as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from dags_vae_search_amd import _lib as dl
    return sc.GpuBackend(dl.load())


@pytest.mark.parametrize("name", sc.BIC_CASE_NAMES)
def test_bic_case(be, name):
    """dvs_bic_scores: per-variable local scores and per-DAG sums within 1e-12 * T of the fsum reference; refused cells NaN
    with status 16 and every other cell intact; bitwise-equal pairs; exact zeros; two calls give equal bytes.  Measured on
    an MI355X: worst |got - ref| / T over all cases 3.7e-16 — the device's fp64 log needs no allowance beyond the bound."""
    worst = sc.check_bic_case(be, sc.bic_case(name), twice=True)
    print(f"\nBIC {name}: worst |got - ref| / T = {worst:.3g} (asserted <= {sc.BIC_RTOL:g})")


@pytest.mark.parametrize("name", sc.BIC_CASE_NAMES)
def test_bic_case_through_the_wrapper(name):
    """BNLearnWrapper.score_masks on the same data and masks.  The wrapper takes its level counts from the data
    (data.max(0) + 1), so the expectation is rebuilt with those: ValueError where a cell is refused — which must be exactly
    the corpus' refusal cases — else the per-DAG sums."""
    import torch
    from dags_vae_search_amd import BNLearnWrapper
    case = sc.bic_case(name)
    card = (case.data.max(0) + 1).astype(np.uint8)
    if np.array_equal(card, case.card):
        mine = case
    else:
        probe = case._replace(card=card, refused=frozenset())
        B, n = case.masks.shape
        refused = {(b, v) for b in range(B) for v in range(n) if sc.expected_path(probe, b, v) == "refused"}
        mine = sc._case(name + "@data-levels", case.data, card, case.masks, status=16 if refused else 0, refused=refused)
    assert bool(mine.refused) == (name in sc.REFUSAL_CASE_NAMES)        # a lost level must not turn a refusal into a score
    ev = BNLearnWrapper(name, "bic", data=case.data)
    masks = torch.from_numpy(mine.masks.view(np.int64).copy())
    if mine.refused:
        with pytest.raises(ValueError):
            ev.score_masks(masks)
        return
    loc, tol = sc.bic_reference(mine)
    got = ev.score_masks(masks).cpu().numpy()
    for b in range(len(got)):
        assert abs(got[b] - math.fsum(loc[b])) <= sc.BIC_RTOL * math.fsum(tol[b]), (name, b, got[b])


@pytest.mark.parametrize("name", sc.RELABEL_CASE_NAMES)
def test_parent_masks_compose_with_scores(be, name):
    sc.check_relabel_case(be, *sc.relabel_case(name))


@pytest.mark.parametrize("na,nb,dim", sc.GP_TRIPLES)
def test_gp_kernel(be, na, nb, dim):
    worst = sc.check_gp_kernel(be, na, nb, dim)
    print(f"\ngp_kernel {(na, nb, dim)}: worst |got - ref| / T = {worst:.3g}")


def test_gp_kernel_edges(be):
    sc.check_gp_kernel_edges(be)
    sc.check_gp_backward_refusals(be)


@pytest.mark.parametrize("na,nb,dim", sc.GP_TRIPLES)
def test_gp_kernel_backward(be, na, nb, dim):
    worst = sc.check_gp_kernel_backward(be, na, nb, dim, 0)
    if na == nb:
        worst = max(worst, sc.check_gp_kernel_backward(be, na, nb, dim, 1))
    print(f"\ngp_kernel_backward {(na, nb, dim)}: worst |got - ref| / T = {worst:.3g}")


@pytest.mark.parametrize("weights", sorted(sc.PREDICT_WEIGHTS))
@pytest.mark.parametrize("batch,m,dim", sc.GP_PREDICT_TRIPLES)
def test_gp_predict(be, batch, m, dim, weights):
    """dvs_gp_predict against the all-fp64 reference within the bound that follows from the kernel's float32 squared
    distance (scoring_corpus docstring), with +-1e6 weights that cancel ("sgpr") and with O(1) weights that resolve every
    inducing point ("resolved").  Worst |error| / bound measured on an MI355X over all triples: sgpr 0.057, resolved
    0.044: the bound was not needed in full, and nothing beyond it was found."""
    ratio = sc.check_gp_predict(be, batch, m, dim, weights)
    print(f"\ngp_predict {weights} {(batch, m, dim)}: worst error / bound = {ratio:.3g}")


@pytest.mark.parametrize("n", sc.ADAM_SIZES)
def test_clip_adam_norm_tail_and_step7_update(be, n):
    """check_clip_adam on the device.  Measured on an MI355X, worst |P - ref| / tolerance over all sizes: 0.14 (the
    library's float32 bias corrections included: they get no term of their own)."""
    worst = sc.check_clip_adam(be, n)
    print(f"\nclip_adam n={n}: worst |P - ref| / tol = {worst:.3g}")
