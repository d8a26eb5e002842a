"""The fp64 scoring kernels (csrc/k_bic.hip) and the clip + Adam norm (csrc/k_optim.hip) on the host emulator over the
whole range include/dvs.h promises: every case, reference and tolerance comes from tests/scoring_corpus.py, which
tests/test_gpu_scoring.py runs unchanged on the device.  Cases are named here and built on first use."""
import pytest

from tests import scoring_corpus as sc


@pytest.fixture(scope="module")
def be():
    from tests.emu.harness import emu
    return sc.EmuBackend(emu())


def test_corpus_is_anchored_to_the_pinned_oracle_and_lists_its_refusals_in_advance():
    """The sparse reference equals oracle.bic.local_score wherever the oracle can represent the table (bic_reference asserts
    it per cell), on the real asia / sachs data as on the synthetic sets; the refused cells of a case are exactly the ones
    the documented limits refuse, in at most one DAG in four."""
    cases = [sc.bic_case(name) for name in sc.BIC_CASE_NAMES]
    for case in cases:
        loc, tol = sc.bic_reference(case)
        B, n = case.masks.shape
        want = {(b, v) for b in range(B) for v in range(n) if sc.expected_path(case, b, v) == "refused"}
        assert want == set(case.refused), case.name
        assert {(b, v) for b in range(B) for v in range(n) if loc[b, v] != loc[b, v]} == want
        assert len({b for b, _ in want}) * 4 <= B
        assert case.status == (16 if want else 0)
    paths = {sc.expected_path(c, b, v) for c in cases for b in range(len(c.masks)) for v in range(c.masks.shape[1])}
    assert paths == {"dense", "sort", "refused"}


@pytest.mark.parametrize("name", sc.BIC_CASE_NAMES)
def test_emu_bic_case(be, name):
    """dvs_bic_scores: per-variable local scores and per-DAG sums within 1e-12 * T of the fsum reference, refused cells NaN
    with status 16 and every other cell intact, bitwise-equal pairs (1-level parent, self-loop bit), exact zeros (1-level
    child); the small cases are also run twice for equal bytes."""
    sc.check_bic_case(be, sc.bic_case(name), twice=name.startswith(("batch", "keybits", "levels")))


@pytest.mark.parametrize("name", sc.RELABEL_CASE_NAMES)
def test_emu_parent_masks_compose_with_scores(be, name):
    """dvs_bic_parent_masks on u64 rows at n = 16, 17, 48 (reversed / random / identity labels), then dvs_bic_scores on its
    output against the reference on the relabelled parent sets."""
    sc.check_relabel_case(be, *sc.relabel_case(name))


@pytest.mark.parametrize("na,nb,dim", sc.GP_TRIPLES)
def test_emu_gp_kernel(be, na, nb, dim):
    sc.check_gp_kernel(be, na, nb, dim)


def test_emu_gp_kernel_edges(be):
    sc.check_gp_kernel_edges(be)
    sc.check_gp_backward_refusals(be)


@pytest.mark.parametrize("na,nb,dim", sc.GP_TRIPLES)
def test_emu_gp_kernel_backward(be, na, nb, dim):
    """dxa and row_sums within 1e-12 * (sum of absolute terms); NaN pre-fill overwritten, guard region after na * dim
    untouched, two calls equal bytes; symmetric (G' = G + G^T with a non-symmetric G) wherever na == nb."""
    sc.check_gp_kernel_backward(be, na, nb, dim, 0)
    if na == nb:
        sc.check_gp_kernel_backward(be, na, nb, dim, 1)


@pytest.mark.parametrize("weights", sorted(sc.PREDICT_WEIGHTS))
@pytest.mark.parametrize("batch,m,dim", sc.GP_PREDICT_TRIPLES)
def test_emu_gp_predict(be, batch, m, dim, weights):
    """dvs_gp_predict against the all-fp64 reference within the bound that follows from the kernel's float32 squared
    distance (scoring_corpus docstring): with alternating 1e6 weights whose sum is O(1) ("sgpr": the bound is then as large
    as the output) and with O(1) weights ("resolved": the bound is 1e-6 .. 1e-4 of the output, every inducing point counts).
    Worst |error| / bound measured on the emulator build over all triples: sgpr 0.056, resolved 0.044."""
    ratio = sc.check_gp_predict(be, batch, m, dim, weights)
    print(f"gp_predict {weights} {(batch, m, dim)}: worst error / bound = {ratio:.3g}")


@pytest.mark.parametrize("n", sc.ADAM_SIZES)
def test_emu_clip_adam_norm_tail_and_step7_update(be, n):
    """k_sqnorm_part's scalar tail (n % 4 != 0; each tail entry carries about 1 % of the sum of squares) and an Adam step in
    which the clip coefficient matters (step 7, non-zero moments, coefficient 0.1): norm, coefficient, clipped gradient,
    both moments and parameters against clip_grad_norm_ + Adam in float64; dvs_clip_adam_from_partials from hand-made
    partials; raised guards; max_norm <= 0."""
    worst = sc.check_clip_adam(be, n)
    print(f"clip_adam n={n}: worst |P - ref| / tol = {worst:.3g}")
