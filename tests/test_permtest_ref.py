"""CPU only: the numpy restatement of the permutation CI tests (tests/permtest_corpus.py) against enumeration in exact
rationals, the fifth header's binding, and that the corpus holds the shapes it names."""
import pytest

from tests import permtest_corpus as pt


@pytest.mark.parametrize("typ", ["mc-mi", "mc-x2"])
@pytest.mark.parametrize("name", sorted(pt.EXACT_CASES))
def test_restatement_agrees_with_exact_enumeration(name, typ):
    pt.check_restatement_against_enumeration(name, typ)


def test_exact_p_of_the_extreme_table_is_its_own_probability():
    from fractions import Fraction
    p, _, _ = pt.exact_law(pt.exact_case("3x3 extreme"), True)
    assert p == Fraction(6 * 24 ** 6, 479001600 * 24 ** 3)      # the six diagonal arrangements of 12! / (4! 4! 4!) tables


def test_draws_are_unbiased_by_construction():
    """multiply-shift with rejection: over all 2^16 words of a 16-bit model of the draw, every u gets floor(2^16 / m) words"""
    for m in (1, 3, 7, 100, 255, 40000):
        h = list(range(1 << 16))
        thr = ((1 << 16) - m) % m
        kept = [(v * m) >> 16 for v in h if (v * m) & 0xFFFF >= thr]
        assert len(kept) == ((1 << 16) // m) * m and all(kept.count(u) == (1 << 16) // m for u in {0, m // 2, m - 1})


def test_corpus_shapes():
    pt.check_shapes_covered()
    assert {S for S, _ in pt.SHAPES} == {1, 37, 256, 257, 300} and {B for _, B in pt.SHAPES} == {1, 255, 256, 257, 600}


def test_fifth_header_binding():
    from dags_vae_search_amd import _lib as dl
    assert list(dl.PERM_SIGNATURES) == ["dvs_ci_perm_workspace_bytes", "dvs_ci_perm_tests"]
    assert not set(dl.PERM_SIGNATURES) & (set(dl.SIGNATURES) | set(dl.EXT_SIGNATURES) | set(dl.INC_SIGNATURES)
                                          | set(dl.AVAIL_SIGNATURES) | set(dl.LOCAL_SIGNATURES))
    assert len(dl.SIGNATURES) == 64 and dl.ABI_VERSION == 202
    assert dl.signature("dvs_ci_perm_tests") is dl.PERM_SIGNATURES["dvs_ci_perm_tests"]
    assert dl.CI_PERM_TYPES == {t: i for i, t in enumerate(pt.TYPES)} == pt.TYPE_ID
    with open(dl.PERM_HEADER) as f:
        text = f.read()
    for t, i in dl.CI_PERM_TYPES.items():
        assert f"DVS_CI_{t.upper().replace('-', '_')} = {i}" in text
    with pytest.raises(KeyError, match="dvs_permtest.h") as e:
        dl.signature("dvs_nothing")
    for header in ("dvs.h", "dvs_eliminate.h", "dvs_incomplete.h", "dvs_available.h", "dvs_local.h"):
        assert header in str(e.value)
