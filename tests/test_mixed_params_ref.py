"""A fitted conditional Gaussian network (include/dvs_mixed_params.h) on the CPU: the binding of the tenth companion header, and
the restatement of tests/mixed_params_corpus.py against its exact references: mpmath for the log-likelihood, the conditioned
Gaussian joint for mode 1, the brute-force posterior for mode 2 (a class with 40 real children, whose linear-domain product is 0
in fp64, among the cases) and the sampler's moments per configuration."""
import pytest

from dags_vae_search_amd import _lib as dl
from tests import mixed_params_corpus as mc

NAMES = ["dvs_cgbn_sample_workspace_bytes", "dvs_cgbn_sample", "dvs_cgbn_loglik_workspace_bytes", "dvs_cgbn_loglik",
         "dvs_cgbn_predict_workspace_bytes", "dvs_cgbn_predict"]
NET = ["n_vars", "n_cont", "n_rows", "n_cells", "card", "parents", "offset", "coef", "intercept", "sd", "packed"]


def test_the_tenth_header_binds_six_entry_points():
    assert list(dl.MPAR_SIGNATURES) == NAMES
    args = lambda fn: [a for a, _ in dl.MPAR_SIGNATURES[fn][1]]
    assert args("dvs_cgbn_sample_workspace_bytes") == ["n_vars"]
    assert args("dvs_cgbn_sample") == NET + ["seed", "row_offset", "workspace", "workspace_bytes", "x_out", "status", "stream"]
    assert args("dvs_cgbn_loglik_workspace_bytes") == ["n_vars", "n_rows", "n_cells"]
    assert args("dvs_cgbn_loglik") == NET + ["x", "per_row", "out", "workspace", "workspace_bytes", "status", "stream"]
    assert args("dvs_cgbn_predict_workspace_bytes") == ["n_vars", "n_cells"]
    assert args("dvs_cgbn_predict") == NET + ["x", "target", "mode", "prior", "pred", "var", "posterior", "workspace", "workspace_bytes",
                                             "status", "stream"]
    assert dl.CGBN_PREDICT_MODES == {"parents": 0, "exact": 1, "class": 2}
    for fn in NAMES:
        assert dl.signature(fn) is dl.MPAR_SIGNATURES[fn]


def test_the_other_tables_are_unchanged_and_disjoint():
    others = {"SIGNATURES": 64, "EXT_SIGNATURES": 1, "INC_SIGNATURES": 5, "AVAIL_SIGNATURES": 2, "LOCAL_SIGNATURES": 2,
              "PERM_SIGNATURES": 2, "GAUSS_SIGNATURES": 5, "GCI_SIGNATURES": 2, "GPAR_SIGNATURES": 6, "MIXED_SIGNATURES": 8}
    for name, length in others.items():
        table = getattr(dl, name)
        assert not set(table) & set(dl.MPAR_SIGNATURES), name
        assert len(table) == length, (name, len(table))
    assert dl.ABI_VERSION == 202
    with pytest.raises(KeyError) as err:
        dl.signature("dvs_cgbn_joint")
    for header in ("dvs.h", "dvs_eliminate.h", "dvs_incomplete.h", "dvs_available.h", "dvs_local.h", "dvs_permtest.h", "dvs_gaussian.h",
                   "dvs_gaussian_ci.h", "dvs_gaussian_params.h", "dvs_mixed.h", "dvs_mixed_params.h"):
        assert "include/" + header in str(err.value), header


@pytest.mark.parametrize("key", ("small", "mid", "wide"))
def test_restated_loglik_against_mpmath(key):
    print(f"{key}: worst error / bound {mc.ref_loglik(key):.3e}")


@pytest.mark.parametrize("key", ("small", "mid", "wide"))
def test_restated_mode_1_against_the_conditioned_joint(key):
    print(f"{key}: worst error / bound {mc.ref_predict_real(key):.3e}")


@pytest.mark.parametrize("key", ("small", "mid"))
def test_restated_mode_2_against_the_brute_force_posterior(key):
    kept, worst = mc.ref_predict_class(key)
    print(f"{key}: {kept} of 48 rows decided, worst error / bound {worst:.3e}")


def test_restated_mode_2_with_40_children_whose_product_underflows():
    net = mc.net_of("kids")
    assert sum(1 for c in net.cvars if 0 in net.pa(c)) == 40
    kept, worst = mc.ref_predict_class("kids", S=24, underflow=True)
    print(f"kids: {kept} of 24 rows decided, worst error / bound {worst:.3e}")


def test_restated_sampler_moments_per_configuration():
    assert mc.ref_sampling_statistics() == 3 + 1 + 6


def test_rules_of_the_restatement():
    net = mc.net_of("small")
    for rule, bit in mc.RULES.items():
        bad = mc.too_many_configurations() if rule == "q" else mc.malformed(net, rule)
        assert mc.net_status(bad)[0] == bit, rule
    assert mc.net_status(net)[0] == 0 and mc.net_status(net)[1] == [0, 2, 3, 1, 4]
