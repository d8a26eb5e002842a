"""Host side of the latent-space search (no GPU): the EI closed form, the structure key / dedup of the driver, the
posterior algebra of fit_posterior (torch.linalg plumbing, run here on the CPU device), and the C ABI of dvs_gp_acquire."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from scipy.stats import norm

from dags_vae_search_amd import _lib as dl

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ei_closed_form_matches_scipy_and_its_sigma_to_zero_limit():
    from dags_vae_search_amd.predictor import expected_improvement_host
    rng = np.random.default_rng(3)
    mean = rng.normal(-100.0, 30.0, 2000)
    std = np.exp(rng.uniform(-6.0, 4.0, 2000))
    best, xi = -95.0, 0.5
    imp = mean - best - xi
    ref = imp * norm.cdf(imp / std) + std * norm.pdf(imp / std)
    got = expected_improvement_host(mean, std, best, xi)
    assert np.abs(got - ref).max() <= 1e-12 * (1.0 + np.abs(ref).max())
    assert (got >= 0.0).all()
    # sigma -> 0: EI -> max(imp, 0); below the floor the limit itself is returned
    for m in (-3.0, -1e-3, 0.0, 2.5):
        limit = max(m - 0.0, 0.0)
        for s in (1e-3, 1e-6, 1e-9):
            assert abs(float(expected_improvement_host([m], [s], 0.0)[0]) - limit) <= 0.5 * s
        assert float(expected_improvement_host([m], [0.0], 0.0, floor=1e-12)[0]) == limit
        assert float(expected_improvement_host([m], [1e-13], 0.0, floor=1e-12)[0]) == limit


def test_structure_key_and_dedup_of_the_driver():
    from dags_vae_search_amd import LabeledDag, LabeledGraph
    from dags_vae_search_amd.search import is_search_valid, new_structures, structure_key
    a = LabeledGraph([0, 1, 2, 3], [(0, 1), (1, 2), (0, 3)])
    a_reordered = LabeledGraph([0, 1, 2, 3], [(0, 3), (1, 2), (0, 1)])
    # the same network with its vertices listed in another order (vertex i of b carries label [2, 0, 1, 3][i])
    b_perm = LabeledGraph([2, 0, 1, 3], [(1, 2), (2, 0), (1, 3)])
    other = LabeledGraph([0, 1, 2, 3], [(0, 1), (1, 2), (1, 3)])
    reversed_edge = LabeledGraph([0, 1, 2, 3], [(1, 0), (1, 2), (0, 3)])
    assert structure_key(a) == structure_key(a_reordered) == structure_key(b_perm)
    assert structure_key(a) != structure_key(other)
    assert structure_key(a) != structure_key(reversed_edge)
    dag = LabeledDag(4, 4)
    cyclic = LabeledGraph([0, 1, 2, 3], [(0, 1), (1, 2), (2, 0)])
    repeated_label = LabeledGraph([0, 1, 1, 3], [(0, 1)])            # a DAG with labels in range, but not a permutation
    assert dag.is_valid_graph(repeated_label) and not is_search_valid(repeated_label, dag)
    assert not is_search_valid(cyclic, dag) and not is_search_valid(None, dag)
    assert not is_search_valid(LabeledGraph([0, 1, 2], []), dag)
    seen = {structure_key(other)}
    draws = [a, None, a_reordered, cyclic, other, repeated_label, b_perm, reversed_edge]
    new, n_valid = new_structures(draws, dag, seen)
    assert n_valid == 5                                               # a, a_reordered, other, b_perm, reversed_edge
    assert new == [a, reversed_edge]                                  # first occurrence kept, known structures dropped
    assert structure_key(a) in seen and structure_key(reversed_edge) in seen


def _rbf(a, b, o, l):
    return o * torch.exp(-0.5 * torch.cdist(a, b, compute_mode="donot_use_mm_for_euclid_dist").pow(2) / l ** 2)


def test_fit_posterior_algebra_against_the_textbook_forms():
    """fit_posterior's matrices (torch.linalg plumbing, device-agnostic) on a small well-conditioned problem: SoR P is
    s^2 (s^2 K_uu + K_uf K_fu)^-1, DTC P is that minus K_uu^-1 with c0 = o, alpha is fit()'s, and set_train_data drops
    both caches.  (The kernel that evaluates them runs only on the GPU: tests/test_gpu_search.py.)"""
    from dags_vae_search_amd.predictor import GPRegressionModel
    g = torch.Generator().manual_seed(5)
    X = torch.randn(80, 6, generator=g, dtype=torch.float64)
    y = torch.randn(80, generator=g, dtype=torch.float64) * 3.0 - 7.0
    gp = GPRegressionModel(X, y, device="cpu")
    gp.inducing_points = X[:20].float().contiguous()
    gp.noise, gp.outputscale, gp.lengthscale, gp.constant = 0.3, 1.7, 1.9, -6.0
    gp.fit_posterior(jitter=1e-6)
    Z = gp.inducing_points.double()
    Kuu = _rbf(Z, Z, 1.7, 1.9) + 1e-6 * torch.eye(20, dtype=torch.float64)
    Kuf = _rbf(Z, X, 1.7, 1.9)
    s2 = 0.3
    sigma = s2 * torch.linalg.inv(s2 * Kuu + Kuf @ Kuf.T)
    alpha = sigma @ Kuf @ (y + 6.0) / s2
    W, c0 = gp._post["sor"]
    assert W.shape == (20, 21) and c0 == 0.0
    assert torch.allclose(W[:, :20], sigma, rtol=1e-9, atol=1e-12) and torch.equal(W[:, :20], W[:, :20].T)
    assert torch.allclose(W[:, 20], alpha, rtol=1e-8, atol=1e-10)
    a_fit = gp._alpha.clone()
    assert torch.equal(W[:, 20], a_fit)
    Wd, c0d = gp._post["dtc"]
    assert c0d == 1.7 and torch.equal(Wd[:, 20], a_fit)
    assert torch.allclose(Wd[:, :20], sigma - torch.linalg.inv(Kuu), rtol=1e-8, atol=1e-8)
    # DTC variance at a training point equals o - Q_** + k^T Sigma k (textbook form), and is >= the SoR one
    k = _rbf(X[30:31], Z, 1.7, 1.9)[0]
    v_dtc = 1.7 + k @ Wd[:, :20] @ k
    assert float(v_dtc) == pytest.approx(float(1.7 - k @ torch.linalg.solve(Kuu, k) + k @ sigma @ k), rel=1e-9)
    assert float(v_dtc) >= float(k @ W[:, :20] @ k)
    # alpha and P come from the same jitter: an alpha fitted with another jitter is refitted
    gp.fit(jitter=1e-3)
    gp.fit_posterior(jitter=1e-6)
    assert torch.equal(gp._post["sor"][0][:, 20], a_fit) and torch.equal(gp._alpha, a_fit)
    gp.set_train_data(X[:50], y[:50])
    assert gp._alpha is None and gp._post is None and gp.train_x.shape == (50, 6)
    with pytest.raises(AssertionError):
        gp.set_train_data(X[:50, :5], y[:50])
    with pytest.raises(RuntimeError):                                  # no CPU path for the acquisition itself
        gp.expected_improvement(X[:4].float(), 0.0)


def test_dvs_gp_acquire_is_declared_exported_and_checks_its_arguments():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "dvs.h")).read(), flags=re.S)
    assert re.search(r"\bint dvs_gp_acquire\s*\(", txt)
    assert "dvs_gp_acquire" in dl.EXPORTS
    lib = dl.load()
    assert hasattr(ctypes.CDLL(dl.lib_path()), "dvs_gp_acquire")
    assert lib.dvs_version() == 202
    buf = ctypes.create_string_buffer(64)                # never dereferenced: every call below fails its checks first
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(Q=4, M=8, D=4, ld=9, o=1.0, l=1.0, c0=0.0, x=p, z=p, w=p, mean=p):
        return lib.dvs_gp_acquire(Q, M, D, ld, x, z, w, c0, o, l, 0.0, 0.0, 0.0, mean, p, p, None, None)
    assert call(D=33) == 2 and b"dim <= 32" in lib.dvs_last_error()
    assert call(Q=0) == 2 and call(M=0) == 2
    assert call(M=dl.GP_ACQ_MAX_INDUCING + 1, ld=2000) == 2 and b"1023" in lib.dvs_last_error()
    assert call(ld=8) == 12
    assert call(c0=-1.0) == 12 and call(c0=math.nan) == 12
    assert call(l=0.0) == 5 and call(o=-1.0) == 5
    assert call(x=None) == 10 and call(w=None) == 10 and call(mean=None) == 10
