"""Exact posterior arc probabilities on the device (csrc/dvs_posterior.h): how sure the data are of every arc.

``boot_strength`` answers that question with one heuristic search per bootstrap replicate.  At the sizes this package works
at (asia n = 8, sachs n = 11, the synthetic n = 12 set, everything up to the n = 20 of ``exact_search``) it has an exact
answer: the posterior probability of every arc, summed over all DAGs, by the subset dynamic programme of Koivisto and Sood
(2004) with the feature step of Koivisto (2006) — O(n^2 2^n) log-domain operations on the table ``local_score_table``
builds.  With ``bde`` or ``k2`` as the score, ``exp(local score)`` is a marginal likelihood, the result is Bayesian model
averaging in the proper sense and ``log_z`` is the log marginal likelihood of the data under the structure prior.

The prior is ORDER-MODULAR, not uniform over DAGs: uniform over the n! variable orders and, apart from ``parent_prior``,
uniform over the admissible parent sets within an order.  A DAG's prior weight is therefore proportional to its number of
linear extensions (the empty graph counts n! times, a chain once).  This is the known bias of the method, kept deliberately
— as are the package's other differences from bnlearn, which has no counterpart of this function.  The definitions are those
of include/dvs.h (dvs_arc_posterior); every sum has a fixed order, so two runs give equal bytes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as dl
from .exact import _refuse_size, local_score_table
from .strength import ArcStrength


class ArcProbabilities:
    """What every result that carries ``prob`` (f64 [..., n, n], [u, v] = P(u -> v | data)) derives from it: ``ArcPosterior``
    here and ``OrderMCMCResult`` of ordermc.py share these formulas, so ``averaged_network`` and ``inclusion_threshold`` take
    either unchanged."""

    @property
    def strength(self) -> torch.Tensor:
        """f64 [..., n, n]: P(u and v are adjacent) = prob + its transpose"""
        return self.prob + self.prob.transpose(-1, -2)

    @property
    def direction(self) -> torch.Tensor:
        """f64 [..., n, n]: prob / strength, 0 where strength is 0"""
        s = self.strength
        return torch.where(s > 0, self.prob / torch.where(s > 0, s, torch.ones_like(s)), torch.zeros_like(s))

    @staticmethod
    def counts(prob: torch.Tensor, resolution) -> ArcStrength:
        """one [n, n] matrix as the counts of ``resolution`` = R imaginary networks: a = min(R, floor(R prob)) per direction,
        ``any[u, v] = a_uv + a_vu`` and ``dir2[u, v] = 2 a_uv`` (so ``any / R`` is within 2 / R of ``strength``)"""
        R = int(resolution)
        if not 1 <= R < 1 << 29:
            raise ValueError(f"to_arc_strength: resolution must be in [1, 2^29) (got {resolution!r})")
        a = torch.clamp(torch.floor(prob * float(R)), max=float(R)).to(torch.int32)
        return ArcStrength((a + a.t()).contiguous(), (2 * a).contiguous(), R)


@dataclass
class ArcPosterior(ArcProbabilities):
    prob: torch.Tensor                     # f64 [B, n, n]: [b, u, v] = P(u -> v | data)
    log_z: torch.Tensor                    # f64 [B]: log of the sum over all (order, parent sets), L[all] of include/dvs.h
    log_z_back: torch.Tensor               # f64 [B]: the same sum taken in the other order, Rb[all]
    families: Optional[torch.Tensor]       # f64 [B, 2^n, n] or None: [b, P, v] = P(the parent set of v is exactly P)
    flags: torch.Tensor                    # int32 [B]: always zero on return (a set flag raises)

    def to_arc_strength(self, b: int = 0, resolution: int = 1_000_000) -> ArcStrength:
        """table ``b`` as the counts of ``resolution`` = R imaginary networks, so that ``averaged_network`` and
        ``inclusion_threshold`` take the exact posterior unchanged: a = min(R, floor(R prob)) per direction,
        ``any[u, v] = a_uv + a_vu`` and ``dir2[u, v] = 2 a_uv`` (so ``any / R`` is within 2 / R of ``strength``)."""
        return self.counts(self.prob[b], resolution)


def _size_prior(what, parent_prior, n, dev):
    if parent_prior is None:
        return None
    if isinstance(parent_prior, str):
        if parent_prior != "koivisto":
            raise ValueError(f"{what}: parent_prior must be None, 'koivisto' or a float64 [{n}] tensor (got {parent_prior!r})")
        return torch.tensor([-math.log(math.comb(n - 1, k)) for k in range(n)], dtype=torch.float64, device=dev)
    if not torch.is_tensor(parent_prior) or parent_prior.dtype != torch.float64 or parent_prior.shape != (n,):
        raise ValueError(f"{what}: parent_prior must be None, 'koivisto' or a float64 [{n}] tensor")
    if not bool(torch.isfinite(parent_prior).all()):
        raise ValueError(f"{what}: parent_prior must be finite")
    return parent_prior.to(dev).contiguous()


def arc_posterior_from_tables(tables: torch.Tensor, *, max_parents: Optional[int] = None, forbidden=None, parent_prior=None,
                              families: bool = False, lib=None) -> ArcPosterior:
    """``tables``, ``max_parents`` and ``forbidden`` are those of ``exact_from_tables``: f64 [B, 2^n, n] on the device, B
    independent tables in one call.  ``parent_prior``: None (all zeros), ``"koivisto"`` (``-log C(n - 1, k)`` for a parent
    set of size k: every size equally likely a priori) or a float64 [n] tensor added to the cells by parent-set size.
    ``families=True`` also returns the posterior of every (parent set, variable), as large as the tables.  A table with no
    admissible DAG raises ``ValueError`` naming the rows.  The prior over DAGs is order-modular (see the module docstring)."""
    what = "arc_posterior_from_tables"
    if not torch.is_tensor(tables):
        raise TypeError(f"{what}: tables must be a torch tensor")
    dl.need_cuda(what, tables.device)
    if tables.dtype != torch.float64 or tables.ndim != 3 or tables.shape[0] < 1 or tables.shape[2] < 1:
        raise ValueError(f"{what}: tables must be float64 [B >= 1, 2^n, n]")
    B, rows, n = tables.shape
    _refuse_size(what, n, B)
    if rows != 1 << n:
        raise ValueError(f"{what}: tables must be float64 [B, 2^n, n] (got {rows} rows for n = {n})")
    lib = dl.load() if lib is None else lib
    tables = tables.contiguous()
    dev = tables.device
    with torch.cuda.device(dev):
        forb = dl.forbidden_rows(forbidden, n, dev)
        prior = _size_prior(what, parent_prior, n, dev)
        ws_bytes = dl.workspace_bytes(lib, "dvs_arc_posterior_workspace_bytes", B, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        prob = torch.empty(B, n, n, dtype=torch.float64, device=dev)
        log_z = torch.empty(B, 2, dtype=torch.float64, device=dev)
        fam = torch.empty(B, rows, n, dtype=torch.float64, device=dev) if families else None
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        p = dl.ptr
        dl.check(lib, lib.dvs_arc_posterior(B, n, p(tables), dl.nbytes(tables), 0 if max_parents is None else int(max_parents),
                                            p(forb), p(prior), p(ws), ws_bytes, p(prob), p(log_z), p(fam),
                                            0 if fam is None else dl.nbytes(fam), p(flags), dl.stream()), "dvs_arc_posterior")
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            raise ValueError(f"{what}: no admissible DAG (a variable's empty parent set is not available): rows "
                             f"{[int(b) for b in bad.cpu()]}")
    return ArcPosterior(prob, log_z[:, 0].contiguous(), log_z[:, 1].contiguous(), fam, flags)


def arc_posterior(evaluator, *, max_parents: Optional[int] = None, forbidden=None, parent_prior=None,
                  families: bool = False) -> ArcPosterior:
    """The exact arc posterior for the evaluator's score and data (B = 1): ``local_score_table`` then
    ``arc_posterior_from_tables``.  Use a marginal-likelihood score (``bde``, ``k2``) for Bayesian model averaging; with a
    penalised likelihood (``bic``) the result is the same sum over exp(score), an approximation of it."""
    dl.need_unmixed("arc_posterior", evaluator)
    table = local_score_table(evaluator, max_parents=max_parents)
    return arc_posterior_from_tables(table[None], max_parents=max_parents, forbidden=forbidden, parent_prior=parent_prior,
                                     families=families, lib=evaluator.lib)
