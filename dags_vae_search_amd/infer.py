"""Inference on a fitted discrete Bayesian network on the device (csrc/dvs_infer.h): bnlearn's ``cpquery``,
``cpdist`` and ``predict`` next to ``bn_fit`` / ``sample`` / ``log_likelihood`` of params.py.

``cpquery`` estimates P(event | evidence) by likelihood weighting, ``cpdist`` returns the weighted particles themselves,
``posterior`` the normalised marginals of chosen variables, and ``predict`` one variable from all the others: from its parents
alone, by the exact posterior over its Markov blanket, or by likelihood weighting (bnlearn's "parents" and "bayes-lw"; "exact"
is what "bayes-lw" with every other variable observed approximates).  ``cross_validate(loss="pred" | "pred-exact" | "pred-lw")``
of params.py composes ``bn_fit`` and ``predict`` into a classification loss.

Variables and levels are indices, as everywhere in this package.  Evidence is either a dict {variable: level} (one query) or a
pair (rows, observed): packed int64 rows [Q, ceil(n / 16)] on the device and an int mask (shared) or int64 tensor [Q] of
masks, bit v set <=> variable v of that query is clamped to its level in the row.

The definitions are those of include/dvs.h (dvs_bn_lw, dvs_bn_blanket_posterior).  Parity with bnlearn rests on them and is
not pinned against an R run; in particular ties in ``predict`` go to the lowest level where bnlearn breaks them at random.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib as dl
from .bic import BNLearnWrapper
from .params import FittedBN

PREDICT_METHODS = ("parents", "exact", "bayes-lw")


def _mask_of(variables, n, what):
    mask = 0
    for v in variables:
        if not 0 <= int(v) < n:
            raise ValueError(f"{what}: variable {v} is not in [0, {n})")
        mask |= 1 << int(v)
    return mask


def _event_words(fitted: FittedBN, event, what):
    """{variable: level or levels} -> uint16 [n] on the device (bit k <=> level k allowed), or None for no event"""
    if event is None:
        return None
    n = fitted.n_vars
    words = np.full(n, 0xFFFF, np.uint16)
    for v, levels in dict(event).items():
        levels = [levels] if np.isscalar(levels) else list(levels)
        if not 0 <= int(v) < n or not levels or any(not 0 <= int(k) < fitted.card_host[int(v)] for k in levels):
            raise ValueError(f"{what}: event names variable {v} with levels {levels}; levels must be in [0, card)")
        words[int(v)] = sum({1 << int(k) for k in levels})
    return torch.from_numpy(words.view(np.int16)).to(fitted.device)


def _evidence(fitted: FittedBN, evidence, what):
    """-> (rows int64 [Q, words] on the device, observed int64 [Q] on the device)"""
    n, dev = fitted.n_vars, fitted.device
    words = (n + 15) // 16
    if isinstance(evidence, dict):
        row = [0] * words
        for v, k in evidence.items():
            if not 0 <= int(v) < n or not 0 <= int(k) < 16:
                raise ValueError(f"{what}: evidence names variable {v} with level {k}")
            row[int(v) // 16] |= int(k) << (4 * (int(v) % 16))
        rows = torch.from_numpy(np.array([row], np.uint64).view(np.int64)).to(dev)
        return rows, torch.tensor([_mask_of(evidence, n, what)], dtype=torch.int64, device=dev)
    rows, observed = evidence
    if isinstance(rows, BNLearnWrapper):
        rows = rows.packed
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.ndim != 2 or rows.shape[1] != words or rows.shape[0] < 1:
        raise ValueError(f"{what}: evidence rows must be packed int64 [Q >= 1, {words}]")
    dl.need_cuda(what, rows.device)
    if torch.is_tensor(observed):
        if observed.dtype != torch.int64 or observed.shape != (rows.shape[0],):
            raise ValueError(f"{what}: observed must be an int or an int64 tensor [{rows.shape[0]}]")
        observed = observed.to(dev).contiguous()
    else:
        if int(observed) >> n:
            raise ValueError(f"{what}: observed has a bit at or above n_vars = {n}")
        observed = torch.full((rows.shape[0],), int(observed), dtype=torch.int64, device=dev)
    return rows.contiguous(), observed


def _lw(fitted: FittedBN, rows, observed, *, n_particles, seed, index=0, event=None, targets=0, particles=False,
        query_offset=0, what="likelihood weighting"):
    """one dvs_bn_lw -> (sums f64 [Q, 3], marginals f64 [Q, T, 16] or None, particles int64 [Q, M, words] or None, weights f64
    [Q, M] or None); the refusals of the status word raise ValueError"""
    dl.need_cuda(what, fitted.device)
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"{what}: index must be in [0, {fitted.batch})")
    if int(n_particles) < 1 or int(query_offset) < 0:
        raise ValueError(f"{what}: n must be >= 1 and query_offset >= 0")
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    Q, M, T = rows.shape[0], int(n_particles), bin(targets).count("1")
    lo, hi = fitted.offsets_host[index * n], fitted.offsets_host[(index + 1) * n]
    with torch.cuda.device(dev):
        ws_bytes = dl.workspace_bytes(lib, "dvs_bn_lw_workspace_bytes", hi - lo, n, Q, M, targets)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        sums = torch.empty(Q, 3, dtype=torch.float64, device=dev)
        marg = torch.empty(Q, T, 16, dtype=torch.float64, device=dev) if T else None
        parts = torch.empty(Q, M, rows.shape[1], dtype=torch.int64, device=dev) if particles else None
        wts = torch.empty(Q, M, dtype=torch.float64, device=dev) if particles else None
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_lw(n, Q, M, p(fitted.card), p(fitted.parents[index]), p(fitted.offsets[index * n:]),
                                    p(fitted.cpt), hi - lo, p(rows), p(observed), p(event), targets,
                                    dl.seed64(seed), int(query_offset), p(ws), ws_bytes, p(sums), p(marg),
                                    p(parts), p(wts), p(status), dl.stream()), "dvs_bn_lw")
        st = int(status.item())
    dl.check_network_status(what, st)
    if st & dl.STATUS_REFUSED:
        raise ValueError(f"{what}: an evidence level is at or above its variable's level count, or the tables do not match the structure")
    return sums, marg, parts, wts


def cpquery(fitted: FittedBN, event, evidence, *, n: int = 10000, seed: int, index: int = 0, query_offset: int = 0) -> torch.Tensor:
    """bnlearn's ``cpquery(method = "lw")``: P(event | evidence) under structure ``index`` of ``fitted`` from ``n`` weighted
    particles per query -> float64 [Q] on the device, sum w [event] / sum w, NaN where the evidence has probability zero under
    every particle (sum w = 0).  ``event``: {variable: level or list of levels}, a conjunction of level sets.  Query q is a
    function of (seed, query_offset + q), so a batch may be cut into calls with consecutive ``query_offset``."""
    what = "cpquery"
    rows, observed = _evidence(fitted, evidence, what)
    if not event:
        raise ValueError(f"{what}: event must name at least one variable")
    sums, _, _, _ = _lw(fitted, rows, observed, n_particles=n, seed=seed, index=index, event=_event_words(fitted, event, what),
                        query_offset=query_offset, what=what)
    return sums[:, 2] / sums[:, 0]


def cpdist(fitted: FittedBN, nodes, evidence, *, n: int, seed: int, index: int = 0, query_offset: int = 0):
    """bnlearn's ``cpdist(method = "lw")``: ``n`` weighted particles per query -> (particles packed int64 [Q, n, ceil(n_vars /
    16)] with the levels of ``nodes`` (every other nibble zero), weights float64 [Q, n], effective sample size float64 [Q] =
    (sum w)^2 / sum w^2, NaN where sum w = 0), all on the device."""
    what = "cpdist"
    rows, observed = _evidence(fitted, evidence, what)
    keep = _mask_of(nodes, fitted.n_vars, what)
    sums, _, parts, wts = _lw(fitted, rows, observed, n_particles=n, seed=seed, index=index, particles=True,
                              query_offset=query_offset, what=what)
    nib = [sum(15 << (4 * (v % 16)) for v in range(fitted.n_vars) if v // 16 == w and (keep >> v) & 1) for w in range(parts.shape[2])]
    parts &= torch.from_numpy(np.array(nib, np.uint64).view(np.int64)).to(parts.device)
    return parts, wts, sums[:, 0] * sums[:, 0] / sums[:, 1]


def posterior(fitted: FittedBN, targets, evidence, *, n: int = 10000, seed: int, index: int = 0, query_offset: int = 0) -> torch.Tensor:
    """The marginal posteriors of ``targets`` (variables, reported in ascending index) given the evidence, by likelihood
    weighting -> float64 [Q, len(targets), 16] on the device: cell k is sum w [level = k] / sum w, zero at and beyond the
    variable's level count, NaN where sum w = 0."""
    what = "posterior"
    rows, observed = _evidence(fitted, evidence, what)
    mask = _mask_of(targets, fitted.n_vars, what)
    if not mask:
        raise ValueError(f"{what}: targets must name at least one variable")
    sums, marg, _, _ = _lw(fitted, rows, observed, n_particles=n, seed=seed, index=index, targets=mask,
                           query_offset=query_offset, what=what)
    return marg / sums[:, 0, None, None]


def _blanket(fitted: FittedBN, data, target, use_children, prob, index=None, what="predict"):
    """dvs_bn_blanket_posterior for structure ``index`` (None: the whole batch) -> (pred uint8 [B, S], posterior [B, S, r] or None)"""
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    B, first = (fitted.batch, 0) if index is None else (1, int(index))
    S, r = data.shape[0], fitted.card_host[target]
    with torch.cuda.device(dev):
        post = torch.empty(B, S, r, dtype=torch.float64, device=dev) if prob else None
        pred = torch.empty(B, S, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_blanket_posterior(B, n, S, p(data), p(fitted.card), p(fitted.parents[first:]),
                                                   p(fitted.offsets[first * n:]), p(fitted.cpt), fitted.cpt.numel() * 8,
                                                   int(target), int(use_children), p(post), p(pred), p(status), dl.stream()),
                 "dvs_bn_blanket_posterior")
        if int(status.item()) & dl.STATUS_REFUSED:
            raise ValueError(f"{what}: a row has a level code at or above its variable's level count, or the tables do not match the structure")
    return pred, post


def predict(fitted: FittedBN, target: int, data, *, method: str = "parents", n: int = 500, seed: int = 0, prob: bool = False,
            index: int = 0, query_offset: int = 0):
    """bnlearn's ``predict`` for a discrete node: the level of variable ``target`` in every row of ``data`` (an evaluator or
    packed int64 rows [S, ceil(n_vars / 16)]; the target's own column is ignored) under structure ``index`` -> uint8 [S] on the
    device, with ``prob`` (predictions, posterior float64 [S, card[target]]).  ``method``: "parents" (the target's table row
    under its parents), "exact" (the posterior given all other variables: parents, children and their other parents) or
    "bayes-lw" (likelihood weighting with ``n`` particles per row and every other variable observed; row i is query
    ``query_offset + i``).  The lowest level wins a tie; a row whose posterior is NaN (an all-zero product, sum w = 0)
    predicts 255."""
    what = "predict"
    dl.need_cuda(what, fitted.device)
    if method not in PREDICT_METHODS:
        raise ValueError(f"method must be one of {PREDICT_METHODS} (got {method!r})")
    if not 0 <= int(target) < fitted.n_vars:
        raise ValueError(f"{what}: target must be in [0, {fitted.n_vars})")
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"{what}: index must be in [0, {fitted.batch})")
    data = dl.packed_rows(what, data, fitted.n_vars)
    target = int(target)
    if method != "bayes-lw":
        pred, post = _blanket(fitted, data, target, method == "exact", prob, index, what)
        return (pred[0], post[0]) if prob else pred[0]
    r = fitted.card_host[target]
    observed = torch.full((data.shape[0],), ((1 << fitted.n_vars) - 1) & ~(1 << target), dtype=torch.int64, device=fitted.device)
    sums, marg, _, _ = _lw(fitted, data, observed, n_particles=n, seed=seed, index=index, targets=1 << target,
                           query_offset=query_offset, what=what)
    post = marg[:, 0, :r] / sums[:, 0, None]
    levels = torch.arange(r, device=post.device).expand_as(post)
    first = torch.where(post == post.max(1, keepdim=True).values, levels, 255).min(1).values      # the lowest of the maxima
    pred = torch.where(sums[:, 0] > 0, first, 255).to(torch.uint8)
    return (pred, post) if prob else pred
