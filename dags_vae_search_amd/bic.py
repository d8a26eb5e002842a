"""Batched scorer for discrete Bayesian networks on the GPU: BIC and bnlearn's other decomposable scores.

Mirror of the reference's ``BNLearnWrapper`` (src/problem/bn/bnlearn.py:10-61): ``score(labeled_graph)`` returns
``bnlearn::score(net, data, type="bic")`` of the DAG whose vertex v stands for data-set variable ``labels[v]``.  The
reference starts one ``Rscript`` per graph; here ``score_batch`` scores thousands of structures in one HIP launch
(csrc/k_bic.hip: LDS contingency counts + fp64 log-likelihood).  The data set is passed in (the reference pulls it from
R's ``data(asia)``; its CSV copies are data/bn_asia/target.csv, data/bn_sachs/target.csv).

The reference hands ``metric_name`` to bnlearn unseen (bnlearn_scripts/bnlearn_score.R); built here are ``bic`` (the
default, dvs_bic_scores) and, through dvs_bn_scores, ``loglik``, ``aic``, ``bde`` (BDeu), ``bds``, ``k2`` and ``bdj`` with
bnlearn's arguments ``k`` (aic, bic) and ``iss`` (bde, bds) — definitions in include/dvs.h.  All of them are to be
maximised, as the search (search.py) and the predictor data (predictor_data.py) assume.  The three classes here are
``Evaluator``s (evaluator.py holds ``score_masks`` / ``toggle_scores`` / ``compact_parent_masks``); each names its entry points.
"""
from __future__ import annotations

import csv
from typing import List, Sequence

import numpy as np
import torch

from . import _lib as dl
from .evaluator import Evaluator, RowSets, check_k, check_positive, pack_levels, score_arg
from .features import LABEL_KEY, _as_labels_edges


def load_discrete_csv(path: str):
    """(names, level-coded uint8 array [S, n]); levels coded by sorted name (BIC does not depend on the coding)."""
    rows = list(csv.reader(open(path)))
    names, rows = rows[0], rows[1:]
    cols = []
    for c in range(len(names)):
        levels = sorted(set(r[c] for r in rows))
        index = {v: i for i, v in enumerate(levels)}
        cols.append(np.fromiter((index[r[c]] for r in rows), np.uint8, len(rows)))
    return names, np.stack(cols, 1)


PENALISED_SCORES = ("aic", "bic")        # take k
DIRICHLET_SCORES = ("bde", "bds")        # take iss


class _DiscreteEvaluator(Evaluator):
    """the refusal the evaluator of a discrete data set and its views share"""

    def _refusal(self, scratch):
        return ("a variable's parent set is too large for the on-chip counting paths (dense table: 36 864 "
                "cells; sorted samples: 16 384 samples, 63 key bits)")


class BNLearnWrapper(_DiscreteEvaluator):
    """``packed`` (int64 [S, ceil(n / 16)], 4-bit level codes), ``card`` (uint8 [n]) and its host copy ``card_host`` are the
    data set on the device; ``score_arg`` is the score type's argument as the library takes it."""

    def __init__(self, dataset_name: str, metric_name: str = "bic", data=None, device="cuda", *, iss=None, k=None):
        """``data``: path of a CSV with a header row of variable names, or a level-coded integer array [S, n].
        ``metric_name``: one of ``_lib.SCORE_TYPES``; ``k``: the penalty coefficient of aic (default 1) / bic (default
        log(S) / 2); ``iss``: the imaginary sample size of bde / bds (default 1)."""
        self._set_score(dataset_name, metric_name, iss, k)
        if data is None:
            raise ValueError("pass data=<csv path or level-coded array>: the reference's R data sets are not bundled")
        arr = load_discrete_csv(data)[1] if isinstance(data, str) else np.asarray(data)
        if arr.ndim != 2 or arr.shape[1] > dl.MAX_TOKENS or arr.min() < 0 or arr.max() > 15:
            raise ValueError("data must be [samples, n_vars <= 48] with level codes 0..15")
        packed = pack_levels(arr, range(arr.shape[1]), arr.shape[1])
        # card_host: pc.py sizes the CI tables' LDS from it
        device = torch.device(device)
        self._set_data(torch.from_numpy(packed).to(device), [int(c) for c in arr.max(0) + 1], device)

    @classmethod
    def from_packed(cls, dataset_name: str, metric_name: str, packed: torch.Tensor, card, *, iss=None, k=None):
        """An evaluator around rows that are already packed on the device (int64 [S, ceil(n / 16)], 4-bit level codes:
        what ``sample`` returns and ``packed`` holds), with no host round trip.  ``card`` (n level counts, 1..16) is taken as
        given, not read off the rows: a sample may miss a level.  ``metric_name``, ``iss`` and ``k`` as in ``__init__``."""
        self = cls.__new__(cls)
        self._set_score(dataset_name, metric_name, iss, k)
        card = dl.level_counts(card)
        n = len(card)
        if not torch.is_tensor(packed) or packed.device.type != "cuda":
            raise RuntimeError("dags_vae_search_amd: from_packed takes rows on the GPU; this package has no CPU path")
        if packed.dtype != torch.int64 or packed.ndim != 2 or packed.shape[0] < 1 or packed.shape[1] != (n + 15) // 16:
            raise ValueError(f"packed must be int64 [S >= 1, {(n + 15) // 16}] for {n} variables")
        self._set_data(packed.contiguous(), card, packed.device)
        return self

    def _set_score(self, dataset_name, metric_name, iss, k):
        if metric_name not in dl.SCORE_TYPES:
            raise NotImplementedError(f"built scores: {', '.join(sorted(dl.SCORE_TYPES))} (got {metric_name!r})")
        check_positive("iss", iss, metric_name, DIRICHLET_SCORES)
        check_k(k, metric_name, PENALISED_SCORES)
        self.dataset_name, self.metric_name, self.iss, self.k = dataset_name, metric_name, iss, k
        self.score_arg = score_arg(iss if iss is not None else k)

    def _set_data(self, packed, card_host, device):
        self.lib = dl.load()
        self.device = device
        self.n_samples, self.n_vars = int(packed.shape[0]), len(card_host)
        self.packed, self.card_host = packed, card_host
        self.card = torch.tensor(card_host, dtype=torch.uint8, device=self.device)

    def _head(self, parents):
        """what every scorer entry point over these rows starts with (include/dvs.h), a row-set view's included"""
        p = dl.ptr
        return parents.shape[0], self.n_vars, self.n_samples, p(self.packed), p(self.card), p(parents)

    def _score_args(self):
        return dl.SCORE_TYPES[self.metric_name], self.score_arg

    def _launch_scores(self, parents, scratch, out, status, used):
        """the default-penalty bic is dvs_bic_scores; everything else dvs_bn_scores"""
        p, lib = dl.ptr, self.lib
        if self.metric_name == "bic" and self.k is None:
            dl.check(lib, lib.dvs_bic_scores(*self._head(parents), p(scratch), p(out), p(status), dl.stream()), "dvs_bic_scores")
        else:
            dl.check(lib, lib.dvs_bn_scores(*self._head(parents), *self._score_args(), p(scratch), p(out), p(status), dl.stream()),
                     "dvs_bn_scores")

    def _launch_toggles(self, parents, worklist, L, T, status):
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_bn_toggle_scores(
            *self._head(parents), *self._score_args(), p(worklist), p(L), L.numel() * 8, p(T), T.numel() * 8, p(status),
            dl.stream()), "dvs_bn_toggle_scores")

    def _parent_masks(self, graphs: Sequence, label_key: str) -> np.ndarray:
        n = self.n_vars
        masks = np.zeros((len(graphs), n), np.uint64)
        for b, g in enumerate(graphs):
            labels, edges = _as_labels_edges(g, label_key)
            assert n == len(labels), f"Expected {n} vertices, but got {len(labels)}"                      # bnlearn.py:34
            assert sorted(labels) == list(range(n)), f"Expected graph labels from 0 to {n - 1}, but got {labels}"   # :35
            for u, v in edges:
                masks[b, labels[v]] |= np.uint64(1) << np.uint64(labels[u])
        return masks

    def score_batch(self, labeled_graphs: Sequence, label_key: str = LABEL_KEY) -> List[float]:
        masks = self._parent_masks(labeled_graphs, label_key)
        return self.score_masks(torch.from_numpy(masks.view(np.int64))).cpu().tolist()

    def score_compact(self, batch) -> torch.Tensor:
        """Score of a ``CompactBatch`` (records.py) that lives on the device -> float64 [B] on the device: the relabelling
        (dvs_bic_parent_masks) and the scoring (dvs_bic_scores / dvs_bn_scores) are both HIP launches, nothing touches
        the host."""
        parents, status = self._compact_parent_masks(batch)
        out = self.score_masks(parents)
        if int(status.item()) & dl.STATUS_LABELS:
            raise AssertionError(f"Expected graph labels from 0 to {self.n_vars - 1}")                        # bnlearn.py:35
        return out

    def with_rows(self, rows: torch.Tensor, set_of=None) -> "RowSetEvaluator":
        """A view of this evaluator in which every structure of a batch is scored on its own multiset of rows
        (dvs_bn_scores_rows / dvs_bn_toggle_scores_rows): ``rows`` int32 [n_sets, set_size] indices into this data set,
        ``set_of`` int32 [B] the set of each structure (None: structure b uses set b).  What ``hill_climb`` and
        ``tabu_search`` take to climb one bootstrap replicate per structure (strength.py)."""
        return RowSetEvaluator(self, rows, set_of)

    def available_case(self, observed: torch.Tensor, metric: str = "pnal", k=None) -> "AvailableCaseEvaluator":
        """A view of this evaluator's rows as incomplete data (dvs_bn_scores_avail / dvs_bn_toggle_scores_avail, DESIGN.md
        §26): ``observed`` int64 [n_samples] on the device, bit v set where variable v is observed in that row (what
        ``incomplete_rows`` returns next to the rows).  ``metric``: ``"nal"``, the node-average likelihood, or ``"pnal"``
        with the penalty coefficient ``k`` (default ``n_samples ** -0.25``).  This evaluator's own score type plays no part.
        What ``hill_climb`` and ``tabu_search`` take to learn a structure without dropping incomplete rows."""
        return AvailableCaseEvaluator(self, observed, metric, k)

    def score(self, labeled_graph, label_key: str = LABEL_KEY) -> float:
        return self.score_batch([labeled_graph], label_key)[0]


class RowSetEvaluator(_DiscreteEvaluator):
    """``BNLearnWrapper.with_rows``: the base evaluator's data, score and device, with structure b counted over the rows
    ``rows[set_of[b]]``.  ``n_samples`` is the set size: every score is, bit for bit, the base score type on the gathered
    data set (bic's default penalty is log(set_size) / 2).  The indices are checked here, once: the device does not."""

    def __init__(self, base: BNLearnWrapper, rows, set_of=None):
        self.base = base
        self.lib, self.device, self.n_vars, self.metric_name = base.lib, base.device, base.n_vars, base.metric_name
        self.dataset_name, self.iss, self.k = base.dataset_name, base.iss, base.k
        self.sets = sets = RowSets(rows, set_of, base.n_samples, self.device)
        self.rows, self.set_of, self.n_sets, self.n_samples = sets.rows, sets.set_of, sets.n_sets, sets.set_size

    def row_sets(self, B):
        return self.sets.of(B)

    def _tail(self, B):
        """what follows ``status`` in the ``_rows`` entry points, which take the plain ones' arguments up to there"""
        n_sets, set_of = self.sets.of(B)
        return dl.ptr(self.rows), self.n_samples, n_sets, dl.ptr(set_of), dl.stream()

    def _launch_scores(self, parents, scratch, out, status, used):
        p, base = dl.ptr, self.base
        dl.check(self.lib, self.lib.dvs_bn_scores_rows(*base._head(parents), *base._score_args(), p(scratch), p(out), p(status),
                                                       *self._tail(parents.shape[0])), "dvs_bn_scores_rows")

    def _launch_toggles(self, parents, worklist, L, T, status):
        p, base = dl.ptr, self.base
        dl.check(self.lib, self.lib.dvs_bn_toggle_scores_rows(
            *base._head(parents), *base._score_args(), p(worklist), p(L), L.numel() * 8, p(T), T.numel() * 8, p(status),
            *self._tail(parents.shape[0])), "dvs_bn_toggle_scores_rows")


AVAILABLE_CASE_SCORES = ("nal", "pnal")


class AvailableCaseEvaluator(_DiscreteEvaluator):
    """``BNLearnWrapper.available_case``: the base evaluator's rows, level counts and device, each family scored on exactly
    the rows that observe it whole: local = LL / m - k (r - 1) q (include/dvs_available.h).  ``nal`` is k = 0; the default k of
    ``pnal``, ``n_samples ** -0.25``, is computed here and is the alpha = 1/4 of Bodewes and Scutari (2021) as recalled: parity
    with bnlearn's ``nal`` / ``pnal`` is unpinned against an R run.  A family that no row observes whole scores -inf (status
    bit 7, which does not raise); a refused family raises as it does for the plain evaluator.  ``observed`` is checked here,
    once."""
    counts_used = True

    def __init__(self, base: BNLearnWrapper, observed, metric="pnal", k=None):
        if metric not in AVAILABLE_CASE_SCORES:
            raise NotImplementedError(f"available-case scores: {', '.join(AVAILABLE_CASE_SCORES)} (got {metric!r})")
        check_k(k, metric, ("pnal",))
        self.base = base
        self.lib, self.device, self.n_vars, self.n_samples = base.lib, base.device, base.n_vars, base.n_samples
        self.card, self.card_host = base.card, base.card_host       # no ``packed``: what reads rows off an evaluator must not take these as complete
        self.dataset_name, self.metric_name, self.iss, self.k = base.dataset_name, metric, None, k
        self.penalty = 0.0 if metric == "nal" else float(base.n_samples) ** -0.25 if k is None else float(k)
        if not torch.is_tensor(observed) or observed.dtype != torch.int64 or observed.shape != (base.n_samples,):
            raise ValueError(f"observed must be an int64 tensor [{base.n_samples}]: bit v set where variable v is observed")
        dl.require_cuda(observed, "observed")
        self.observed = observed.to(self.device).contiguous()
        seen = int(np.bitwise_or.reduce(self.observed.cpu().numpy().view(np.uint64)))
        never = [v for v in range(self.n_vars) if not (seen >> v) & 1]
        if never:
            raise ValueError(f"available_case: no row observes variable(s) {never}: nothing could score them")

    def _head(self, parents):
        """what the ``_avail`` entry points start with (include/dvs_available.h)"""
        p, base = dl.ptr, self.base
        return (parents.shape[0], self.n_vars, base.n_samples, p(base.packed), p(self.observed), p(base.card), p(parents),
                self.penalty)

    def _launch_scores(self, parents, scratch, out, status, used):
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_bn_scores_avail(*self._head(parents), p(scratch), p(out), p(used), p(status), dl.stream()),
                 "dvs_bn_scores_avail")

    def _launch_toggles(self, parents, worklist, L, T, status):
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_bn_toggle_scores_avail(
            *self._head(parents), p(worklist), p(L), L.numel() * 8, p(T), T.numel() * 8, p(status), dl.stream()),
            "dvs_bn_toggle_scores_avail")

    def used(self, parents: torch.Tensor) -> torch.Tensor:
        """the rows that count for every family of ``parents`` (int64 [B, n_vars]) -> int32 [B, n_vars]; 0 where no row does
        and where the family is refused"""
        parents = parents.to(self.device).contiguous()
        B = parents.shape[0]
        scratch = torch.empty(B, self.n_vars, dtype=torch.float64, device=self.device)
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        used = torch.empty(B, self.n_vars, dtype=torch.int32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.launch_scores(parents, scratch, out, status, used=used)
        return used

    def with_rows(self, rows, set_of=None):
        raise NotImplementedError("row sets over an available-case view (bootstrap on incomplete data) are not built")
