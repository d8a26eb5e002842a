"""The surface every evaluator offers the searches, stated once.

``hill_climb``, ``tabu_search``, ``boot_strength``, ``exact_search``, ``order_mcmc``, ``pc_stable``, ``mmpc`` ... work through "an
evaluator".  ``Evaluator`` holds the bodies of that surface; a subclass (bic.py, gaussian.py, mixed.py) holds its data and the
hooks.  Next to it: what the constructors share: the checks of row sets and score arguments, the packing of level codes.
"""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

from . import _lib as dl


def check_k(k, metric_name, takers):
    """``k``, the penalty coefficient of the score types ``takers``"""
    if k is not None and metric_name not in takers:
        raise ValueError(f"k is the argument of {' / '.join(takers)}, not of {metric_name!r}")
    if k is not None and not (math.isfinite(k) and k >= 0):
        raise ValueError(f"k must be finite and >= 0 (got {k!r})")


def check_positive(name, value, metric_name=None, takers=()):
    """an imaginary sample size (``iss``, ``iss_mu``) of the score types ``takers`` (none: the caller has checked the type)"""
    if value is not None and takers and metric_name not in takers:
        raise ValueError(f"{name} is the argument of {' / '.join(takers)}, not of {metric_name!r}")
    if value is not None and not (math.isfinite(value) and value > 0):
        raise ValueError(f"{name} must be finite and > 0 (got {value!r})")


def score_arg(value) -> float:
    """a score type's argument as the library takes it; NaN: the type's default (include/dvs.h)"""
    return float("nan") if value is None else float(value)


def pack_levels(codes: np.ndarray, cols, n) -> np.ndarray:
    """level codes [S, len(cols)] of the variables ``cols`` -> the packed int64 rows [S, ceil(n / 16)]: variable v in nibble
    v % 16 of word v // 16, the other nibbles zero"""
    packed = np.zeros((codes.shape[0], (n + 15) // 16), np.uint64)
    for j, v in enumerate(cols):
        packed[:, v // 16] |= codes[:, j].astype(np.uint64) << np.uint64(4 * (v % 16))
    return packed.view(np.int64)


class RowSets:
    """``rows`` int32 [n_sets, set_size] indices into a data set of ``n_samples`` rows and ``set_of`` (int32 [B] or None:
    structure b on set b) of a row-set view, on ``device``.  The indices are checked here, once, on the device the caller's
    tensors are on: the library does not."""

    def __init__(self, rows, set_of, n_samples, device):
        if not torch.is_tensor(rows) or rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1 or \
                rows.dtype not in (torch.int32, torch.int64):
            raise ValueError("rows must be an integer tensor [n_sets >= 1, set_size >= 1]")
        if int(torch.amin(rows)) < 0 or int(torch.amax(rows)) >= n_samples:
            raise ValueError(f"rows must lie in [0, {n_samples})")
        self.rows = rows.to(device=device, dtype=torch.int32).contiguous()
        self.n_sets, self.set_size = int(rows.shape[0]), int(rows.shape[1])
        self.set_of = None
        if set_of is not None:
            set_of = torch.as_tensor(set_of)
            if set_of.ndim != 1 or set_of.numel() < 1 or set_of.dtype not in (torch.int32, torch.int64):
                raise ValueError("set_of must be an integer tensor [B]")
            if int(torch.amin(set_of)) < 0 or int(torch.amax(set_of)) >= self.n_sets:
                raise ValueError(f"set_of must lie in [0, {self.n_sets})")
            self.set_of = set_of.to(device=device, dtype=torch.int32).contiguous()

    def of(self, B):
        """(n_sets, set_of) for a batch of ``B`` structures"""
        if self.set_of is None:
            if B > self.n_sets:
                raise ValueError(f"{B} structures but {self.n_sets} row sets: pass set_of")
        elif self.set_of.numel() != B:
            raise ValueError(f"{B} structures but set_of names {self.set_of.numel()}")
        return self.n_sets, self.set_of


_NO_GUARD = contextlib.nullcontext()


class Evaluator:
    """A subclass sets ``lib``, ``device``, ``n_vars``, ``n_samples`` and ``data_kind``, and implements

    * ``_launch_scores(parents, scratch, out, status, used)``: the scorer's library call on the caller's buffers;
    * ``_launch_toggles(parents, worklist, L, T, status)``: the toggle table's;
    * ``_refusal(scratch) -> str``: what ``score_masks`` raises when status bit 4 is set;
    * ``row_sets(B)``, where a batch of B structures does not read one set of rows.

    ``score_masks``, ``toggle_scores`` and ``compact_parent_masks`` run with the evaluator's device current (``_guard``), so
    their launches go to that device's stream whatever the caller's current device is."""
    data_kind = "discrete"                 # "discrete" / "continuous" / "mixed": what _lib.need_discrete and need_unmixed read
    counts_used = False                    # whether launch_scores fills used= (an available-case view)

    def _guard(self):
        """the evaluator's device made current for a body's launches; a device without an index is the current one already"""
        index = self.device.index
        return _NO_GUARD if index is None else torch.cuda.device(index)

    def row_sets(self, B):
        """(n_sets, set_of int32 [B] or None) of a batch of ``B`` structures: here the data set is the one set"""
        return 1, None

    def launch_scores(self, parents, scratch, out, status, used=None):
        """The scorer on the caller's buffers, unchecked: ``parents`` int64 [B, n_vars] contiguous on the device ->
        ``scratch`` f64 [B, n_vars] (the local scores), ``out`` f64 [B], ``status`` int32 [1] (bit 4: a family was refused).
        An available-case view also fills ``used`` int32 [B, n_vars], the rows that counted per family."""
        if used is not None and not self.counts_used:
            raise ValueError("used= is what an available-case view counts (BNLearnWrapper.available_case)")
        self._launch_scores(parents, scratch, out, status, used)

    def score_masks(self, parents: torch.Tensor, local: bool = False):
        """parents: int64 [B, n_vars] bit rows in data-set variable indices (bit u of [b, v] <=> u -> v); -> f64 [B], or
        with ``local`` (scores f64 [B], per-variable local scores f64 [B, n_vars]).  A refused family raises."""
        with self._guard():
            parents = parents.to(self.device).contiguous()
            B = parents.shape[0]
            scratch = torch.empty(B, self.n_vars, dtype=torch.float64, device=self.device)
            out = torch.empty(B, dtype=torch.float64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.launch_scores(parents, scratch, out, status)
            if int(status.item()) & dl.STATUS_REFUSED:
                raise ValueError(self._refusal(scratch))
        return (out, scratch) if local else out

    def toggle_scores(self, parents: torch.Tensor, *, worklist=None, out=None, return_status: bool = False):
        """The single-edge neighbourhood of every structure -> (L f64 [B, n_vars], T f64 [B, n_vars, n_vars])
        on the device: L the local scores as ``score_masks(local=True)`` gives them, T[b, v, u] the local score of v with
        bit u of ``parents[b, v]`` flipped (NaN on the diagonal and where the family is refused: that move is not
        available).  ``worklist`` (int32 [2 B], ``hill_climb``'s) with ``out=(L, T)`` recomputes only the rows it names, in
        place.  ``return_status`` appends the status word (bit 4: some family was refused)."""
        with self._guard():
            parents = parents.to(self.device).contiguous()
            B, n = parents.shape
            assert n == self.n_vars, f"Expected {self.n_vars} variables, but got {n}"
            if out is None:
                if worklist is not None:
                    raise ValueError("an incremental pass (worklist=) updates a table in place: pass out=(L, T)")
                out = (torch.empty(B, n, dtype=torch.float64, device=self.device),
                       torch.empty(B, n, n, dtype=torch.float64, device=self.device))
            L, T = out
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._launch_toggles(parents, worklist, L, T, status)
        return (L, T, status) if return_status else (L, T)

    def _compact_parent_masks(self, batch):
        """(parent masks, the relabelling's status word), both on the device and unchecked"""
        with self._guard():
            labels = batch.labels.to(self.device).contiguous()
            preds = batch.preds.to(self.device).contiguous()
            B, n = labels.shape
            assert n == self.n_vars, f"Expected {self.n_vars} vertices, but got {n}"                         # bnlearn.py:34
            parents = torch.empty(B, n, dtype=torch.int64, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            p = dl.ptr
            dl.check(self.lib, self.lib.dvs_bic_parent_masks(B, n, 1 if preds.dtype == torch.int64 else 0, p(labels), p(preds),
                                                             p(parents), p(status), dl.stream()), "dvs_bic_parent_masks")
        return parents, status

    def compact_parent_masks(self, batch) -> torch.Tensor:
        """Parent masks (int64 [B, n_vars], data-set variable indices) of a ``CompactBatch`` that lives on the device: the
        relabelling of bnlearn.py:34-45 as one HIP launch (dvs_bic_parent_masks), which reads no data.  What ``score_masks``,
        ``toggle_scores`` and ``hill_climb`` take."""
        parents, status = self._compact_parent_masks(batch)
        if int(status.item()) & dl.STATUS_LABELS:
            raise AssertionError(f"Expected graph labels from 0 to {self.n_vars - 1}")                        # bnlearn.py:35
        return parents
