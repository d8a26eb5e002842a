"""Gaussian Bayesian networks on real-valued data on the device (csrc/dvs_gaussian.h).

The reference hands ``metric_name`` to ``bnlearn::score`` unseen; on a continuous data set that means ``loglik-g``, ``aic-g``,
``bic-g`` and ``bge``.  ``GaussianEvaluator`` is their evaluator: it holds the moments of its rows (``dvs_gbn_moments``: size,
means, centred cross-products) and scores families from fp64 Cholesky factors of their principal submatrices
(``dvs_gbn_scores``, ``dvs_gbn_toggle_scores``).  It has the surface ``hill_climb``, ``tabu_search``, ``exact_search``,
``local_score_table``, ``family_scores``, ``order_mcmc``, ``arc_posterior`` and ``boot_strength`` work through, so each of them
runs on real-valued data as it stands; ``gaussian_fit`` (``dvs_gbn_fit``) gives the regression parameters of a structure.

The definitions are those of include/dvs_gaussian.h.  Three things follow bnlearn as recalled and are unpinned against an R
run: the unbiased residual variance RSS / (m - p - 1) in the likelihood, the defaults alpha_mu = 1 (``iss_mu``) and alpha_w =
n + 2 (``iss_w``) of ``bge``, and its prior mean, the sample mean.  A family whose Cholesky pivot is within rounding of zero (a
duplicated or collinear column) and a family of more than ``_lib.GBN_MAX_PARENTS`` parents are refused: NaN in their cell.
``ci_tests``, ``ci_test``, ``pc_stable``, ``ci_tests_group``, ``mmpc``, ``rsmax2`` and ``mmhc`` take this evaluator with
``test`` "cor", "zf" or "mi-g" (include/dvs_gaussian_ci.h, DESIGN.md §30: the tests read ``moments``); with a discrete or
permutation test name, their default "mi" included, they raise ``ValueError``.  The entry points that read discrete levels
alone (``bn_fit``, ``cross_validate``, ``available_case``) raise ``ValueError`` on this evaluator: their Gaussian counterparts
are not built.
"""
from __future__ import annotations

import csv
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as dl
from .bic import BNLearnWrapper

PENALISED = ("aic-g", "bic-g")             # take k


def load_real_csv(path: str):
    """(names, float64 array [S, n]) of a CSV with a header row of variable names"""
    rows = list(csv.reader(open(path)))
    return rows[0], np.asarray([[float(x) for x in r] for r in rows[1:]], np.float64)


def _moments(lib, x, rows):
    """dvs_gbn_moments of the device rows ``x`` f64 [S, n] over ``rows`` (int32 [n_sets, set_size] or None) -> f64 [n_sets, stride]"""
    S, n = x.shape
    n_sets, size = (1, S) if rows is None else rows.shape
    ws = torch.empty(dl.workspace_bytes(lib, "dvs_gbn_moments_workspace_bytes", n, n_sets, size), dtype=torch.uint8, device=x.device)
    mom = torch.empty(n_sets, dl.gbn_stride(n), dtype=torch.float64, device=x.device)
    dl.check(lib, lib.dvs_gbn_moments(n, S, dl.ptr(x), dl.ptr(rows), n_sets, size, dl.ptr(ws), dl.nbytes(ws), dl.ptr(mom),
                                      dl.nbytes(mom), dl.stream()), "dvs_gbn_moments")
    return mom


class _GaussianScorer:
    """The launches of the Gaussian evaluators: ``moments`` f64 [n_sets, stride] and ``set_of`` (int32 [B] or None: set 0, or
    structure b on set b for a row-set view) name the data; the score type and its arguments are the base evaluator's."""
    continuous = True                      # what _lib.need_discrete looks at

    def _sets(self, B):
        return self.moments.shape[0], None

    def _score_args(self):
        return dl.GSCORE_TYPES[self.metric_name], self.score_arg, self.score_arg2

    def launch_scores(self, parents, scratch, out, status, used=None):
        """``dvs_gbn_scores`` on the caller's buffers, unchecked: ``parents`` int64 [B, n_vars] contiguous on the device ->
        ``scratch`` f64 [B, n_vars] (the local scores), ``out`` f64 [B], ``status`` int32 [1] (bit 4: a family was refused)."""
        if used is not None:
            raise ValueError("used= is what an available-case view counts (BNLearnWrapper.available_case)")
        n_sets, set_of = self._sets(parents.shape[0])
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_gbn_scores(parents.shape[0], self.n_vars, p(self.moments), n_sets, p(set_of), p(parents),
                                                   *self._score_args(), p(scratch), p(out), p(status), dl.stream()), "dvs_gbn_scores")

    def score_masks(self, parents: torch.Tensor, local: bool = False):
        """parents: int64 [B, n_vars] bit rows (bit u of [b, v] <=> u -> v) -> f64 [B], or with ``local`` (scores f64 [B],
        local scores f64 [B, n_vars]).  A refused family (collinear columns, too many parents, too few rows) raises."""
        parents = parents.to(self.device).contiguous()
        B = parents.shape[0]
        scratch = torch.empty(B, self.n_vars, dtype=torch.float64, device=self.device)
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.launch_scores(parents, scratch, out, status)
        if int(status.item()) & dl.STATUS_REFUSED:
            raise ValueError(f"a family was refused: a Cholesky pivot within rounding of zero (a duplicated or collinear "
                             f"column), more than {dl.GBN_MAX_PARENTS} parents, a parent bit >= {self.n_vars}, or fewer "
                             f"than p + 2 rows for a likelihood score")
        return (out, scratch) if local else out

    def toggle_scores(self, parents: torch.Tensor, *, worklist=None, out=None, return_status: bool = False):
        """The single-edge neighbourhood of every structure (dvs_gbn_toggle_scores) -> (L f64 [B, n_vars], T f64 [B, n_vars,
        n_vars]), with the meaning, the ``worklist`` / ``out`` pass and ``return_status`` of ``BNLearnWrapper.toggle_scores``."""
        parents = parents.to(self.device).contiguous()
        B, n = parents.shape
        assert n == self.n_vars, f"Expected {self.n_vars} variables, but got {n}"
        n_sets, set_of = self._sets(B)
        if out is None:
            if worklist is not None:
                raise ValueError("an incremental pass (worklist=) updates a table in place: pass out=(L, T)")
            out = (torch.empty(B, n, dtype=torch.float64, device=self.device),
                   torch.empty(B, n, n, dtype=torch.float64, device=self.device))
        L, T = out
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_gbn_toggle_scores(
            B, n, p(self.moments), n_sets, p(set_of), p(parents), *self._score_args(), p(worklist), p(L), L.numel() * 8, p(T),
            T.numel() * 8, p(status), dl.stream()), "dvs_gbn_toggle_scores")
        return (L, T, status) if return_status else (L, T)

    def available_case(self, *args, **kwargs):
        dl.need_discrete("available_case", self)


class GaussianEvaluator(_GaussianScorer):
    """``x`` (f64 [S, n] on the device) is the data set, ``moments`` (f64 [1, 1 + n + n n]) what the scorers read."""

    def __init__(self, dataset_name: str, metric_name: str = "bic-g", data=None, device="cuda", *, k=None, iss_mu=None, iss_w=None):
        """``data``: path of a CSV with a header row of variable names, or a real array [S, n <= 48] (float32 is converted
        once).  ``metric_name``: ``loglik-g``, ``aic-g``, ``bic-g`` or ``bge``; ``k``: the penalty coefficient of aic-g
        (default 1) / bic-g (default log(S) / 2); ``iss_mu``, ``iss_w``: bge's alpha_mu (default 1) and alpha_w (default
        n + 2, must exceed n + 1)."""
        if data is None:
            raise ValueError("pass data=<csv path or real array [S, n]>")
        arr = load_real_csv(data)[1] if isinstance(data, str) else np.asarray(data)
        if arr.ndim != 2 or arr.shape[0] < 1 or not 1 <= arr.shape[1] <= dl.MAX_TOKENS or arr.dtype.kind != "f":
            raise ValueError("data must be a real array [samples >= 1, 1 <= n_vars <= 48]")
        device = torch.device(device)
        dl.need_cuda("GaussianEvaluator", device)
        self._set(dataset_name, metric_name, k, iss_mu, iss_w, torch.from_numpy(np.array(arr, np.float64, order="C")).to(device))

    @classmethod
    def from_device(cls, dataset_name: str, metric_name: str, x: torch.Tensor, *, k=None, iss_mu=None, iss_w=None):
        """An evaluator around rows that are already on the device (float64 or float32 [S, n <= 48]), with no host round trip."""
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise RuntimeError("dags_vae_search_amd: from_device takes rows on the GPU; this package has no CPU path")
        if x.ndim != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= dl.MAX_TOKENS or x.dtype not in (torch.float32, torch.float64):
            raise ValueError("x must be float64 or float32 [S >= 1, 1 <= n <= 48]")
        self = cls.__new__(cls)
        self._set(dataset_name, metric_name, k, iss_mu, iss_w, x.to(torch.float64).contiguous())
        return self

    def _set(self, dataset_name, metric_name, k, iss_mu, iss_w, x):
        if metric_name not in dl.GSCORE_TYPES:
            raise NotImplementedError(f"built Gaussian scores: {', '.join(sorted(dl.GSCORE_TYPES))} (got {metric_name!r})")
        n = int(x.shape[1])
        if k is not None and metric_name not in PENALISED:
            raise ValueError(f"k is the argument of {' / '.join(PENALISED)}, not of {metric_name!r}")
        if (iss_mu is not None or iss_w is not None) and metric_name != "bge":
            raise ValueError(f"iss_mu and iss_w are the arguments of bge, not of {metric_name!r}")
        if k is not None and not (math.isfinite(k) and k >= 0):
            raise ValueError(f"k must be finite and >= 0 (got {k!r})")
        if iss_mu is not None and not (math.isfinite(iss_mu) and iss_mu > 0):
            raise ValueError(f"iss_mu must be finite and > 0 (got {iss_mu!r})")
        if iss_w is not None and not (math.isfinite(iss_w) and iss_w > n + 1):
            raise ValueError(f"iss_w must be finite and > n_vars + 1 = {n + 1} (got {iss_w!r})")
        self.dataset_name, self.metric_name, self.k, self.iss_mu, self.iss_w = dataset_name, metric_name, k, iss_mu, iss_w
        first = iss_mu if metric_name == "bge" else k
        self.score_arg = float("nan") if first is None else float(first)         # NaN: the type's default (include/dvs_gaussian.h)
        self.score_arg2 = float("nan") if iss_w is None else float(iss_w)
        self.lib, self.device, self.x = dl.load(), x.device, x
        self.n_samples, self.n_vars = int(x.shape[0]), n
        with torch.cuda.device(self.device):
            self.moments = _moments(self.lib, x, None)

    @property
    def mean(self) -> torch.Tensor:
        """f64 [n]: the column means"""
        return self.moments[0, 1:1 + self.n_vars]

    @property
    def cross_products(self) -> torch.Tensor:
        """f64 [n, n]: the centred cross-products, sum (x_i - mean_i) (x_j - mean_j)"""
        return self.moments[0, 1 + self.n_vars:].view(self.n_vars, self.n_vars)

    # the relabelling of a CompactBatch (dvs_bic_parent_masks) reads no data: BNLearnWrapper's own, unbound from its class
    _compact_parent_masks = BNLearnWrapper._compact_parent_masks
    compact_parent_masks = BNLearnWrapper.compact_parent_masks

    def with_rows(self, rows: torch.Tensor, set_of=None) -> "GaussianRowSetEvaluator":
        """A view in which every structure of a batch is scored on its own multiset of rows: ``rows`` int32 [n_sets, set_size]
        indices into this data set, ``set_of`` int32 [B] the set of each structure (None: structure b uses set b).  The
        moments of all sets come from one ``dvs_gbn_moments`` call and are, as bytes, those of the gathered rows."""
        return GaussianRowSetEvaluator(self, rows, set_of)


class GaussianRowSetEvaluator(_GaussianScorer):
    """``GaussianEvaluator.with_rows``: the base evaluator's score and device over the moments of the row sets.  ``n_samples``
    is the set size.  The indices are checked here, once: the device does not."""

    def __init__(self, base: GaussianEvaluator, rows, set_of=None):
        self.base = base
        self.lib, self.device, self.n_vars, self.metric_name = base.lib, base.device, base.n_vars, base.metric_name
        self.dataset_name, self.k, self.iss_mu, self.iss_w = base.dataset_name, base.k, base.iss_mu, base.iss_w
        self.score_arg, self.score_arg2 = base.score_arg, base.score_arg2
        if not torch.is_tensor(rows) or rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1 or \
                rows.dtype not in (torch.int32, torch.int64):
            raise ValueError("rows must be an integer tensor [n_sets >= 1, set_size >= 1]")
        rows = rows.to(self.device)
        if int(torch.amin(rows)) < 0 or int(torch.amax(rows)) >= base.n_samples:
            raise ValueError(f"rows must lie in [0, {base.n_samples})")
        self.rows = rows.to(torch.int32).contiguous()
        self.n_sets, self.n_samples = int(rows.shape[0]), int(rows.shape[1])
        self.set_of = None
        if set_of is not None:
            set_of = torch.as_tensor(set_of).to(self.device)
            if set_of.ndim != 1 or set_of.numel() < 1 or set_of.dtype not in (torch.int32, torch.int64):
                raise ValueError("set_of must be an integer tensor [B]")
            if int(torch.amin(set_of)) < 0 or int(torch.amax(set_of)) >= self.n_sets:
                raise ValueError(f"set_of must lie in [0, {self.n_sets})")
            self.set_of = set_of.to(torch.int32).contiguous()
        with torch.cuda.device(self.device):
            self.moments = _moments(self.lib, base.x, self.rows)
            self._own = torch.arange(self.n_sets, dtype=torch.int32, device=self.device)      # structure b on set b

    def compact_parent_masks(self, batch) -> torch.Tensor:
        return self.base.compact_parent_masks(batch)

    def _sets(self, B):
        if self.set_of is None:
            if B > self.n_sets:
                raise ValueError(f"{B} structures but {self.n_sets} row sets: pass set_of")
            return self.n_sets, self._own
        if self.set_of.numel() != B:
            raise ValueError(f"{B} structures but set_of names {self.set_of.numel()}")
        return self.n_sets, self.set_of

    def with_rows(self, rows, set_of=None):
        raise NotImplementedError("row sets over a row-set view are not built: index the base evaluator's rows")


@dataclass
class FittedGBN:
    parents: torch.Tensor                  # int64 [B, n]: the structures
    coef: torch.Tensor                     # f64 [B, n, n]: coef[b, v, u] the regression coefficient of u in v's equation, 0 off the parent set
    intercept: torch.Tensor                # f64 [B, n]
    sd: torch.Tensor                       # f64 [B, n]: the residual standard deviation, sqrt(RSS / (m - p - 1))


def gaussian_fit(evaluator, parents) -> FittedGBN:
    """bnlearn's ``bn.fit`` on a Gaussian network, for a batch: ``parents`` int64 [n] or [B, n] parent masks -> the regression
    of every variable on its parents from the evaluator's moments (dvs_gbn_fit).  A family the scorer would refuse (collinear
    columns, more than ``_lib.GBN_MAX_PARENTS`` parents, fewer than p + 2 rows) raises ``ValueError``."""
    what = "gaussian_fit"
    if not getattr(evaluator, "continuous", False):
        raise ValueError(f"{what}: the evaluator holds discrete data: bn_fit fits its tables")
    if not torch.is_tensor(parents) or parents.dtype != torch.int64 or parents.ndim not in (1, 2):
        raise ValueError(f"{what}: parents must be an int64 tensor [n] or [B, n] of parent masks")
    n, dev, lib, p = evaluator.n_vars, evaluator.device, evaluator.lib, dl.ptr
    parents = parents.reshape(-1, parents.shape[-1]).to(dev).contiguous()
    if parents.shape[1] != n or parents.shape[0] < 1:
        raise ValueError(f"{what}: expected {n} variables per structure, got {tuple(parents.shape)}")
    B = parents.shape[0]
    n_sets, set_of = evaluator._sets(B)
    with torch.cuda.device(dev):
        coef = torch.empty(B, n, n, dtype=torch.float64, device=dev)
        intercept = torch.empty(B, n, dtype=torch.float64, device=dev)
        sd = torch.empty(B, n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_fit(B, n, p(evaluator.moments), n_sets, p(set_of), p(parents), p(coef), dl.nbytes(coef),
                                      p(intercept), p(sd), p(status), dl.stream()), "dvs_gbn_fit")
        if int(status.item()) & dl.STATUS_REFUSED:
            bad = torch.nonzero(torch.isnan(sd)).cpu().tolist()
            raise ValueError(f"{what}: refused families (structure, variable): {bad[:8]}: collinear columns, more than "
                             f"{dl.GBN_MAX_PARENTS} parents, a parent bit >= {n}, or fewer than p + 2 rows")
    return FittedGBN(parents, coef, intercept, sd)
