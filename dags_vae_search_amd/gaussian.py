"""Gaussian Bayesian networks on real-valued data on the device (csrc/dvs_gaussian.h).

The reference hands ``metric_name`` to ``bnlearn::score`` unseen; on a continuous data set that means ``loglik-g``, ``aic-g``,
``bic-g`` and ``bge``.  ``GaussianEvaluator`` is their evaluator: it holds the moments of its rows (``dvs_gbn_moments``: size,
means, centred cross-products) and scores families from fp64 Cholesky factors of their principal submatrices
(``dvs_gbn_scores``, ``dvs_gbn_toggle_scores``).  It is an ``Evaluator`` (evaluator.py), the surface ``hill_climb``, ``tabu_search``, ``exact_search``,
``local_score_table``, ``family_scores``, ``order_mcmc``, ``arc_posterior`` and ``boot_strength`` work through, so each of them
runs on real-valued data as it stands; ``gaussian_fit`` (``dvs_gbn_fit``) gives the regression parameters of a structure.

The definitions are those of include/dvs_gaussian.h.  Three things follow bnlearn as recalled and are unpinned against an R
run: the unbiased residual variance RSS / (m - p - 1) in the likelihood, the defaults alpha_mu = 1 (``iss_mu``) and alpha_w =
n + 2 (``iss_w``) of ``bge``, and its prior mean, the sample mean.  A family whose Cholesky pivot is within rounding of zero (a
duplicated or collinear column) and a family of more than ``_lib.GBN_MAX_PARENTS`` parents are refused: NaN in their cell.
``ci_tests``, ``ci_test``, ``pc_stable``, ``ci_tests_group``, ``mmpc``, ``rsmax2`` and ``mmhc`` take this evaluator with
``test`` "cor", "zf" or "mi-g" (include/dvs_gaussian_ci.h, DESIGN.md §30: the tests read ``moments``); with a discrete or
permutation test name, their default "mi" included, they raise ``ValueError``.  The entry points that read discrete levels
alone (``bn_fit``, ``cross_validate``, ``available_case``) raise ``ValueError`` on this evaluator; the counterparts of the first
two have names of their own, ``gaussian_fit`` and ``gaussian_cross_validate``.

A data set that holds factors next to real columns has an evaluator of its own, ``MixedEvaluator`` (mixed.py),
whose cells on all-real data are this one's bytes.

A ``FittedGBN`` goes to ``gaussian_joint`` (bnlearn's gbn2mvnorm), ``gaussian_sample`` (rbn), ``gaussian_log_likelihood`` (logLik
on held-out rows) and ``gaussian_predict`` (from the parents, or the exact conditional given every other variable):
include/dvs_gaussian_params.h, DESIGN.md §31.
"""
from __future__ import annotations

import csv
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib as dl
from .evaluator import Evaluator, RowSets, check_k, check_positive, score_arg

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


class _GaussianScorer(Evaluator):
    """The launches of the Gaussian evaluators: ``moments`` f64 [n_sets, stride] and ``row_sets`` (set 0, or structure b on set
    b for a row-set view) name the data; the score type and its arguments are the base evaluator's."""
    data_kind = "continuous"

    def _head(self, parents):
        """what dvs_gbn_scores and dvs_gbn_toggle_scores start with (include/dvs_gaussian.h)"""
        B, p = parents.shape[0], dl.ptr
        n_sets, set_of = self.row_sets(B)
        return (B, self.n_vars, p(self.moments), n_sets, p(set_of), p(parents), dl.GSCORE_TYPES[self.metric_name], self.score_arg,
                self.score_arg2)

    def _launch_scores(self, parents, scratch, out, status, used):
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_gbn_scores(*self._head(parents), p(scratch), p(out), p(status), dl.stream()), "dvs_gbn_scores")

    def _launch_toggles(self, parents, worklist, L, T, status):
        p = dl.ptr
        dl.check(self.lib, self.lib.dvs_gbn_toggle_scores(
            *self._head(parents), p(worklist), p(L), L.numel() * 8, p(T), T.numel() * 8, p(status), dl.stream()),
            "dvs_gbn_toggle_scores")

    def _refusal(self, scratch):
        return (f"a family was refused: a Cholesky pivot within rounding of zero (a duplicated or collinear "
                f"column), more than {dl.GBN_MAX_PARENTS} parents, a parent bit >= {self.n_vars}, or fewer "
                f"than p + 2 rows for a likelihood score")

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
        self._set_score(dataset_name, metric_name, k, iss_mu, iss_w, arr.shape[1])
        self._set_data(torch.from_numpy(np.array(arr, np.float64, order="C")).to(device))

    @classmethod
    def from_device(cls, dataset_name: str, metric_name: str, x: torch.Tensor, *, k=None, iss_mu=None, iss_w=None):
        """An evaluator around rows that are already on the device (float64 or float32 [S, n <= 48]), with no host round trip."""
        if not torch.is_tensor(x) or x.device.type != "cuda":
            raise RuntimeError("dags_vae_search_amd: from_device takes rows on the GPU; this package has no CPU path")
        if x.ndim != 2 or x.shape[0] < 1 or not 1 <= x.shape[1] <= dl.MAX_TOKENS or x.dtype not in (torch.float32, torch.float64):
            raise ValueError("x must be float64 or float32 [S >= 1, 1 <= n <= 48]")
        self = cls.__new__(cls)
        self._set_score(dataset_name, metric_name, k, iss_mu, iss_w, x.shape[1])
        self._set_data(x.to(torch.float64).contiguous())
        return self

    def _set_score(self, dataset_name, metric_name, k, iss_mu, iss_w, n):
        if metric_name not in dl.GSCORE_TYPES:
            raise NotImplementedError(f"built Gaussian scores: {', '.join(sorted(dl.GSCORE_TYPES))} (got {metric_name!r})")
        check_k(k, metric_name, PENALISED)
        if (iss_mu is not None or iss_w is not None) and metric_name != "bge":
            raise ValueError(f"iss_mu and iss_w are the arguments of bge, not of {metric_name!r}")
        check_positive("iss_mu", iss_mu)
        if iss_w is not None and not (math.isfinite(iss_w) and iss_w > n + 1):
            raise ValueError(f"iss_w must be finite and > n_vars + 1 = {n + 1} (got {iss_w!r})")
        self.dataset_name, self.metric_name, self.k, self.iss_mu, self.iss_w = dataset_name, metric_name, k, iss_mu, iss_w
        self.score_arg, self.score_arg2 = score_arg(iss_mu if metric_name == "bge" else k), score_arg(iss_w)

    def _set_data(self, x):
        self.lib, self.device, self.x = dl.load(), x.device, x
        self.n_samples, self.n_vars = int(x.shape[0]), int(x.shape[1])
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
        self.sets = sets = RowSets(rows, set_of, base.n_samples, self.device)
        self.rows, self.set_of, self.n_sets, self.n_samples = sets.rows, sets.set_of, sets.n_sets, sets.set_size
        with torch.cuda.device(self.device):
            self.moments = _moments(self.lib, base.x, self.rows)
            self._own = torch.arange(self.n_sets, dtype=torch.int32, device=self.device)      # structure b on set b

    def row_sets(self, B):
        n_sets, set_of = self.sets.of(B)
        return n_sets, self._own if set_of is None else set_of

    def with_rows(self, rows, set_of=None):
        raise NotImplementedError("row sets over a row-set view are not built: index the base evaluator's rows")


class GaussianMomentsEvaluator(_GaussianScorer):
    """A Gaussian scorer over moments that are given, not taken from rows: f64 [1, 1 + n + n n] in ``dvs_gbn_moments``'s layout
    (size, means, centred cross-products), e.g. the expected moments of incomplete data (``ExpectedMoments.evaluator``,
    gaussian_incomplete.py).  It has the whole evaluator surface, so the searches and ``gaussian_fit`` take it as they take a
    ``GaussianEvaluator``; it has no rows (no ``x``), so what reads rows refuses it, and the CI tests do too: whether a test on
    expected moments should count the rows as observed is not decided here."""
    ci_refusal = ("the evaluator holds given (expected) moments, not rows: a CI test would count every row as observed, and what a "
                  "test on expected moments means is not decided")

    def __init__(self, dataset_name: str, metric_name: str, moments: torch.Tensor, *, k=None, iss_mu=None, iss_w=None):
        if not torch.is_tensor(moments) or moments.device.type != "cuda":
            raise RuntimeError("dags_vae_search_amd: GaussianMomentsEvaluator takes moments on the GPU; this package has no CPU path")
        if moments.dtype != torch.float64 or moments.ndim != 2 or moments.shape[0] != 1 or moments.shape[1] < 3:
            raise ValueError("moments must be float64 [1, 1 + n + n n] (dvs_gbn_moments's layout)")
        n = int(round((math.sqrt(4 * moments.shape[1] - 3) - 1) / 2))
        if not 1 <= n <= dl.MAX_TOKENS or dl.gbn_stride(n) != moments.shape[1]:
            raise ValueError("moments must be float64 [1, 1 + n + n n] with 1 <= n <= 48")
        GaussianEvaluator._set_score(self, dataset_name, metric_name, k, iss_mu, iss_w, n)
        self.lib, self.device, self.moments = dl.load(), moments.device, moments.contiguous()
        self.n_vars, self.n_samples = n, int(moments[0, 0].item())

    def with_rows(self, rows, set_of=None):
        raise NotImplementedError("a GaussianMomentsEvaluator holds moments, not rows: there is nothing to index")


@dataclass
class FittedGBN:
    parents: torch.Tensor                  # int64 [B, n]: the structures
    coef: torch.Tensor                     # f64 [B, n, n]: coef[b, v, u] the regression coefficient of u in v's equation, 0 off the parent set
    intercept: torch.Tensor                # f64 [B, n]
    sd: torch.Tensor                       # f64 [B, n]: the residual standard deviation, sqrt(RSS / (m - p - 1))

    @property
    def batch(self) -> int:
        return int(self.parents.shape[0])

    @property
    def n_vars(self) -> int:
        return int(self.parents.shape[1])

    @property
    def device(self) -> torch.device:
        return self.parents.device


def _fit(what, evaluator, parents):
    """dvs_gbn_fit -> (FittedGBN, status); the checks of gaussian_fit"""
    dl.need_unmixed(what, evaluator)
    if dl.data_kind(evaluator) != "continuous":
        raise ValueError(f"{what}: the evaluator holds discrete data: bn_fit fits its tables")
    if not torch.is_tensor(parents) or parents.dtype != torch.int64 or parents.ndim not in (1, 2):
        raise ValueError(f"{what}: parents must be an int64 tensor [n] or [B, n] of parent masks")
    n, dev, lib, p = evaluator.n_vars, evaluator.device, evaluator.lib, dl.ptr
    parents = parents.reshape(-1, parents.shape[-1]).to(dev).contiguous()
    if parents.shape[1] != n or parents.shape[0] < 1:
        raise ValueError(f"{what}: expected {n} variables per structure, got {tuple(parents.shape)}")
    B = parents.shape[0]
    n_sets, set_of = evaluator.row_sets(B)
    with torch.cuda.device(dev):
        coef = torch.empty(B, n, n, dtype=torch.float64, device=dev)
        intercept = torch.empty(B, n, dtype=torch.float64, device=dev)
        sd = torch.empty(B, n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_fit(B, n, p(evaluator.moments), n_sets, p(set_of), p(parents), p(coef), dl.nbytes(coef),
                                      p(intercept), p(sd), p(status), dl.stream()), "dvs_gbn_fit")
        st = int(status.item())
    return FittedGBN(parents, coef, intercept, sd), st


def _refused_families(n):
    return f"collinear columns, more than {dl.GBN_MAX_PARENTS} parents, a parent bit >= {n}, or fewer than p + 2 rows"


def gaussian_fit(evaluator, parents) -> FittedGBN:
    """bnlearn's ``bn.fit`` on a Gaussian network, for a batch: ``parents`` int64 [n] or [B, n] parent masks -> the regression
    of every variable on its parents from the evaluator's moments (dvs_gbn_fit).  A family the scorer would refuse (collinear
    columns, more than ``_lib.GBN_MAX_PARENTS`` parents, fewer than p + 2 rows) raises ``ValueError``."""
    what = "gaussian_fit"
    fitted, st = _fit(what, evaluator, parents)
    if st & dl.STATUS_REFUSED:
        bad = torch.nonzero(torch.isnan(fitted.sd)).cpu().tolist()
        raise ValueError(f"{what}: refused families (structure, variable): {bad[:8]}: {_refused_families(fitted.n_vars)}")
    return fitted


# ---- what is done with a fitted network (include/dvs_gaussian_params.h) ---------------------------------------------
MALFORMED = ((dl.STATUS_CYCLE, "the structure has a cycle"),
             (dl.STATUS_REFUSED, "a parent bit lies at or above the number of variables"),
             (dl.STATUS_NOT_PROBABILITY, "an intercept, an sd or a coefficient at a parent bit is not finite, or an sd is not > 0"))
PREDICT_METHODS = dl.GBN_PREDICT_MODES
GCV_LOSSES = {"logl-g": None, "mse": "parents", "mse-exact": "exact"}      # loss -> gaussian_predict's method


def _network(what, fitted):
    """the checks every function here makes of its FittedGBN -> (n, B, device, the four tensors contiguous)"""
    if not isinstance(fitted, FittedGBN):
        raise ValueError(f"{what}: takes a FittedGBN (gaussian_fit, or FittedGBN(parents, coef, intercept, sd)), got "
                         f"{type(fitted).__name__}: a discrete network has sample, log_likelihood and predict")
    par, coef, icpt, sd = fitted.parents, fitted.coef, fitted.intercept, fitted.sd
    if not all(torch.is_tensor(t) for t in (par, coef, icpt, sd)):
        raise ValueError(f"{what}: the fields of a FittedGBN are torch tensors")
    dl.need_cuda(what, par.device)
    if par.dtype != torch.int64 or par.ndim != 2 or par.shape[0] < 1 or not 1 <= par.shape[1] <= dl.MAX_TOKENS:
        raise ValueError(f"{what}: parents must be int64 [B >= 1, n <= 48] parent masks")
    B, n = par.shape
    for name, t, shape in (("coef", coef, (B, n, n)), ("intercept", icpt, (B, n)), ("sd", sd, (B, n))):
        if t.dtype != torch.float64 or tuple(t.shape) != shape or t.device != par.device:
            raise ValueError(f"{what}: {name} must be float64 {list(shape)} on {par.device}")
    return n, B, par.device, (par.contiguous(), coef.contiguous(), icpt.contiguous(), sd.contiguous())


def _raise_malformed(what, st):
    said = [text for bit, text in MALFORMED if st & bit]
    if said:
        raise ValueError(f"{what}: {'; '.join(said)}")


def _rows(what, data, n, dev):
    """``data``: a GaussianEvaluator over n variables (its ``x``) or float64 / float32 rows [S >= 1, n] on the device -> f64, contiguous"""
    if not torch.is_tensor(data):
        if dl.data_kind(data) != "continuous" or not hasattr(data, "x"):
            raise ValueError(f"{what}: data must be a GaussianEvaluator or real-valued rows [S, {n}] on the device (a discrete "
                             f"evaluator's rows go to log_likelihood and predict)")
        if data.n_vars != n:
            raise ValueError(f"{what}: the evaluator has {data.n_vars} variables, the network {n}")
        data = data.x
    dl.need_cuda(what, data.device)
    if data.dtype not in (torch.float64, torch.float32) or data.ndim != 2 or data.shape[0] < 1 or data.shape[1] != n:
        raise ValueError(f"{what}: data must be a GaussianEvaluator or float64 / float32 rows [S >= 1, {n}]")
    return data.to(device=dev, dtype=torch.float64).contiguous()


def gaussian_joint(fitted: FittedGBN):
    """bnlearn's ``gbn2mvnorm``: the multivariate normal every network of ``fitted`` defines -> (mean f64 [B, n], cov f64
    [B, n, n]) on the device (dvs_gbn_joint).  A malformed network raises ``ValueError`` naming the rule."""
    what = "gaussian_joint"
    n, B, dev, net = _network(what, fitted)
    lib, p = dl.load(), dl.ptr
    with torch.cuda.device(dev):
        mean = torch.empty(B, n, dtype=torch.float64, device=dev)
        cov = torch.empty(B, n, n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_joint(B, n, *(p(t) for t in net), p(mean), p(cov), dl.nbytes(cov), p(status), dl.stream()),
                 "dvs_gbn_joint")
        _raise_malformed(what, int(status.item()))
    return mean, cov


def gaussian_sample(fitted: FittedGBN, n_rows: int, *, seed: int, row_offset: int = 0, index: int = 0) -> torch.Tensor:
    """bnlearn's ``rbn``: ``n_rows`` rows drawn by forward sampling from structure ``index`` of ``fitted`` -> float64
    [n_rows, n] on the device, what ``GaussianEvaluator.from_device`` takes.  Row i is a function of (seed, row_offset + i) and
    the network only, so a request may be cut into calls with consecutive ``row_offset`` and gives the same rows.  A malformed
    network raises ``ValueError`` naming the rule."""
    what = "gaussian_sample"
    n, B, dev, net = _network(what, fitted)
    if not 0 <= int(index) < B:
        raise ValueError(f"{what}: index must be in [0, {B})")
    if int(n_rows) < 1 or int(row_offset) < 0:
        raise ValueError(f"{what}: n_rows must be >= 1 and row_offset >= 0")
    lib, p = dl.load(), dl.ptr
    with torch.cuda.device(dev):
        ws_bytes = dl.workspace_bytes(lib, "dvs_gbn_sample_workspace_bytes", n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(int(n_rows), n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_sample(n, int(n_rows), *(p(t[index]) for t in net), dl.seed64(seed), int(row_offset), p(ws),
                                         ws_bytes, p(out), p(status), dl.stream()), "dvs_gbn_sample")
        _raise_malformed(what, int(status.item()))
    return out


def _malformed_batch(what, st, fitted):
    """dvs_gbn_loglik and dvs_gbn_predict report one bit for a malformed network whichever rule it breaks; dvs_gbn_joint
    checks the same three rules and says which, so the error names the rule and the structures"""
    if not st & dl.STATUS_REFUSED:
        return
    n, B, dev, net = _network(what, fitted)
    lib, p = dl.load(), dl.ptr
    mean = torch.empty(B, n, dtype=torch.float64, device=dev)
    cov = torch.empty(B, n, n, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    dl.check(lib, lib.dvs_gbn_joint(B, n, *(p(t) for t in net), p(mean), p(cov), dl.nbytes(cov), p(status), dl.stream()), "dvs_gbn_joint")
    bad = torch.nonzero(torch.isnan(mean[:, 0])).flatten().cpu().tolist()
    said = [text for bit, text in MALFORMED if int(status.item()) & bit]
    raise ValueError(f"{what}: malformed structures {bad[:8]}: {'; '.join(said)}")


def gaussian_log_likelihood(fitted: FittedGBN, data, *, per_row: bool = False):
    """bnlearn's ``logLik(fitted, newdata)`` for every structure of ``fitted``: ``data`` a ``GaussianEvaluator`` over the same
    variables (its rows) or float64 / float32 rows [S, n] on the device -> float64 [B] on the device, with ``per_row`` (total
    [B], row terms [B, S]) (dvs_gbn_loglik).  A NaN or infinite cell of the data propagates; a malformed network raises."""
    what = "gaussian_log_likelihood"
    n, B, dev, net = _network(what, fitted)
    x = _rows(what, data, n, dev)
    S, lib, p = x.shape[0], dl.load(), dl.ptr
    up = lambda v: (v + 255) & ~255
    ws_bytes = up(B * ((S + 255) // 256) * 8) + up(B * n * 4) + B * n * 8
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        rows = torch.empty(B, S, dtype=torch.float64, device=dev) if per_row else None
        out = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_loglik(B, n, S, p(x), *(p(t) for t in net), p(rows), p(out), p(ws), ws_bytes, p(status),
                                         dl.stream()), "dvs_gbn_loglik")
        _malformed_batch(what, int(status.item()), fitted)
    return (out, rows) if per_row else out


def gaussian_predict(fitted: FittedGBN, target: int, data, *, method: str = "parents", var: bool = False):
    """bnlearn's ``predict`` of variable ``target`` for every row of ``data`` (as for ``gaussian_log_likelihood``; the target's
    own column is not read) under every structure -> float64 [B, S], with ``var`` (predictions, the conditional variance f64
    [B]).  ``method="parents"``: the regression on the parents; ``"exact"``: the conditional mean given every other variable,
    closed-form over the Markov blanket (dvs_gbn_predict)."""
    what = "gaussian_predict"
    n, B, dev, net = _network(what, fitted)
    if method not in PREDICT_METHODS:
        raise ValueError(f"{what}: method must be one of {sorted(PREDICT_METHODS)} (got {method!r})")
    if not 0 <= int(target) < n:
        raise ValueError(f"{what}: target must be in [0, {n})")
    x = _rows(what, data, n, dev)
    S, lib, p = x.shape[0], dl.load(), dl.ptr
    ws_bytes = (B * 4 + 255) & ~255
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        pred = torch.empty(B, S, dtype=torch.float64, device=dev)
        cvar = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_gbn_predict(B, n, S, p(x), *(p(t) for t in net), int(target), PREDICT_METHODS[method], p(pred),
                                          p(cvar), p(ws), ws_bytes, p(status), dl.stream()), "dvs_gbn_predict")
        _malformed_batch(what, int(status.item()), fitted)
    return (pred, cvar) if var else pred


def gaussian_cross_validate(evaluator, parents, *, folds: int = 10, seed: int = 0, loss: str = "logl-g", target=None) -> torch.Tensor:
    """bnlearn's ``bn.cv`` for fixed structures on real-valued data: the rows are permuted (``params.cv_folds``), each part is
    held out in turn, the regressions are fitted on the rest and the part is scored -> float64 [B] on the device.

    ``loss="logl-g"``: minus the held-out log-likelihood per row (the parts' ``gaussian_log_likelihood`` added in fold order,
    divided by the number of rows).  ``"mse"`` / ``"mse-exact"``: the mean squared error of ``target`` predicted from its
    parents / from every other variable (``gaussian_predict``).  The training moments of all folds come from
    ``evaluator.with_rows`` (the parts differ by at most one row, so at most two views) and one ``gaussian_fit`` per view fits
    every structure on every fold; the result is, as bytes, the per-fold composition ``from_device(x[rest])`` + ``gaussian_fit``
    + ``gaussian_log_likelihood``.  A family ``gaussian_fit`` refuses on some fold raises its ``ValueError``, naming the fold."""
    from .params import cv_folds
    what = "gaussian_cross_validate"
    dl.need_unmixed(what, evaluator)
    if dl.data_kind(evaluator) != "continuous":
        raise ValueError(f"{what}: the evaluator holds discrete data: cross_validate is its counterpart")
    if not isinstance(evaluator, GaussianEvaluator):
        raise ValueError(f"{what}: takes the evaluator of a data set, not a row-set view")
    dl.need_cuda(what, evaluator.device)
    S, n, dev = evaluator.n_samples, evaluator.n_vars, evaluator.device
    if not 2 <= int(folds) <= S:
        raise ValueError(f"{what}: folds must be in [2, {S}]")
    if loss not in GCV_LOSSES:
        raise ValueError(f"{what}: loss must be one of {sorted(GCV_LOSSES)} (got {loss!r})")
    if (loss == "logl-g") != (target is None):
        raise ValueError(f"{what}: target is the argument of the prediction losses, and they need it")
    if target is not None and not 0 <= int(target) < n:
        raise ValueError(f"{what}: target must be in [0, {n})")
    if not torch.is_tensor(parents) or parents.dtype != torch.int64 or parents.ndim not in (1, 2) or parents.shape[-1] != n:
        raise ValueError(f"{what}: parents must be an int64 tensor [{n}] or [B, {n}] of parent masks")
    folds = int(folds)
    with torch.cuda.device(dev):
        parents = parents.reshape(-1, n).to(dev).contiguous()
        B = parents.shape[0]
        parts = [torch.from_numpy(p).to(dev) for p in cv_folds(S, folds, seed)]
        rests = [torch.cat([p for g, p in enumerate(parts) if g != f]) for f in range(folds)]
        fitted = [None] * folds
        for size in sorted({int(r.numel()) for r in rests}):
            mine = [f for f in range(folds) if rests[f].numel() == size]
            view = evaluator.with_rows(torch.stack([rests[f] for f in mine]).to(torch.int32),
                                       torch.arange(len(mine), dtype=torch.int32, device=dev).repeat_interleave(B))
            fit, st = _fit(what, view, parents.repeat(len(mine), 1))
            if st & dl.STATUS_REFUSED:
                bad = [(mine[b // B], b % B, v) for b, v in torch.nonzero(torch.isnan(fit.sd)).cpu().tolist()]
                raise ValueError(f"{what}: refused families (fold, structure, variable): {bad[:8]}: {_refused_families(n)}")
            for j, f in enumerate(mine):
                fitted[f] = FittedGBN(*(t[j * B:(j + 1) * B] for t in (fit.parents, fit.coef, fit.intercept, fit.sd)))
        total = None
        for f in range(folds):
            held = evaluator.x[parts[f]]
            if loss == "logl-g":
                term = gaussian_log_likelihood(fitted[f], held)
            else:
                err = gaussian_predict(fitted[f], int(target), held, method=GCV_LOSSES[loss]) - held[:, int(target)]
                term = (err * err).sum(dim=1)
            total = term if total is None else total + term
    return -total / S if loss == "logl-g" else total / S
