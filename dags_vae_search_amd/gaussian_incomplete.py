"""Gaussian networks on incomplete real-valued data (csrc/dvs_gaussian_incomplete.h).

A fitted Gaussian network defines one multivariate normal (``dvs_gbn_joint``).  ``dvs_gbn_condition`` conditions it on the observed
part of every row by one partial Cholesky factorisation per missingness pattern (include/dvs_gaussian_incomplete.h), and that one
call gives what the Gaussian side lacked next to the discrete ``infer.py`` / ``eliminate.py`` / ``incomplete.py``:

* ``gaussian_posterior``: the conditional mean and variance of some variables given partial evidence, the Gaussian ``exact_posterior``;
* ``gaussian_incomplete_log_likelihood``: the log-likelihood of rows with missing values;
* ``gaussian_impute``: bnlearn's ``impute`` on a Gaussian network by the exact conditional mean;
* ``expected_moments`` and ``gaussian_em_fit``: the E-step's expected moments in ``dvs_gbn_moments``'s layout, so that the M-step is
  ``dvs_gbn_fit`` and every search that reads a Gaussian evaluator's moments runs on ``ExpectedMoments.evaluator()`` unchanged.

Incomplete real data is a pair ``(x, observed)`` as in incomplete.py: ``x`` float64 [S, n] on the device and ``observed`` int64 [S],
bit v set where x[:, v] is observed (``incomplete_real_rows`` makes it from an array with NaNs).  An unobserved cell is never
read into arithmetic.

Not built: a structural-EM loop (``expected_moments`` + a search compose one step), batches of networks per call, likelihood
weighting / ``cpquery`` on intervals / ``mse-lw``, incomplete mixed data, and the joint conditional covariance per row (only its
diagonal per row and its sum over the rows are returned).  bnlearn parity is as recalled and unpinned against an R run.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib as dl
from .gaussian import (FittedGBN, GaussianMomentsEvaluator, _moments, _network, _raise_malformed, _refused_families)


def incomplete_real_rows(values, device="cuda"):
    """A real array [S, n <= 48] in which a NaN entry is missing -> ``(x, observed)`` on the device: float64 rows (a missing cell
    is stored as +0) and int64 [S] observed bits."""
    what = "incomplete_real_rows"
    dl.need_cuda(what, device)
    v = np.asarray(values)
    if v.ndim != 2 or v.shape[0] < 1 or not 1 <= v.shape[1] <= dl.MAX_TOKENS or v.dtype.kind != "f":
        raise ValueError(f"{what}: values must be a real array [S >= 1, n <= 48] (NaN: missing)")
    v = v.astype(np.float64)
    seen = ~np.isnan(v)
    observed = (seen.astype(np.uint64) << np.arange(v.shape[1], dtype=np.uint64)).sum(1, dtype=np.uint64)
    dev = torch.device(device)
    return torch.from_numpy(np.where(seen, v, 0.0)).to(dev), torch.from_numpy(observed.view(np.int64)).to(dev)


@dataclass
class GaussianConditioned:
    completed: torch.Tensor                # f64 [S, n]: observed cells as they are, missing ones at their conditional mean
    var: Optional[torch.Tensor]            # f64 [S, n]: 0 on observed cells, the conditional variance on missing ones (cov=True)
    quad: torch.Tensor                     # f64 [S]: the squared Mahalanobis distance of the observed part
    log_density: torch.Tensor              # f64 [S]: the log-density of the observed part
    log_likelihood: torch.Tensor           # f64 [1]: its sum (dvs_bn_loglik's order over the positions of the order used)
    cov_sum: Optional[torch.Tensor]        # f64 [n, n]: the conditional covariance summed over the rows (cov=True)
    refused: torch.Tensor                  # int64 [1]: rows refused (NaN in their cells): a singular observed block, a mask bit
                                           # at or above n, an observed cell that is not finite


def _one_network(what, fitted, index):
    """the checks of a FittedGBN and of ``index`` -> (n, device, the four tensors of network ``index`` as a batch of one)"""
    if not isinstance(fitted, FittedGBN):
        kind = type(fitted).__name__
        if kind == "FittedBN":
            raise ValueError(f"{what}: takes a FittedGBN, got a FittedBN: a discrete network's counterparts are exact_posterior, "
                             f"expected_counts, impute and em_fit")
        if kind == "FittedCGBN":
            raise ValueError(f"{what}: takes a FittedGBN, got a FittedCGBN: incomplete mixed data is not built (cg_predict "
                             f"conditions on complete rows)")
    n, B, dev, net = _network(what, fitted)
    if not 0 <= int(index) < B:
        raise ValueError(f"{what}: index must be in [0, {B})")
    return n, dev, tuple(t[int(index):int(index) + 1].contiguous() for t in net)


def _pair(what, data, n, dev):
    """``data`` = (x, observed) -> (x f64 [S, n], observed int64 [S]) contiguous on ``dev``"""
    if not (isinstance(data, tuple) and len(data) == 2):
        if not torch.is_tensor(data) and hasattr(data, "data_kind"):
            other = ("gaussian_log_likelihood and gaussian_predict take its complete rows" if dl.data_kind(data) == "continuous" else
                     "discrete data goes to expected_counts, impute and em_fit" if dl.data_kind(data) == "discrete" else
                     "incomplete mixed data is not built")
            raise ValueError(f"{what}: data must be (x, observed), as incomplete_real_rows gives it, not an evaluator: {other}")
        raise ValueError(f"{what}: data must be (x, observed), as incomplete_real_rows gives it")
    x, observed = data
    if not torch.is_tensor(x) or not torch.is_tensor(observed):
        raise ValueError(f"{what}: x and observed must be torch tensors (incomplete_real_rows makes them)")
    dl.require_cuda(x, f"{what}: x")
    dl.require_cuda(observed, f"{what}: observed")
    if x.dtype not in (torch.float64, torch.float32) or x.ndim != 2 or x.shape[0] < 1 or x.shape[1] != n:
        raise ValueError(f"{what}: x must be float64 / float32 [S >= 1, {n}] (integer level codes go to incomplete_rows and em_fit)")
    if observed.dtype != torch.int64 or observed.shape != (x.shape[0],):
        raise ValueError(f"{what}: observed must be int64 [{x.shape[0]}] bit rows")
    return x.to(device=dev, dtype=torch.float64).contiguous(), observed.to(dev).contiguous()


def _order(what, order, observed):
    """"sorted": the stable order of the masks (plumbing, on the device); None: the rows as they come; a tensor: checked here,
    once, to be a permutation, since the device does not check it"""
    S = observed.shape[0]
    if order is None:
        return None
    if isinstance(order, str):
        if order != "sorted":
            raise ValueError(f"{what}: order must be \"sorted\", None or a permutation of the rows (got {order!r})")
        return torch.sort(observed, stable=True).indices.to(torch.int32)
    if not torch.is_tensor(order) or order.dtype not in (torch.int32, torch.int64) or order.shape != (S,):
        raise ValueError(f"{what}: order must be \"sorted\", None or an integer tensor [{S}]")
    order = order.to(observed.device)
    if not bool((torch.sort(order).values == torch.arange(S, device=order.device, dtype=order.dtype)).all()):
        raise ValueError(f"{what}: order must be a permutation of the {S} rows")
    return order.to(torch.int32).contiguous()


def _joint(lib, n, net, dev):
    """dvs_gbn_joint of a batch of one -> (mean [n], cov [n, n], status [1]) with no read-back"""
    p = dl.ptr
    mean = torch.empty(1, n, dtype=torch.float64, device=dev)
    cov = torch.empty(1, n, n, dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    dl.check(lib, lib.dvs_gbn_joint(1, n, *(p(t) for t in net), p(mean), p(cov), dl.nbytes(cov), p(status), dl.stream()), "dvs_gbn_joint")
    return mean[0], cov[0], status


def _condition(lib, n, mean, cov, x, observed, order, *, completed=True, var=True, cov_sum=None, quad=True):
    """dvs_gbn_condition -> (GaussianConditioned, status [1]) with no read-back; ``cov_sum`` None: as ``var``"""
    S, dev, p = x.shape[0], x.device, dl.ptr
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    out = GaussianConditioned(f64(S, n) if completed else None, f64(S, n) if var else None, f64(S) if quad else None, f64(S), f64(1),
                              f64(n, n) if (var if cov_sum is None else cov_sum) else None, torch.empty(1, dtype=torch.int64, device=dev))
    ws_bytes = dl.workspace_bytes(lib, "dvs_gbn_condition_workspace_bytes", n, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    dl.check(lib, lib.dvs_gbn_condition(n, S, p(mean), p(cov), p(x), p(observed), p(order), p(out.completed), p(out.var), p(out.quad),
                                        p(out.log_density), p(out.log_likelihood), p(out.cov_sum), p(out.refused), p(ws), ws_bytes,
                                        p(status), dl.stream()), "dvs_gbn_condition")
    return out, status


def gaussian_condition(fitted: FittedGBN, data, index: int = 0, *, cov: bool = True, order="sorted") -> GaussianConditioned:
    """Network ``index`` of ``fitted`` conditioned on the observed part of every row of ``data`` = (x, observed): one
    ``dvs_gbn_joint`` and one ``dvs_gbn_condition``.  ``order="sorted"`` groups equal masks (``torch.sort(observed, stable=True)``)
    so that a pattern is factored once per 256 rows; None takes the rows as they come.  Per-row results do not depend on the
    order; ``log_likelihood`` and ``cov_sum`` are summed in it.  ``cov=False`` leaves ``var`` and ``cov_sum`` out (None) and lets
    the kernel skip the updates they alone need.  A refused row (see ``GaussianConditioned.refused``) has NaN in its cells and is
    counted, not raised.  A malformed network raises ``ValueError`` naming the rule."""
    return _conditioned("gaussian_condition", fitted, data, index, var=bool(cov), order=order)


def _conditioned(what, fitted, data, index, *, var, cov_sum=None, order="sorted", pair=_pair):
    """the body of gaussian_condition under the caller's name: the checks, one dvs_gbn_joint, one dvs_gbn_condition"""
    n, dev, net = _one_network(what, fitted, index)
    x, observed = pair(what, data, n, dev)
    lib = dl.load()
    with torch.cuda.device(dev):
        mean, joint_cov, jst = _joint(lib, n, net, dev)
        _raise_malformed(what, int(jst.item()))
        out, _ = _condition(lib, n, mean, joint_cov, x, observed, _order(what, order, observed), var=var, cov_sum=cov_sum)
    return out


def _evidence_rows(what, evidence, n, dev):
    if isinstance(evidence, dict):
        if not evidence:
            x = torch.zeros(1, n, dtype=torch.float64, device=dev)
            return x, torch.zeros(1, dtype=torch.int64, device=dev)
        row, mask = np.zeros((1, n)), 0
        for v, value in evidence.items():
            if not 0 <= int(v) < n:
                raise ValueError(f"{what}: evidence names variable {v!r}, the network has {n}")
            row[0, int(v)], mask = float(value), mask | (1 << int(v))
        return torch.from_numpy(row).to(dev), torch.tensor([mask], dtype=torch.int64, device=dev)
    return _pair(what, evidence, n, dev)


def gaussian_posterior(fitted: FittedGBN, targets, evidence, index: int = 0):
    """The Gaussian ``exact_posterior``: the conditional mean and variance of the variables ``targets`` given partial evidence,
    ``evidence`` a dict {variable: value} (one row) or an (x, observed) pair (a row each) -> (mean f64 [R, T], var f64 [R, T]) on
    the device.  A target that is itself observed has its value and variance 0.  Only the marginal variances are returned, not the
    joint covariance of several targets."""
    what = "gaussian_posterior"
    targets = [int(t) for t in ([targets] if isinstance(targets, int) else targets)]
    if isinstance(fitted, FittedGBN) and (not targets or any(not 0 <= t < fitted.n_vars for t in targets)):
        raise ValueError(f"{what}: targets must name variables in [0, {fitted.n_vars})")
    out = _conditioned(what, fitted, evidence, index, var=True, cov_sum=False, pair=_evidence_rows)
    dev = out.completed.device
    if int(out.refused.item()):
        bad = torch.nonzero(torch.isnan(out.log_density)).flatten().cpu().tolist()
        raise ValueError(f"{what}: refused evidence rows {bad[:8]}: {_REFUSED_ROWS}")
    idx = torch.tensor(targets, dtype=torch.int64, device=dev)
    return out.completed[:, idx], out.var[:, idx]


_REFUSED_ROWS = ("the observed variables are collinear under the network, a mask bit lies at or above the number of variables, or an "
                 "observed cell is not finite")


def gaussian_impute(fitted: FittedGBN, data, index: int = 0) -> torch.Tensor:
    """bnlearn's ``impute`` on a Gaussian network by the exact conditional mean -> float64 [S, n]: observed cells bit for bit,
    missing ones at their mean given the row's observed ones.  A refused row is NaN throughout (``gaussian_condition`` counts)."""
    return _conditioned("gaussian_impute", fitted, data, index, var=False).completed


def gaussian_incomplete_log_likelihood(fitted: FittedGBN, data, index: int = 0, per_row: bool = False):
    """The log-likelihood of rows with missing values under network ``index``: the log-density of every row's observed part,
    summed -> float64 [1] on the device, with ``per_row`` (total [1], row terms [S]).  A refused row counts 0 and has NaN in its
    term.  On complete rows this is ``gaussian_log_likelihood`` up to rounding (another factorisation of the same density)."""
    out = _conditioned("gaussian_incomplete_log_likelihood", fitted, data, index, var=False)
    return (out.log_likelihood, out.log_density) if per_row else out.log_likelihood


@dataclass
class ExpectedMoments:
    moments: torch.Tensor                  # f64 [1, 1 + n + n n]: dvs_gbn_moments's layout
    log_likelihood: torch.Tensor           # f64 [1]: of the incomplete data under the network the expectation was taken in
    refused: int                           # 0: a refused row raises

    def evaluator(self, metric_name: str = "bic-g", **score_args) -> GaussianMomentsEvaluator:
        """A Gaussian scorer over these moments: what hill_climb, tabu_search, exact_search, order_mcmc, arc_posterior and
        gaussian_fit take.  ``score_args``: ``k``, ``iss_mu``, ``iss_w`` as for ``GaussianEvaluator``."""
        return GaussianMomentsEvaluator("expected", metric_name, self.moments, **score_args)


def _expected(lib, n, net, x, observed, order, dev):
    """(moments, conditioned, joint status, condition status) with no read-back: dvs_gbn_moments of the completed rows, the summed
    conditional covariance added to the cross-product block by one elementwise add"""
    mean, cov, jst = _joint(lib, n, net, dev)
    out, cst = _condition(lib, n, mean, cov, x, observed, order, quad=False)
    moments = _moments(lib, out.completed, None)
    moments[0, 1 + n:] += out.cov_sum.reshape(-1)
    return moments, out, jst, cst


def expected_moments(fitted: FittedGBN, data, index: int = 0) -> ExpectedMoments:
    """The E-step: the expected sufficient statistics of the incomplete rows under network ``index``, in the layout
    ``dvs_gbn_moments`` writes: the moments of the completed rows, plus the summed conditional covariance in the cross-product
    block.  On complete data these are ``GaussianEvaluator.moments`` as bytes.  A refused row raises ``ValueError``."""
    what = "expected_moments"
    n, dev, net = _one_network(what, fitted, index)
    x, observed = _pair(what, data, n, dev)
    lib = dl.load()
    with torch.cuda.device(dev):
        moments, out, jst, _ = _expected(lib, n, net, x, observed, _order(what, "sorted", observed), dev)
        _raise_malformed(what, int(jst.item()))
        if int(out.refused.item()):
            bad = torch.nonzero(torch.isnan(out.log_density)).flatten().cpu().tolist()
            raise ValueError(f"{what}: refused rows {bad[:8]}: {_REFUSED_ROWS}")
    return ExpectedMoments(moments, out.log_likelihood, 0)


@dataclass
class GaussianEMResult:
    fitted: FittedGBN                      # the last M-step's parameters
    log_likelihood: List[float]            # entry t: of the incomplete data under the parameters after t M-steps
    iterations: int                        # E-steps done
    converged: bool


def _start(parents, x, observed, n):
    """zero coefficients; the intercept and sd of every column from its observed cells (a column no row observes: 0 and 1)"""
    seen = ((observed[:, None] >> torch.arange(n, device=x.device)) & 1).bool()
    cnt = seen.sum(0).double()
    safe = torch.clamp(cnt, min=1.0)
    mean = torch.where(seen, x, torch.zeros_like(x)).sum(0) / safe
    dev2 = torch.where(seen, (x - mean) ** 2, torch.zeros_like(x)).sum(0) / safe
    sd = torch.where(cnt > 0, torch.sqrt(dev2), torch.ones_like(dev2))
    return FittedGBN(parents, torch.zeros(1, n, n, dtype=torch.float64, device=x.device), mean[None].contiguous(), sd[None].contiguous())


def gaussian_em_fit(parents, data, *, start: Optional[FittedGBN] = None, variance: str = "mle", max_iter: int = 100,
                    tol: float = 1e-6) -> GaussianEMResult:
    """Parameter learning from incomplete real-valued data for ONE structure: EM with exact expected moments.  Every iteration
    runs ``expected_moments`` (the E-step) and ``dvs_gbn_fit`` on them (the M-step), and reads one packet back: the log-likelihood
    and the status words.

    ``parents`` n parent masks (ints or an int64 tensor [n]); ``data`` = (x, observed).  ``start``: a FittedGBN of this structure,
    or None for zero coefficients with the intercept and sd of every column taken from its observed cells.
    ``variance="mle"`` rescales ``dvs_gbn_fit``'s sd by sqrt((m - p - 1) / m): RSS / m is the true M-step, under which the
    log-likelihood of the incomplete data never falls beyond rounding; ``"unbiased"`` keeps ``gaussian_fit``'s RSS / (m - p - 1).
    It stops as the discrete ``em_fit`` does: when the log-likelihood changed by less than ``tol`` relative to its magnitude
    (``converged``), or after ``max_iter`` E-steps; the default ``tol`` = 1e-6 is that function's unmeasured choice.  A row the
    E-step refuses, and a family ``dvs_gbn_fit`` refuses (more than ``_lib.GBN_MAX_PARENTS`` parents, or collinear expected
    moments), raise ``ValueError``."""
    what = "gaussian_em_fit"
    if variance not in ("mle", "unbiased"):
        raise ValueError(f"{what}: variance must be \"mle\" or \"unbiased\" (got {variance!r})")
    if int(max_iter) < 1 or not float(tol) >= 0.0:
        raise ValueError(f"{what}: max_iter must be >= 1 and tol >= 0")
    host = [int(m) for m in (parents.reshape(-1).tolist() if torch.is_tensor(parents) else parents)]
    n = len(host)
    if not 1 <= n <= dl.MAX_TOKENS:
        raise ValueError(f"{what}: parents must hold one parent mask per variable of ONE structure (1 .. 48)")
    x, observed = _pair(what, data, n, data[0].device if isinstance(data, tuple) and len(data) == 2 and torch.is_tensor(data[0]) else None)
    dev = x.device
    ptensor = torch.tensor([host], dtype=torch.int64, device=dev)
    if start is None:
        fitted = _start(ptensor, x, observed, n)
    else:
        n0, _, net0 = _one_network(what, start, 0)
        low = (1 << n) - 1
        if start.batch != 1 or n0 != n or [int(m) & low & ~(1 << v) for v, m in enumerate(start.parents[0].tolist())] != \
                [m & low & ~(1 << v) for v, m in enumerate(host)]:
            raise ValueError(f"{what}: start must be a FittedGBN of this one structure")
        fitted = FittedGBN(ptensor, *net0[1:])
    lib, p = dl.load(), dl.ptr
    m = float(x.shape[0])
    low = (1 << n) - 1
    scale = torch.tensor([[math.sqrt(max(m - bin(pm & low & ~(1 << v)).count("1") - 1.0, 0.0) / m) for v, pm in enumerate(host)]],
                         dtype=torch.float64, device=dev)
    trace, converged = [], False
    with torch.cuda.device(dev):
        order = _order(what, "sorted", observed)
        for it in range(int(max_iter)):
            net = (fitted.parents, fitted.coef, fitted.intercept, fitted.sd)
            moments, out, jst, cst = _expected(lib, n, net, x, observed, order, dev)
            coef = torch.empty(1, n, n, dtype=torch.float64, device=dev)
            intercept = torch.empty(1, n, dtype=torch.float64, device=dev)
            sd = torch.empty(1, n, dtype=torch.float64, device=dev)
            fst = torch.zeros(1, dtype=torch.int32, device=dev)
            dl.check(lib, lib.dvs_gbn_fit(1, n, p(moments), 1, None, p(ptensor), p(coef), dl.nbytes(coef), p(intercept), p(sd), p(fst),
                                          dl.stream()), "dvs_gbn_fit")
            ll, refused, js, fs = torch.cat([out.log_likelihood, out.refused.double(), jst.double(), fst.double()]).tolist()
            _raise_malformed(f"{what} (iteration {it})", int(js))
            if int(refused):
                bad = torch.nonzero(torch.isnan(out.log_density)).flatten().cpu().tolist()
                raise ValueError(f"{what}: refused rows {bad[:8]} (iteration {it}): {_REFUSED_ROWS}")
            if int(fs) & dl.STATUS_REFUSED:
                bad = torch.nonzero(torch.isnan(sd)).cpu().tolist()
                raise ValueError(f"{what}: refused families (structure, variable): {bad[:8]} (iteration {it}): {_refused_families(n)}")
            trace.append(ll)
            fitted = FittedGBN(ptensor, coef, intercept, sd * scale if variance == "mle" else sd)
            if it and abs(trace[-1] - trace[-2]) <= float(tol) * abs(trace[-1]):
                converged = True
                break
    return GaussianEMResult(fitted, trace, len(trace), converged)
