"""Learning from incomplete data on the device (csrc/dvs_incomplete.h, include/dvs_incomplete.h): bnlearn's
``bn.fit`` on data with ``NA`` and ``impute``, on the exact inference of eliminate.py.

Incomplete data is what infer.py calls evidence: ``(rows, observed)`` — packed int64 rows [R, ceil(n / 16)] (or an evaluator)
and int64 [R] (or one int for all rows) whose bit v says that variable v is observed in that row; the nibble of an unobserved
variable is ignored.  ``incomplete_rows`` makes the pair from an integer array in which a negative entry is missing.

``expected_counts`` is the E-step: for every family the expected number of rows in every cell of its table, exactly — a row
whose family is wholly observed adds an integer, any other row the exact posterior of the family given what the row observes —
with P(observed part) of every row and the log-likelihood of the incomplete data.  ``fit_counts`` is the M-step, the arithmetic
of ``bn_fit`` on such counts.  ``em_fit`` alternates them.  ``impute`` fills every missing value with the most probable level
given the row's observed values (ties to the lowest level; bnlearn breaks them at random).

Structure learning on the same data: ``available_case_evaluator`` wraps the pair in the available-case scorer
(``BNLearnWrapper.available_case``: nal / pnal, which ``hill_climb`` and ``tabu_search`` take as they are), and
``structural_em`` is bnlearn's ``structural.em``: impute, maximise the structure on the completed rows, fit, repeated.

Everything is fp64 in the linear domain with stated summation orders: two runs give equal bytes.  The limits are those of
``elimination_plan``; here the arena and the family's cells share LDS, so ``arena_cells + out_cells`` must fit
``DVS_BN_ELIM_MAX_CELLS``.  Parity with bnlearn is unpinned against an R run.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from . import _lib as dl
from .eliminate import MAX_CELLS, EliminationPlan, plan_network
from .infer import _evidence
from .params import UNOBSERVED, FittedBN, _family, _offsets


def incomplete_rows(levels, device="cuda"):
    """An integer array [R, n] in which a negative entry is missing -> ``(rows, observed)`` on the device: packed int64 rows
    (the nibble of a missing value is 0) and int64 [R] observed bits."""
    dl.need_cuda("incomplete_rows", device)
    lv = np.asarray(levels)
    if lv.ndim != 2 or lv.shape[0] < 1 or not 1 <= lv.shape[1] <= dl.MAX_TOKENS or lv.dtype.kind not in "iu":
        raise ValueError("incomplete_rows: levels must be an integer array [R >= 1, n <= 48]")
    lv = lv.astype(np.int64)
    if (lv > 15).any():
        raise ValueError("incomplete_rows: a level is above 15")
    R, n = lv.shape
    seen = lv >= 0
    v = np.arange(n)
    rows = np.zeros((R, (n + 15) // 16), np.uint64)
    np.bitwise_or.at(rows, (np.arange(R)[:, None], (v // 16)[None, :]), (np.where(seen, lv, 0).astype(np.uint64) << (4 * (v % 16)).astype(np.uint64)))
    observed = (seen.astype(np.uint64) << v.astype(np.uint64)).sum(1, dtype=np.uint64)
    dev = torch.device(device)
    return torch.from_numpy(rows.view(np.int64)).to(dev), torch.from_numpy(observed.view(np.int64)).to(dev)


def check_cells(plans, what: str, targets: bool = False):
    """The arena and the last step's cells of one row share LDS: the largest arena plus the largest last step of ``plans`` (for
    the plans of ``impute``, ``targets``: plus the 16 levels a variable can have, as dvs_bn_impute counts) must fit the cap."""
    arena = max(p.arena_cells for p in plans)
    out = 16 if targets else max(p.out_cells for p in plans)
    if arena + out > MAX_CELLS:
        raise ValueError(f"{what}: an arena of {arena} cells and a last step of {out} cells need {arena + out} cells; the cap is "
                         f"{MAX_CELLS} fp64 cells of LDS and there is no global-memory fallback")


def plan_families(card, parents, targets: bool = False) -> List[EliminationPlan]:
    """The plans of one structure from host data alone (``plan_network`` for each): the n + 1 plans of ``expected_counts`` —
    plan v keeps the family of v, the last nothing — or, with ``targets``, the n plans of ``impute`` that keep {v}.  Raises
    ValueError when a plan is over the cap of ``elimination_plan`` or arena and last step together are."""
    card = dl.level_counts(card)
    n = len(card)
    rows = [int(m) for m in parents]
    keeps = [(v,) for v in range(n)] if targets else _keeps(rows, n)
    plans = [plan_network(card, rows, keep) for keep in keeps]
    check_cells(plans, "target_plans" if targets else "family_plans", targets)
    return plans


def _keeps(rows, n):
    return [tuple(u for u in range(n) if u == v or (rows[v] >> u) & 1) for v in range(n)] + [()]


def _plans(fitted, index, targets, plans, what) -> List[EliminationPlan]:
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"{what}: index must be in [0, {fitted.batch})")
    n = fitted.n_vars
    rows = [int(m) for m in fitted.parents_host[int(index)]]
    keeps = [(v,) for v in range(n)] if targets else _keeps(rows, n)
    if plans is None:
        plans = plan_families(fitted.card_host, rows, targets)
    parents = tuple(m & ~(1 << v) for v, m in enumerate(rows))
    if len(plans) != len(keeps) or any(not isinstance(p, EliminationPlan) or p.card != tuple(fitted.card_host) or p.parents != parents
                                       or p.keep != tuple(keep) for p, keep in zip(plans, keeps)):
        raise ValueError(f"{what}: plans must be the {len(keeps)} plans of this structure, from family_plans or target_plans")
    for p in plans:
        if p.words_device is None or p.words_device.device != fitted.device:
            p.words_device = torch.from_numpy(p.words).to(fitted.device)
    check_cells(plans, what, targets)
    return plans


def family_plans(fitted: FittedBN, index: int = 0) -> List[EliminationPlan]:
    """The n + 1 plans of ``expected_counts`` for structure ``index``, built once: plan v keeps the family of v, the last
    nothing.  They depend on the structure alone, not on the tables, so an EM loop reuses them."""
    return _plans(fitted, index, False, None, "family_plans")


def target_plans(fitted: FittedBN, index: int = 0) -> List[EliminationPlan]:
    """The n plans of ``impute``: plan v keeps {v}."""
    return _plans(fitted, index, True, None, "target_plans")


def _plan_args(plans, dev):
    words = torch.cat([p.words_device for p in plans])
    starts = torch.tensor(np.concatenate([[0], np.cumsum([len(p.words) for p in plans])]), dtype=torch.int64, device=dev)
    return words, starts, max(len(p.words) for p in plans), max(p.arena_cells for p in plans), max(p.max_step_cells for p in plans)


class ExpectedCounts:
    """The E-step's results on the device: ``counts`` float64 [n_cells] in the CPT layout of the structure (``table(v)``: the
    [q, r] view of family v), ``row_z`` float64 [R] = P(observed part of row r) (NaN for a row with a bad level or observed
    bit), ``log_likelihood`` float64 [1] = the sum of log row_z over the rows that count, ``skipped`` int64 [1] = the rows that
    do not (a bad level or bit, or row_z = 0), ``n_rows``, and the structure (``parents`` n ints, ``card``)."""

    def __init__(self, counts, row_z, log_likelihood, skipped, n_rows, parents, card):
        self.counts, self.row_z, self.log_likelihood, self.skipped, self.n_rows = counts, row_z, log_likelihood, skipped, n_rows
        self.parents, self.card = list(parents), list(card)
        self._offsets = _offsets(self.card, [self.parents])

    def table(self, v: int) -> torch.Tensor:
        q, r = _family(self.card, self.parents[v], v)
        return self.counts[self._offsets[v]:self._offsets[v] + q * r].view(q, r)


def _expected_counts(fitted, rows, observed, index, plans, rows_per_group, what):
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    R = rows.shape[0]
    lo, hi = fitted.offsets_host[index * n], fitted.offsets_host[(index + 1) * n]
    cells = hi - lo
    with torch.cuda.device(dev):
        words, starts, plan_words, arena, step = _plan_args(plans, dev)
        ws_bytes = dl.workspace_bytes(lib, "dvs_bn_expected_counts_workspace_bytes", cells, n, R)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(cells, dtype=torch.float64, device=dev)
        row_z = torch.empty(R, dtype=torch.float64, device=dev)
        loglik = torch.empty(1, dtype=torch.float64, device=dev)
        skipped = torch.empty(1, dtype=torch.int64, device=dev)
        flags = torch.empty(n + 1, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_expected_counts(n, R, p(fitted.card), p(fitted.parents[index]), p(fitted.offsets[index * n:]),
                                                 p(fitted.cpt), cells, p(words), dl.nbytes(words), p(starts), plan_words, arena,
                                                 max(pl.out_cells for pl in plans), step, p(rows), p(observed), int(rows_per_group),
                                                 p(counts), p(row_z), p(loglik), p(skipped), p(flags), p(ws), ws_bytes, p(status),
                                                 dl.stream()), "dvs_bn_expected_counts")
    parents = [int(m) for m in fitted.parents_host[index]]
    return ExpectedCounts(counts, row_z, loglik, skipped, R, parents, fitted.card_host), flags, status


def _data(fitted, data, what):
    if not (isinstance(data, tuple) and len(data) == 2):
        raise ValueError(f"{what}: data must be (rows, observed), as incomplete_rows gives it")
    rows, observed = _evidence(fitted, data, what)
    return rows.contiguous(), observed


def expected_counts(fitted: FittedBN, data, index: int = 0, *, plans=None, rows_per_group: int = 0) -> ExpectedCounts:
    """The E-step of EM under structure ``index`` of ``fitted`` on the incomplete ``data`` = (rows, observed) ->
    ``ExpectedCounts``.  ``plans``: the list of ``family_plans`` (built here when None).  A row with a bad level or observed bit
    raises ValueError; rows of probability zero are skipped and counted.  One status read-back."""
    what = "expected_counts"
    dl.need_cuda(what, fitted.device)
    rows, observed = _data(fitted, data, what)
    plans = _plans(fitted, index, False, plans, what)
    if not 0 <= int(rows_per_group) <= 64:
        raise ValueError(f"{what}: rows_per_group must be in [0, 64]")
    out, _, status = _expected_counts(fitted, rows, observed, int(index), plans, rows_per_group, what)
    if int(status.item()) & dl.STATUS_REFUSED:
        raise ValueError(f"{what}: a row has an observed level at or above its variable's level count or an observed bit at or "
                         f"above n_vars, a plan is malformed, or the tables do not match the structure")
    return out


def _fit_args(method, iss, unobserved):
    if method not in dl.FIT_METHODS:
        raise ValueError(f"method must be one of {sorted(dl.FIT_METHODS)} (got {method!r})")
    if unobserved not in UNOBSERVED:
        raise ValueError(f"unobserved must be one of {sorted(UNOBSERVED)} (got {unobserved!r})")
    if iss is not None and method != "bayes":
        raise ValueError("iss is the argument of method='bayes'")
    iss = 1.0 if iss is None else float(iss)
    if not (math.isfinite(iss) and iss > 0):
        raise ValueError(f"iss must be finite and > 0 (got {iss!r})")
    return dl.FIT_METHODS[method], iss, UNOBSERVED[unobserved]


def _fit_counts(counts, parents, card, offsets, method, iss, unobserved):
    n, dev, lib, p = len(card), counts.device, dl.load(), dl.ptr
    with torch.cuda.device(dev):
        cpt = torch.empty_like(counts)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_fit_counts(n, p(card), p(parents), p(offsets), p(counts), counts.numel(), method, iss, unobserved,
                                            p(cpt), p(status), dl.stream()), "dvs_bn_fit_counts")
    return cpt, status


def _structure_tensors(parents, card, dev):
    host = np.array([[int(m) for m in parents]], np.uint64)
    off = _offsets(card, host)
    return (torch.from_numpy(host.view(np.int64)).to(dev), torch.tensor(card, dtype=torch.uint8, device=dev),
            torch.tensor(off, dtype=torch.int64, device=dev), host, off)


def fit_counts(counts: ExpectedCounts, *, method: str = "mle", iss=None, unobserved: str = "nan") -> FittedBN:
    """The M-step: the tables of the structure of ``counts`` from its expected counts, with the arithmetic and the arguments of
    ``bn_fit`` (on integer counts: its bytes).  A family with a negative or non-finite count raises ValueError."""
    if not isinstance(counts, ExpectedCounts):
        raise ValueError("fit_counts: counts must be the ExpectedCounts of expected_counts")
    dl.need_cuda("fit_counts", counts.counts.device)
    method, iss, unobserved = _fit_args(method, iss, unobserved)
    parents, card, offsets, host, off = _structure_tensors(counts.parents, counts.card, counts.counts.device)
    cpt, status = _fit_counts(counts.counts.contiguous(), parents, card, offsets, method, iss, unobserved)
    if int(status.item()) & dl.STATUS_REFUSED:
        raise ValueError("fit_counts: a family holds a negative or non-finite count, or the counts do not match the structure")
    return FittedBN(parents, card, offsets, cpt, host, counts.card, off)


class EMResult:
    """``fitted`` (the last M-step's tables), ``log_likelihood`` (a list: the log-likelihood of the incomplete data under the
    tables each E-step saw, so entry t belongs to the tables after t M-steps), ``iterations`` (E-steps done), ``converged`` and
    ``skipped`` (the rows the last E-step left out: probability zero under its tables)."""

    def __init__(self, fitted, log_likelihood, iterations, converged, skipped):
        self.fitted, self.log_likelihood, self.iterations, self.converged, self.skipped = fitted, log_likelihood, iterations, converged, skipped


def em_fit(parents, card, data, *, start: Optional[FittedBN] = None, method: str = "mle", iss=None, max_iter: int = 100,
           tol: float = 1e-6, unobserved: str = "uniform") -> EMResult:
    """Parameter learning from incomplete data for ONE structure: **soft EM with exact expected counts** (the E-step is
    ``expected_counts``, the M-step ``fit_counts``).  bnlearn's ``hard-em`` is impute-then-fit instead, which ``impute`` +
    ``BNLearnWrapper.from_packed`` + ``bn_fit`` compose.

    ``parents`` n parent rows (ints or an int64 tensor [n]), ``card`` n level counts, ``data`` = (rows, observed).  ``start``: a
    FittedBN of this structure, or None for uniform tables.  The plans are built once.  After every E-step one scalar is read
    back: the iteration stops when the log-likelihood changed by less than ``tol`` relative to its magnitude (``converged``), or
    after ``max_iter`` E-steps.  The default ``tol`` = 1e-6 is an unmeasured choice.  With ``method="mle"`` the log-likelihood
    never falls beyond rounding; ``unobserved="uniform"`` (the default here, unlike ``bn_fit``) keeps a configuration no row
    supports usable in the next E-step."""
    what = "em_fit"
    if not (isinstance(data, tuple) and len(data) == 2):
        raise ValueError(f"{what}: data must be (rows, observed), as incomplete_rows gives it")
    dev = data[0].packed.device if hasattr(data[0], "packed") else data[0].device if torch.is_tensor(data[0]) else None
    if dev is None:
        raise ValueError(f"{what}: the rows of data must be an evaluator or a packed int64 tensor")
    dl.need_cuda(what, dev)
    code, iss_value, unobs = _fit_args(method, iss, unobserved)
    card = dl.level_counts(card)
    rows_host = [int(m) for m in (parents.tolist() if torch.is_tensor(parents) else parents)]
    if len(rows_host) != len(card):
        raise ValueError(f"{what}: parents must hold one parent row per variable ({len(card)})")
    if int(max_iter) < 1 or not float(tol) >= 0.0:
        raise ValueError(f"{what}: max_iter must be >= 1 and tol >= 0")
    ptensor, ctensor, offsets, host, off = _structure_tensors(rows_host, card, dev)
    if start is None:
        cpt = torch.cat([torch.full((off[v + 1] - off[v],), 1.0 / card[v], dtype=torch.float64, device=dev) for v in range(len(card))])
        fitted = FittedBN(ptensor, ctensor, offsets, cpt, host, card, off)
    else:
        if (not isinstance(start, FittedBN) or start.batch != 1 or list(start.card_host) != card
                or [int(m) & ~(1 << v) for v, m in enumerate(start.parents_host[0])] != [m & ~(1 << v) for v, m in enumerate(rows_host)]):
            raise ValueError(f"{what}: start must be a FittedBN of this one structure")
        fitted = start
    rows, observed = _data(fitted, data, what)
    plans = family_plans(fitted)
    trace, converged, skipped = [], False, 0
    for it in range(int(max_iter)):
        ec, _, status = _expected_counts(fitted, rows, observed, 0, plans, 0, what)
        cpt, fit_status = _fit_counts(ec.counts, ptensor, ctensor, offsets, code, iss_value, unobs)
        ll, st, fst, skipped = (float(x) for x in torch.cat([ec.log_likelihood, status.double(), fit_status.double(), ec.skipped.double()]).tolist())
        if (int(st) | int(fst)) & dl.STATUS_REFUSED:
            raise ValueError(f"{what}: a row has a bad observed level or bit, the tables do not match the structure, or the counts "
                             f"are not finite (iteration {it})")
        trace.append(ll)
        fitted = FittedBN(ptensor, ctensor, offsets, cpt, host, card, off)
        if it and abs(trace[-1] - trace[-2]) <= float(tol) * abs(trace[-1]):
            converged = True
            break
    return EMResult(fitted, trace, len(trace), converged, int(skipped))


def impute(fitted: FittedBN, data, index: int = 0, *, plans=None):
    """bnlearn's ``impute`` by exact inference: every missing value of ``data`` = (rows, observed) becomes the most probable
    level given the row's observed values under structure ``index`` (the lowest level among equals) -> ``(rows, observed_out)``
    on the device.  A value stays missing (nibble 0, bit clear in ``observed_out``) where the row's evidence has probability
    zero.  ``plans``: the list of ``target_plans``.  A row with a bad level or observed bit raises ValueError."""
    what = "impute"
    dl.need_cuda(what, fitted.device)
    rows, observed = _data(fitted, data, what)
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    plans = _plans(fitted, index, True, plans, what)
    index, R = int(index), rows.shape[0]
    lo, hi = fitted.offsets_host[index * n], fitted.offsets_host[(index + 1) * n]
    with torch.cuda.device(dev):
        words, starts, plan_words, arena, step = _plan_args(plans, dev)
        ws_bytes = dl.workspace_bytes(lib, "dvs_bn_impute_workspace_bytes", n, R)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty_like(rows)
        seen = torch.empty(R, dtype=torch.int64, device=dev)
        flags = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_impute(n, R, p(fitted.card), p(fitted.parents[index]), p(fitted.offsets[index * n:]), p(fitted.cpt),
                                        hi - lo, p(words), dl.nbytes(words), p(starts), plan_words, arena, step, p(rows), p(observed),
                                        0, p(out), p(seen), p(flags), p(ws), ws_bytes, p(status), dl.stream()), "dvs_bn_impute")
        if int(status.item()) & dl.STATUS_REFUSED:
            raise ValueError(f"{what}: a row has an observed level at or above its variable's level count or an observed bit at or "
                             f"above n_vars, a plan is malformed, or the tables do not match the structure")
    return out, seen


def available_case_evaluator(data, card, metric: str = "pnal", k=None, name: str = "incomplete"):
    """The ``(rows, observed)`` pair of ``incomplete_rows`` as an available-case evaluator (``AvailableCaseEvaluator``, bic.py):
    every family is scored on exactly the rows that observe it whole.  ``metric`` "nal" or "pnal" with the penalty coefficient
    ``k`` (default ``n_samples ** -0.25``; parity with bnlearn's pnal is unpinned against an R run).  ``hill_climb`` and
    ``tabu_search`` take the result as they take any evaluator."""
    from .bic import BNLearnWrapper
    if not (isinstance(data, tuple) and len(data) == 2 and torch.is_tensor(data[0]) and torch.is_tensor(data[1])):
        raise ValueError("available_case_evaluator: data must be (rows, observed) tensors, as incomplete_rows gives them")
    return BNLearnWrapper.from_packed(name, "loglik", data[0], card).available_case(data[1], metric, k)


@dataclass
class StructuralEMResult:
    parents: torch.Tensor          # int64 [n] on the device: the last iteration's parent masks
    fitted: FittedBN               # its tables
    iterations: int                # iterations done
    converged: bool                # the last iteration's masks equal the one before's
    trace: list                    # per iteration: dict(parents=[n ints], score, left_out, log_likelihood)


def structural_em(data, card, *, start=None, maximize: str = "hc", maximize_args=None, score: str = "bic", score_args=None,
                  fit: str = "bayes", iss=None, refit: str = "completed", max_iter: int = 5, max_parents: Optional[int] = 3) -> StructuralEMResult:
    """bnlearn's ``structural.em`` as a composition of what the package has: from the empty graph (or the parent masks
    ``start``), whose tables come from ``em_fit``, every iteration runs ``impute`` with the current network, builds
    ``BNLearnWrapper.from_packed("completed", score, completed rows, card, **score_args)``, runs ``hill_climb`` (``maximize="hc"``) or
    ``tabu_search`` ("tabu") from the current structure with ``max_parents`` and ``maximize_args`` (``max_steps`` defaults to
    max(16, n^2)), and fits the new structure: ``bn_fit`` on the completed rows (``refit="completed"``, bnlearn's way) or
    ``em_fit`` on the incomplete rows (``refit="em"``), with ``fit`` ("bayes" or "mle"; an unobserved configuration is uniform)
    and ``iss``.  A row in which ``impute`` leaves a value missing is left out of that iteration's completed rows and counted.
    It stops when the parent masks equal the previous iteration's (``converged``) or after ``max_iter`` iterations.

    ``trace`` holds per iteration the parent masks, the search's score, the rows left out and the log-likelihood of the
    incomplete data under the new network.  This is hard EM: none of them need be monotone.  The defaults ``max_iter=5``
    (bnlearn's), ``fit="bayes"`` (no table zero leaves a value unimputable) and ``max_parents=3`` (the plans stay within the
    16 384-cell cap) are unmeasured choices.  A structure whose plans exceed the cap raises the ValueError of ``check_cells``
    with the iteration number (0: the start) in front."""
    from .bic import BNLearnWrapper
    from .hillclimb import hill_climb
    from .params import bn_fit
    from .tabu import tabu_search
    what = "structural_em"
    if maximize not in ("hc", "tabu"):
        raise ValueError(f"{what}: maximize must be 'hc' or 'tabu' (got {maximize!r})")
    if refit not in ("completed", "em"):
        raise ValueError(f"{what}: refit must be 'completed' or 'em' (got {refit!r})")
    if fit not in dl.FIT_METHODS:
        raise ValueError(f"{what}: fit must be one of {sorted(dl.FIT_METHODS)} (got {fit!r})")
    if int(max_iter) < 1:
        raise ValueError(f"{what}: max_iter must be >= 1")
    if not (isinstance(data, tuple) and len(data) == 2 and torch.is_tensor(data[0]) and torch.is_tensor(data[1])):
        raise ValueError(f"{what}: data must be (rows, observed) tensors, as incomplete_rows gives them")
    card = dl.level_counts(card)
    n, dev = len(card), data[0].device
    dl.need_cuda(what, dev)
    if start is None:
        current = [0] * n
    else:
        current = [int(m) & ~(1 << v) for v, m in enumerate(start.reshape(-1).tolist() if torch.is_tensor(start) else start)]
        if len(current) != n:
            raise ValueError(f"{what}: start must hold one parent row per variable ({n})")
    search = hill_climb if maximize == "hc" else tabu_search
    search_args = {"max_steps": max(16, n * n), **(maximize_args or {})}
    full = (1 << n) - 1

    def at_iteration(it, fn, *args, **kw):
        try:
            return fn(*args, **kw)
        except ValueError as e:
            raise ValueError(f"{what}: iteration {it}: {e}") from e

    fitted = at_iteration(0, em_fit, current, card, data, method=fit, iss=iss).fitted
    trace, converged = [], False
    for it in range(1, int(max_iter) + 1):
        rows, seen = at_iteration(it, impute, fitted, data)
        whole = (seen & full) == full
        left_out = int(whole.numel() - int(whole.sum()))
        if left_out == whole.numel():
            raise ValueError(f"{what}: iteration {it}: impute left a value missing in every row")
        completed = rows[whole].contiguous() if left_out else rows
        ev = BNLearnWrapper.from_packed("completed", score, completed, card, **(score_args or {}))
        starts = torch.tensor([current], dtype=torch.int64, device=dev)
        found = at_iteration(it, search, ev, starts, max_parents=max_parents, **search_args)
        new = [int(m) for m in found.parents[0].tolist()]
        if refit == "completed":
            fitted = at_iteration(it, bn_fit, ev, found.parents[0], method=fit, iss=iss, unobserved="uniform")
        else:
            fitted = at_iteration(it, em_fit, new, card, data, method=fit, iss=iss).fitted
        ll = float(at_iteration(it, expected_counts, fitted, data).log_likelihood.item())
        trace.append(dict(parents=new, score=float(found.scores[0].item()), left_out=left_out, log_likelihood=ll))
        converged = new == current
        current = new
        if converged:
            break
    return StructuralEMResult(torch.tensor(current, dtype=torch.int64, device=dev), fitted, len(trace), converged, trace)
