"""Exact inference on a fitted discrete Bayesian network by bucket (variable) elimination on the device
(csrc/dvs_eliminate.h, include/dvs_eliminate.h): the exact yardstick next to the likelihood weighting of
infer.py, as ``exact_search`` stands next to ``hill_climb``.  gRain's ``querygrain`` is the bnlearn user's counterpart.

``evidence_probability`` is P(evidence [and event]) — the likelihood of a row with missing values; ``exact_cpquery`` is
``cpquery`` without particles; ``exact_posterior`` has the layout of ``posterior``; ``exact_joint`` is the joint posterior of a
few variables.  Evidence and events are given as in infer.py.  The results are fp64 in the linear domain, deterministic to the
byte: a probability of the evidence below the range of fp64 underflows to 0 and the posteriors are then NaN (a log-domain
variant does not exist).

The plan is built here on the host and executed by the kernel.  The factors are the n tables; a variable outside ``keep`` is
eliminated by multiplying every live factor that holds it and summing it out, which leaves a factor over the union of the
scopes; what is left is multiplied into the output over ``keep``.  Intermediate factors live in an arena of fp64 cells in LDS.
The order is greedy (fewest fill-in edges, then smallest result, then lowest index): a heuristic, not the optimal order.

The limit is honest rather than hidden: the arena and every table must fit ``DVS_BN_ELIM_MAX_CELLS`` = 16 384 fp64 cells
(128 KiB of LDS), and there is no global-memory fallback.  Narrow networks fit easily (asia: 8 cells; a 48-variable network
whose parents lie within a window of 6: a few hundred).  Dense ones do not: a CPU prototype of this heuristic on random
37-variable DAGs with up to 3 parents per variable needed 55 296 to 110 592 cells in two of four draws.  ``elimination_plan``
raises ValueError for those, naming the width and the cells needed.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as dl
from .infer import _event_words, _evidence, _mask_of
from .params import FittedBN

MAX_CELLS = dl.ELIM_MAX_CELLS


class EliminationPlan:
    """One elimination plan of one structure: ``order`` (the eliminated variables in turn), ``keep`` (ascending), ``width`` (the
    most variables one step multiplies over, the eliminated one included), ``max_step_cells`` (the largest step output),
    ``arena_cells``, ``out_cells`` (the product of the kept variables' level counts), ``depth`` (the roundings behind an output
    cell: a table cell has 0, a step output the largest depth of its inputs + (inputs - 1) + (levels summed - 1)), ``z_depth``
    (depth + ceil(out_cells / 256) - 1 + 8: the fixed tree of z), ``steps`` (one dict per step), ``words`` (the int32 plan words
    of include/dvs_eliminate.h on the host) and ``words_device`` (the same on the device; None for a plan made on the host
    alone)."""

    def __init__(self, card, parents, keep, order, steps, arena_cells, words):
        self.card, self.parents, self.keep, self.order, self.steps = tuple(card), tuple(parents), tuple(keep), list(order), steps
        self.n_vars = len(card)
        self.arena_cells = int(arena_cells)
        self.width = max(len(s["scope"]) + (s["x"] >= 0) for s in steps)
        self.max_step_cells = max(s["cells"] for s in steps)
        self.out_cells = steps[-1]["cells"]
        self.depth = steps[-1]["depth"]
        self.z_depth = self.depth + (self.out_cells + 255) // 256 - 1 + 8
        self.words = words
        self.words_device = None


def _first_fit(spans, cells):
    """the lowest offset at which ``cells`` cells lie clear of the (offset, cells) spans in use"""
    at = 0
    for lo, size in sorted(spans):
        if lo - at >= cells:
            break
        at = max(at, lo + size)
    return at


def _greedy_order(card, scopes, keep):
    """fewest fill-in edges first, then the smallest result table, then the lowest index"""
    n = len(card)
    adj = [0] * n
    for scope in scopes:
        for v in scope:
            adj[v] |= sum(1 << u for u in scope if u != v)
    left = [v for v in range(n) if v not in keep]
    order = []
    while left:
        best = None
        for x in left:
            nb = [u for u in range(n) if (adj[x] >> u) & 1]
            fill = sum(1 for i, u in enumerate(nb) for t in nb[i + 1:] if not (adj[u] >> t) & 1)
            key = (fill, math.prod(card[u] for u in nb), x)
            if best is None or key < best:
                best = key
        x = best[2]
        nb = adj[x]
        for u in range(n):
            if (nb >> u) & 1:
                adj[u] = (adj[u] | nb) & ~(1 << u) & ~(1 << x)
        adj[x] = 0
        left.remove(x)
        order.append(x)
    return order


def plan_network(card, parents, keep=(), order=None, max_cells=None) -> EliminationPlan:
    """The plan of one structure from host data alone: ``card`` n level counts, ``parents`` n parent rows (bit u of row v <=>
    u -> v).  ``elimination_plan`` is this for a FittedBN, with the words on the device as well."""
    what = "elimination_plan"
    card = dl.level_counts(card)
    n = len(card)
    parents = [int(m) & ~(1 << v) for v, m in enumerate(parents)]
    if len(parents) != n or any(m >> n for m in parents):
        raise ValueError(f"{what}: parents must hold {n} parent rows over the variables 0..{n - 1}")
    max_cells = MAX_CELLS if max_cells is None else int(max_cells)
    if not 1 <= max_cells <= MAX_CELLS:
        raise ValueError(f"{what}: max_cells must be in [1, DVS_BN_ELIM_MAX_CELLS = {MAX_CELLS}]")
    keep = sorted({int(v) for v in keep})
    if any(not 0 <= v < n for v in keep):
        raise ValueError(f"{what}: keep names a variable outside [0, {n})")
    # the live factors in plan order: the tables in ascending id, then the intermediates as they are made
    live = []
    for v in range(n):
        strides, stride = {v: 1}, card[v]
        for u in range(n):
            if (parents[v] >> u) & 1:
                strides[u] = stride
                stride *= card[u]
        live.append(dict(kind=v, offset=0, cells=stride, strides=strides, depth=0))
    if order is None:
        order = _greedy_order(card, [sorted(f["strides"]) for f in live], keep)
    else:
        order = [int(v) for v in order]
        if sorted(order) != [v for v in range(n) if v not in keep]:
            raise ValueError(f"{what}: order must be a permutation of the variables that are not kept")
    steps, in_use, arena_cells = [], [], 0
    for x in order + [-1]:
        ins = [f for f in live if x in f["strides"]] if x >= 0 else list(live)
        scope = sorted(set().union(*(f["strides"] for f in ins)) - {x}) if x >= 0 else keep
        cells = math.prod(card[v] for v in scope)
        summed = card[x] if x >= 0 else 1
        depth = max(f["depth"] for f in ins) + len(ins) - 1 + summed - 1
        offset = -1
        if x >= 0:
            offset = _first_fit(in_use, cells)               # before the inputs are freed: the output never overlaps them
            in_use.append((offset, cells))
            arena_cells = max(arena_cells, offset + cells)
            for f in ins:
                if f["kind"] < 0:
                    in_use.remove((f["offset"], f["cells"]))
        steps.append(dict(x=x, offset=offset, cells=cells, scope=scope, inputs=ins, depth=depth))
        live = [f for f in live if not any(f is g for g in ins)]
        strides, stride = {}, 1
        for v in scope:
            strides[v] = stride
            stride *= card[v]
        live.append(dict(kind=-1, offset=offset, cells=cells, strides=strides, depth=depth))
    arena_cells = max(arena_cells, 1)
    width = max(len(s["scope"]) + (s["x"] >= 0) for s in steps)
    largest = max(max(s["cells"] for s in steps), max(f["cells"] for s in steps for f in s["inputs"]))
    if largest > max_cells or arena_cells > max_cells:
        raise ValueError(f"{what}: elimination of width {width} needs a table of {largest} cells and an arena of {arena_cells} "
                         f"cells; the cap is {max_cells} fp64 cells of LDS and there is no global-memory fallback")
    if max(len(s["scope"]) for s in steps) > dl.ELIM_MAX_SCOPE:
        raise ValueError(f"{what}: elimination of width {width} has a scope of more than {dl.ELIM_MAX_SCOPE} variables")
    words = [dl.ELIM_TAG, n, len(steps), arena_cells, steps[-1]["cells"], len(keep), *keep]
    for s in steps:
        words += [s["x"], s["offset"], s["cells"], len(s["scope"]), len(s["inputs"]), *s["scope"]]
        for f in s["inputs"]:
            words += [f["kind"], f["offset"], f["cells"], f["strides"].get(s["x"], 0), *(f["strides"].get(v, 0) for v in s["scope"])]
    if len(words) > dl.ELIM_MAX_WORDS:
        raise ValueError(f"{what}: the plan has {len(words)} words; DVS_BN_ELIM_MAX_WORDS is {dl.ELIM_MAX_WORDS}")
    return EliminationPlan(card, parents, keep, order, steps, arena_cells, np.asarray(words, np.int32))


def elimination_plan(fitted: FittedBN, keep=(), index: int = 0, order=None, max_cells=None) -> EliminationPlan:
    """The elimination plan of structure ``index`` of ``fitted`` with the variables of ``keep`` left in the output (lowest id
    fastest).  ``order`` (a permutation of the variables that are not kept) overrides the greedy order.  Raises ValueError when
    the arena or a table exceeds ``max_cells`` (default and upper limit: DVS_BN_ELIM_MAX_CELLS = 16 384 fp64 cells, 128 KiB of
    LDS; there is no global-memory fallback — dense networks such as random 37-variable DAGs with up to 3 parents per variable
    can need 55 296 to 110 592 cells and are refused): the message names the width and the cells needed."""
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"elimination_plan: index must be in [0, {fitted.batch})")
    plan = plan_network(fitted.card_host, [int(m) for m in fitted.parents_host[int(index)]], keep, order, max_cells)
    plan.words_device = torch.from_numpy(plan.words).to(fitted.device)
    return plan


def _plan_for(fitted, keep, index, plan, what):
    if plan is None:
        return elimination_plan(fitted, keep, index)
    if (not isinstance(plan, EliminationPlan) or plan.card != tuple(fitted.card_host) or plan.keep != tuple(sorted({int(v) for v in keep}))
            or plan.parents != tuple(int(m) & ~(1 << v) for v, m in enumerate(fitted.parents_host[int(index)]))):
        raise ValueError(f"{what}: plan must be an EliminationPlan of this structure that keeps {sorted(keep)}")
    if plan.words_device is None or plan.words_device.device != fitted.device:
        plan.words_device = torch.from_numpy(plan.words).to(fitted.device)
    return plan


def level_masks(fitted: FittedBN, rows, observed, event=None, what="exact inference") -> torch.Tensor:
    """The u16 level masks of dvs_bn_eliminate (stored as int16 [Q, n] on the device): bit k of [q, v] <=> level k of variable v
    is allowed in query q.  An observed variable has the one bit of its level, an unconstrained one 0xFFFF; ``event`` (the
    words of infer.py, int16 [n]) is and-ed in.  An observed level at or above its variable's level count is a ValueError."""
    n, dev = fitted.n_vars, fitted.device
    v = torch.arange(n, device=dev)
    levels = (rows[:, v // 16] >> (4 * (v % 16))) & 15                           # int64 [Q, n]
    seen = ((observed[:, None] >> v) & 1).bool()
    if n < 63 and bool(((observed >> n) != 0).any()):
        raise ValueError(f"{what}: observed has a bit at or above n_vars = {n}")
    if bool((seen & (levels >= fitted.card.to(torch.int64))).any()):
        raise ValueError(f"{what}: an evidence level is at or above its variable's level count, or the tables do not match the structure")
    masks = torch.where(seen, torch.ones_like(levels) << levels, torch.full_like(levels, 0xFFFF))
    if event is not None:
        masks = masks & (event.to(torch.int64) & 0xFFFF)
    return ((masks + 32768) % 65536 - 32768).to(torch.int16).contiguous()


def run_plans(fitted: FittedBN, plans, masks, *, index: int = 0, rows_per_group: int = 0, out_stride=None, what="exact inference"):
    """one dvs_bn_eliminate: every plan over every mask row -> (out f64 [P, R, out_stride] the unnormalised cells, z f64 [P, R]
    their sums), on the device.  A plan or a network the device refuses raises ValueError."""
    dl.need_cuda(what, fitted.device)
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    P, R = len(plans), masks.shape[0]
    stride = max(pl.out_cells for pl in plans) if out_stride is None else int(out_stride)
    lo, hi = fitted.offsets_host[index * n], fitted.offsets_host[(index + 1) * n]
    with torch.cuda.device(dev):
        words = plans[0].words_device if P == 1 else torch.cat([pl.words_device for pl in plans])
        starts = torch.tensor(np.concatenate([[0], np.cumsum([len(pl.words) for pl in plans])]), dtype=torch.int64, device=dev)
        out = torch.empty(P, R, stride, dtype=torch.float64, device=dev)
        z = torch.empty(P, R, dtype=torch.float64, device=dev)
        flags = torch.empty(P, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_eliminate(n, P, R, p(fitted.card), p(fitted.parents[index]), p(fitted.offsets[index * n:]),
                                           p(fitted.cpt), hi - lo, p(words), dl.nbytes(words), p(starts),
                                           max(len(pl.words) for pl in plans), max(pl.arena_cells for pl in plans),
                                           max(pl.max_step_cells for pl in plans), p(masks), int(rows_per_group), stride, p(out),
                                           dl.nbytes(out), p(z), p(flags), p(status), dl.stream()), "dvs_bn_eliminate")
        if int(status.item()) & dl.STATUS_REFUSED:
            raise ValueError(f"{what}: a plan is malformed, or the tables do not match the structure")
    return out, z


def _query(fitted, evidence, event, index, what):
    dl.need_cuda(what, fitted.device)
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"{what}: index must be in [0, {fitted.batch})")
    rows, observed = _evidence(fitted, evidence, what)
    return rows, observed, _event_words(fitted, event, what)


def evidence_probability(fitted: FittedBN, evidence, event=None, index: int = 0, *, plan=None) -> torch.Tensor:
    """P(evidence) — with ``event``, P(evidence and event) — under structure ``index`` -> float64 [Q] on the device, exact up
    to rounding: the likelihood of a row with missing values.  Evidence and event as in ``cpquery``."""
    what = "evidence_probability"
    rows, observed, words = _query(fitted, evidence, event, index, what)
    plan = _plan_for(fitted, (), index, plan, what)
    _, z = run_plans(fitted, [plan], level_masks(fitted, rows, observed, words, what), index=index, what=what)
    return z[0]


def exact_cpquery(fitted: FittedBN, event, evidence, index: int = 0, *, plan=None) -> torch.Tensor:
    """``cpquery`` without particles: P(event | evidence) = Z(event and evidence) / Z(evidence) -> float64 [Q] on the device,
    NaN where P(evidence) = 0.  One plan over 2 Q mask rows."""
    what = "exact_cpquery"
    if not event:
        raise ValueError(f"{what}: event must name at least one variable")
    rows, observed, words = _query(fitted, evidence, event, index, what)
    plan = _plan_for(fitted, (), index, plan, what)
    masks = torch.cat([level_masks(fitted, rows, observed, words, what), level_masks(fitted, rows, observed, None, what)])
    _, z = run_plans(fitted, [plan], masks, index=index, what=what)
    Q = rows.shape[0]
    return z[0, :Q] / z[0, Q:]


def exact_posterior(fitted: FittedBN, targets, evidence, index: int = 0, *, plan=None) -> torch.Tensor:
    """The marginal posteriors of ``targets`` given the evidence, exactly -> float64 [Q, len(targets), 16] on the device in the
    layout and target order (ascending index) of ``posterior``: zero at and beyond the variable's level count, NaN where
    P(evidence) = 0.  One plan per target; ``plan``: the list of them, in ascending target."""
    what = "exact_posterior"
    rows, observed, _ = _query(fitted, evidence, None, index, what)
    mask = _mask_of(targets, fitted.n_vars, what)
    if not mask:
        raise ValueError(f"{what}: targets must name at least one variable")
    tg = [v for v in range(fitted.n_vars) if (mask >> v) & 1]
    if plan is not None and len(plan) != len(tg):
        raise ValueError(f"{what}: plan must hold one EliminationPlan per target")
    plans = [_plan_for(fitted, (v,), index, None if plan is None else plan[t], what) for t, v in enumerate(tg)]
    out, z = run_plans(fitted, plans, level_masks(fitted, rows, observed, None, what), index=index, out_stride=16, what=what)
    return (out / z[:, :, None]).permute(1, 0, 2).contiguous()


def exact_joint(fitted: FittedBN, nodes, evidence, index: int = 0, *, plan=None) -> torch.Tensor:
    """The joint posterior of the variables ``nodes`` given the evidence -> float64 [Q, prod card] on the device, the lowest
    variable id fastest, NaN where P(evidence) = 0."""
    what = "exact_joint"
    rows, observed, _ = _query(fitted, evidence, None, index, what)
    keep = [v for v in range(fitted.n_vars) if (_mask_of(nodes, fitted.n_vars, what) >> v) & 1]
    if not keep:
        raise ValueError(f"{what}: nodes must name at least one variable")
    plan = _plan_for(fitted, keep, index, plan, what)
    out, z = run_plans(fitted, [plan], level_masks(fitted, rows, observed, None, what), index=index, what=what)
    return out[0] / z[0, :, None]
