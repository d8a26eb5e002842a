"""Greedy hill climbing over single-edge moves on the device (csrc/dvs_hillclimb.h).

The baseline every structure-search method is measured against — bnlearn's ``hc``: from each start take the add, delete or
reversal with the largest score gain until none gains more than ``min_delta`` — batched over thousands of starts, with the
evaluator's own score (any of ``BNLearnWrapper``'s types) and data.  Per step two launches: ``dvs_hc_step`` picks and
applies one move per structure, ``dvs_bn_toggle_scores`` re-scores the 2 n families of the one or two rows that changed.
Nothing but the count of structures that moved is read back, every ``check_every`` steps.

The move rules are those of include/dvs.h (dvs_hc_step); parity with bnlearn's ``hc`` rests on them and is not pinned
against a bnlearn run.  Random restarts: ``restarts=`` here; a tabu list: ``tabu_search`` (tabu.py), which
shares this module's starts, argument handling and round loop.  No whitelist.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as dl
from .records import CompactBatch

FLAG_CYCLE, FLAG_NAN_SCORE = 1, 2          # dvs_hc_step's flags


@dataclass
class HillClimbResult:
    parents: torch.Tensor                  # int64 [B, n]: the final parent masks (bit u of [b, v] <=> u -> v)
    scores: torch.Tensor                   # f64 [B]: evaluator.score_masks(parents)
    steps: torch.Tensor                    # int32 [B]: moves taken
    converged: torch.Tensor                # int32 [B]: 1 where no move gains more than min_delta (0: max_steps ran out)
    flags: torch.Tensor                    # int32 [B]: always zero on return (a set flag raises)
    trace: Optional[Tuple[torch.Tensor, torch.Tensor]]   # (codes int64 [B, max_steps], deltas f64 [B, max_steps]) or None


def decode_move(code: int, n: int):
    """code = op n^2 + v n + u -> (op, u, v): op 0 adds, 1 deletes, 2 reverses the edge u -> v"""
    return ("add", "delete", "reverse")[code // (n * n)], code % n, (code % (n * n)) // n


class _Search:
    """The device state and the round loop that ``hill_climb`` and ``tabu_search`` (tabu.py) share: starts and argument
    handling, two launches per step, random restarts."""

    def __init__(self, what, evaluator, starts, batch, max_steps, max_parents, forbidden, check_every, restarts, perturb, trace):
        self.what, self.ev = what, evaluator
        self.lib, dev, n = evaluator.lib, evaluator.device, evaluator.n_vars
        dl.need_cuda(what, dev)
        if max_steps < 1 or check_every < 1:
            raise ValueError("max_steps and check_every must be >= 1")
        if restarts < 0 or perturb < 1:
            raise ValueError("restarts must be >= 0 and perturb >= 1")
        if isinstance(starts, CompactBatch):
            parents = evaluator.compact_parent_masks(starts)
        elif starts is None:
            if batch is None:
                raise ValueError(f"{what}: pass starts, or batch= for empty graphs")
            parents = torch.zeros(int(batch), n, dtype=torch.int64, device=dev)
        else:
            parents = torch.as_tensor(starts).to(device=dev, dtype=torch.int64, copy=True).contiguous()
        if parents.ndim != 2 or parents.shape[1] != n or parents.shape[0] < 1:
            raise ValueError(f"starts must be [B >= 1, {n}] parent masks")
        self.parents, self.n, self.dev = parents, n, dev
        self.B = B = parents.shape[0]
        self.max_steps, self.check_every, self.restarts, self.perturb = int(max_steps), int(check_every), int(restarts), int(perturb)
        self.cap = 0 if max_parents is None else int(max_parents)
        with torch.cuda.device(dev):
            self.forb = dl.forbidden_rows(forbidden, n, dev)
            self.worklist = torch.full((2 * B,), -1, dtype=torch.int32, device=dev)
            self.steps = torch.zeros(B, dtype=torch.int32, device=dev)
            self.converged = torch.zeros(B, dtype=torch.int32, device=dev)
            self.flags = torch.zeros(B, dtype=torch.int32, device=dev)
            self.active = torch.zeros((self.restarts + 1) * self.max_steps, dtype=torch.int32, device=dev)
            self.tr = torch.zeros(B, self.max_steps, 2, dtype=torch.int64, device=dev) if trace else None
        self.rounds = 0

    def step_args(self, min_delta, slot):
        """the arguments dvs_hc_step and dvs_tabu_step have in common: (batch .. active)"""
        p, tr = dl.ptr, self.tr
        return (self.B, self.n, p(self.parents), p(self.L), p(self.T), self.T.numel() * 8, self.cap, float(min_delta),
                p(self.forb), self.max_steps, p(self.worklist), p(self.steps), p(self.converged), p(self.flags), p(tr),
                0 if tr is None else tr.numel() * 8, p(self.active, 4 * slot))

    def run(self, launch_step, round_best, reset_round, seed):
        """``launch_step(slot, stream)`` enqueues one step kernel counting into ``active[slot]``; ``round_best()`` gives the
        (parents, scores) a round ends with; ``reset_round()`` clears the step kernel's own state.  Returns the best
        (parents, scores) over the rounds, or None with ``restarts == 0`` (nothing to fold)."""
        ev, p = self.ev, dl.ptr
        best = None
        with torch.cuda.device(self.dev):
            self.L, self.T = ev.toggle_scores(self.parents)
            stream = dl.stream()
            for rnd in range(self.restarts + 1):
                if rnd:
                    # from the best so far: one full pass, then `perturb` random legal moves, each with its incremental pass
                    self.parents.copy_(best[0])
                    ev.toggle_scores(self.parents, out=(self.L, self.T))
                    for k in range(self.perturb):
                        dl.check(self.lib, self.lib.dvs_hc_perturb(
                            self.B, self.n, p(self.parents), p(self.L), p(self.T), self.T.numel() * 8, self.cap, p(self.forb),
                            p(self.worklist), p(self.flags), dl.seed64(seed),
                            (rnd * self.perturb + k) & 0xFFFFFFFF, stream), "dvs_hc_perturb")
                        ev.toggle_scores(self.parents, worklist=self.worklist, out=(self.L, self.T))
                    self.steps.zero_()
                    self.converged.zero_()
                    if self.tr is not None:
                        self.tr.zero_()
                    reset_round()
                    self.rounds = rnd
                for t in range(self.max_steps):
                    launch_step(rnd * self.max_steps + t, stream)
                    ev.toggle_scores(self.parents, worklist=self.worklist, out=(self.L, self.T))
                    if (t + 1) % self.check_every == 0 and int(self.active[rnd * self.max_steps + t].item()) == 0:
                        break
                self.raise_flagged()
                if self.restarts == 0:
                    return None
                rp, rs = round_best()
                if best is None:
                    best = (rp.clone(), rs.clone())
                else:
                    better = rs > best[1]                             # ties keep the earlier round's
                    best = (torch.where(better[:, None], rp, best[0]), torch.where(better, rs, best[1]))
        return best

    def raise_flagged(self):
        bad = torch.nonzero(self.flags).reshape(-1)
        if bad.numel():
            fl = self.flags.cpu()
            cyc = [int(b) for b in bad.cpu() if int(fl[b]) & FLAG_CYCLE]
            nan = [int(b) for b in bad.cpu() if int(fl[b]) & FLAG_NAN_SCORE]
            raise ValueError(f"{self.what}: starts with a cycle: rows {cyc}; starts the evaluator refuses to score (a parent "
                             f"set too large for the counting paths, or a parent bit >= {self.n}): rows {nan}")

    def out_trace(self):
        if self.tr is None:
            return None
        return (self.tr[..., 0].contiguous(), self.tr[..., 1].contiguous().view(torch.float64))


def hill_climb(evaluator, starts=None, *, batch: Optional[int] = None, max_steps: int, max_parents: Optional[int] = None,
               min_delta: float = 0.0, forbidden=None, check_every: int = 8, restarts: int = 0, perturb: int = 1, seed: int = 0,
               trace: bool = False) -> HillClimbResult:
    """Climb from every start at once.

    ``evaluator``: a ``BNLearnWrapper``, a ``GaussianEvaluator`` or a ``MixedEvaluator``.  ``starts``: int64 [B, n] parent masks in data-set variable indices, a
    ``CompactBatch`` (e.g. from ``generate_dags``), or None with ``batch=`` for that many empty graphs.  ``max_parents``:
    no add or reversal gives a variable more parents than this (None: no cap).  ``forbidden``: int64 [n], bit u of
    ``forbidden[v]`` bars the edge u -> v (bnlearn's blacklist).  A move is taken only if it gains more than ``min_delta``.
    ``trace=True`` records every move as (code, delta), see ``decode_move``.  A start with a cycle, or one the evaluator
    cannot score, raises ``ValueError`` naming the rows.

    ``restarts`` (bnlearn's ``hc(restart=, perturb=)``): that many further rounds, each from the best structure so far after
    ``perturb`` uniformly random legal moves (``dvs_hc_perturb``, drawn from ``seed``), up to ``max_steps`` moves each;
    ``parents`` / ``scores`` are then the best over the rounds and ``steps`` / ``converged`` / ``trace`` those of the last
    round.  With the default 0 the launch sequence is that of a plain climb."""
    s = _Search("hill_climb", evaluator, starts, batch, max_steps, max_parents, forbidden, check_every, restarts, perturb, trace)
    lib = s.lib

    def launch_step(slot, stream):
        dl.check(lib, lib.dvs_hc_step(*s.step_args(min_delta, slot), stream), "dvs_hc_step")

    # a greedy round ends at its best structure
    best = s.run(launch_step, lambda: (s.parents, evaluator.score_masks(s.parents)), lambda: None, seed)
    with torch.cuda.device(s.dev):
        parents = s.parents if best is None else best[0]
        scores = evaluator.score_masks(parents)
    return HillClimbResult(parents, scores, s.steps, s.converged, s.flags, s.out_trace())
