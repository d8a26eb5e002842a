"""Tabu search over single-edge moves on the device (csrc/dvs_tabu.h), next to ``hill_climb``.

bnlearn's ``tabu``: from each start take the best add, delete or reversal that does not lead back to one of the last ``tabu``
structures stood on — whatever its sign, so the walk leaves a local optimum instead of stopping there — remember the best
structure seen, and stop after ``max_tabu`` moves in a row that did not raise it.  Batched like ``hill_climb`` and built on
the same pieces (``hillclimb._Search``): per step ``dvs_tabu_step`` and the incremental ``dvs_bn_toggle_scores`` pass, only
the count of structures that moved read back every ``check_every`` steps; ``restarts`` rounds from the best so far after
``perturb`` random legal moves (``dvs_hc_perturb``).

The rules are those of include/dvs.h (dvs_tabu_step); parity with bnlearn's ``tabu`` is not pinned against a bnlearn run,
and where every move is tabu this search stops (bnlearn picks one of the tabu moves).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _lib as dl
from .hillclimb import _Search


@dataclass
class TabuResult:
    parents: torch.Tensor                  # int64 [B, n]: the best structure seen (bit u of [b, v] <=> u -> v)
    scores: torch.Tensor                   # f64 [B]: evaluator.score_masks(parents)
    last_parents: torch.Tensor             # int64 [B, n]: where the last round's walk stood when it stopped
    steps: torch.Tensor                    # int32 [B]: moves taken in the last round
    converged: torch.Tensor                # int32 [B]: 1 where the last round stopped by itself (0: max_steps ran out)
    flags: torch.Tensor                    # int32 [B]: always zero on return (a set flag raises)
    trace: Optional[Tuple[torch.Tensor, torch.Tensor]]   # the last round's (codes int64, deltas f64) [B, max_steps] or None
    rounds: int                            # restarts done


def tabu_search(evaluator, starts=None, *, batch: Optional[int] = None, max_steps: int, tabu: int = 10,
                max_tabu: Optional[int] = None, max_parents: Optional[int] = None, min_delta: float = 0.0, forbidden=None,
                check_every: int = 8, restarts: int = 0, perturb: int = 1, seed: int = 0, trace: bool = False) -> TabuResult:
    """Tabu search from every start at once.

    ``evaluator``, ``starts`` / ``batch``, ``max_parents``, ``forbidden``, ``check_every``, ``trace``, ``restarts`` /
    ``perturb`` / ``seed`` and the errors are those of ``hill_climb``.  ``tabu``: the number of structures remembered (the
    one stood on included).  ``max_tabu``: a walk stops after this many moves in a row that did not raise its best score by
    more than ``min_delta`` (None: ``tabu``, bnlearn's default), or when every legal move is tabu, or after ``max_steps``."""
    if tabu < 1:
        raise ValueError("tabu must be >= 1")
    max_tabu = int(tabu) if max_tabu is None else int(max_tabu)
    if max_tabu < 1:
        raise ValueError("max_tabu must be >= 1")
    s = _Search("tabu_search", evaluator, starts, batch, max_steps, max_parents, forbidden, check_every, restarts, perturb, trace)
    lib, B, n, p = s.lib, s.B, s.n, dl.ptr
    with torch.cuda.device(s.dev):
        ring = torch.zeros(B, int(tabu), n, dtype=torch.int64, device=s.dev)
        visited = torch.zeros(B, dtype=torch.int32, device=s.dev)
        stall = torch.zeros(B, dtype=torch.int32, device=s.dev)
        best_score = torch.full((B,), float("-inf"), dtype=torch.float64, device=s.dev)
        best_parents = torch.zeros(B, n, dtype=torch.int64, device=s.dev)

    def launch_step(slot, stream):
        dl.check(lib, lib.dvs_tabu_step(*s.step_args(min_delta, slot), int(tabu), p(ring), ring.numel() * 8, p(visited), max_tabu,
                                        p(stall), p(best_score), p(best_parents), best_parents.numel() * 8, stream),
                 "dvs_tabu_step")

    def reset_round():
        visited.zero_()
        stall.zero_()
        best_score.fill_(float("-inf"))

    best = s.run(launch_step, lambda: (best_parents, best_score), reset_round, seed)
    with torch.cuda.device(s.dev):
        parents = best_parents if best is None else best[0]
        scores = evaluator.score_masks(parents)
    return TabuResult(parents, scores, s.parents, s.steps, s.converged, s.flags, s.out_trace(), s.rounds)
