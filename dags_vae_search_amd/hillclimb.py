"""Greedy hill climbing over single-edge moves on the device (csrc/dvs_hillclimb.h).

The baseline every structure-search method is measured against — bnlearn's ``hc``: from each start take the add, delete or
reversal with the largest score gain until none gains more than ``min_delta`` — batched over thousands of starts, with the
evaluator's own score (any of ``BNLearnWrapper``'s types) and data.  Per step two launches: ``dvs_hc_step`` picks and
applies one move per structure, ``dvs_bn_toggle_scores`` re-scores the 2 n families of the one or two rows that changed.
Nothing but the count of structures that moved is read back, every ``check_every`` steps.

The move rules are those of include/dvs.h (dvs_hc_step); parity with bnlearn's ``hc`` rests on them and is not pinned
against a bnlearn run.  No tabu list, no random restarts, no whitelist.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
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


def hill_climb(evaluator, starts=None, *, batch: Optional[int] = None, max_steps: int, max_parents: Optional[int] = None,
               min_delta: float = 0.0, forbidden=None, check_every: int = 8, trace: bool = False) -> HillClimbResult:
    """Climb from every start at once.

    ``evaluator``: a ``BNLearnWrapper``.  ``starts``: int64 [B, n] parent masks in data-set variable indices, a
    ``CompactBatch`` (e.g. from ``generate_dags``), or None with ``batch=`` for that many empty graphs.  ``max_parents``:
    no add or reversal gives a variable more parents than this (None: no cap).  ``forbidden``: int64 [n], bit u of
    ``forbidden[v]`` bars the edge u -> v (bnlearn's blacklist).  A move is taken only if it gains more than ``min_delta``.
    ``trace=True`` records every move as (code, delta), see ``decode_move``.  A start with a cycle, or one the evaluator
    cannot score, raises ``ValueError`` naming the rows."""
    lib, dev, n = evaluator.lib, evaluator.device, evaluator.n_vars
    if dev.type != "cuda":
        raise RuntimeError(f"dags_vae_search_amd: hill_climb runs on the GPU (got device {dev}); this package has no CPU path")
    if max_steps < 1 or check_every < 1:
        raise ValueError("max_steps and check_every must be >= 1")
    if isinstance(starts, CompactBatch):
        parents = evaluator.compact_parent_masks(starts)
    elif starts is None:
        if batch is None:
            raise ValueError("hill_climb: pass starts, or batch= for empty graphs")
        parents = torch.zeros(int(batch), n, dtype=torch.int64, device=dev)
    else:
        parents = torch.as_tensor(starts).to(device=dev, dtype=torch.int64, copy=True).contiguous()
    if parents.ndim != 2 or parents.shape[1] != n or parents.shape[0] < 1:
        raise ValueError(f"starts must be [B >= 1, {n}] parent masks")
    B = parents.shape[0]
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        forb = None
        if forbidden is not None:
            forb = torch.as_tensor(np.asarray(forbidden).astype(np.uint64).view(np.int64) if not torch.is_tensor(forbidden)
                                   else forbidden).to(device=dev, dtype=torch.int64).contiguous()
            if forb.shape != (n,):
                raise ValueError(f"forbidden must be [{n}] bit rows")
        worklist = torch.full((2 * B,), -1, dtype=torch.int32, device=dev)
        steps = torch.zeros(B, dtype=torch.int32, device=dev)
        converged = torch.zeros(B, dtype=torch.int32, device=dev)
        flags = torch.zeros(B, dtype=torch.int32, device=dev)
        active = torch.zeros(max_steps, dtype=torch.int32, device=dev)
        tr = torch.zeros(B, max_steps, 2, dtype=torch.int64, device=dev) if trace else None
        L, T = evaluator.toggle_scores(parents)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        cap = 0 if max_parents is None else int(max_parents)
        for t in range(max_steps):
            dl.check(lib, lib.dvs_hc_step(B, n, p(parents), p(L), p(T), T.numel() * 8, cap, float(min_delta), p(forb),
                                          int(max_steps), p(worklist), p(steps), p(converged), p(flags), p(tr),
                                          0 if tr is None else tr.numel() * 8, ctypes.c_void_p(active.data_ptr() + 4 * t),
                                          stream), "dvs_hc_step")
            evaluator.toggle_scores(parents, worklist=worklist, out=(L, T))
            if (t + 1) % check_every == 0 and int(active[t].item()) == 0:
                break
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            fl = flags.cpu()
            cyc = [int(b) for b in bad.cpu() if int(fl[b]) & FLAG_CYCLE]
            nan = [int(b) for b in bad.cpu() if int(fl[b]) & FLAG_NAN_SCORE]
            raise ValueError(f"hill_climb: starts with a cycle: rows {cyc}; starts the evaluator refuses to score (a parent "
                             f"set too large for the counting paths, or a parent bit >= {n}): rows {nan}")
        scores = evaluator.score_masks(parents)
    out_trace = None
    if tr is not None:
        out_trace = (tr[..., 0].contiguous(), tr[..., 1].contiguous().view(torch.float64))
    return HillClimbResult(parents, scores, steps, converged, flags, out_trace)
