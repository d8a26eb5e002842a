"""Exact structure search on the device (csrc/dvs_exact.h): the DAG with the largest score that exists.

``hill_climb``, ``tabu_search`` and ``latent_bo_search`` are heuristics; at the sizes this package works at (asia n = 8,
sachs n = 11, the synthetic n = 12 set) the optimum itself is computable by the subset dynamic programme of Silander and
Myllymaki (2006): the local score of every (variable, parent set), the best parent set within every candidate set, the best
sink of every vertex subset, a backtrack from the full set — n 2^n cells, up to n = 20 on one device.  ``exact_search`` gives
the searches a yardstick ("tabu's best is this far below the optimum") and ``compare_structures(..., equivalence=True)`` a
target on data sets with no published network.

The definitions are those of include/dvs.h (dvs_exact_search): every choice is made by a total order, so two runs give equal
bytes.  Parity with an external exact solver is unpinned; the result rests on those definitions and on brute force.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as dl

MAX_VARS = 20                              # 2^n n cells: 21 M at n = 20, 252 MB of workspace; n = 21 would not index in 31 bits


@dataclass
class ExactResult:
    parents: torch.Tensor                  # int64 [B, n]: the optimal parent masks (bit u of [b, v] <=> u -> v)
    scores: torch.Tensor                   # f64 [B]: the dynamic programme's own value, R[all] of include/dvs.h
    order: torch.Tensor                    # int32 [B, n]: a topological order of parents (parents[order[k]] within order[:k])
    flags: torch.Tensor                    # int32 [B]: always zero on return (a set flag raises)
    rescored: Optional[torch.Tensor] = None    # exact_search: evaluator.score_masks(parents), the other summation order


def _refuse_size(what, n, batch=1):
    if n > MAX_VARS:
        raise ValueError(f"{what}: n_vars = {n} > {MAX_VARS}: the dynamic programme holds 2^n * n cells per table "
                         f"({(1 << n) * n:,} here), which is beyond one device's memory and a 31-bit index")
    if batch * (1 << n) * n >= 1 << 31:
        raise ValueError(f"{what}: batch * 2^n * n = {batch * (1 << n) * n:,} cells must be < 2^31")


def exact_from_tables(tables: torch.Tensor, *, max_parents: Optional[int] = None, forbidden=None, lib=None) -> ExactResult:
    """``tables``: f64 [B, 2^n, n] on the device, cell [b, S, v] the local score of v with parent set ``S & ~(1 << v)`` (NaN:
    not available); B independent tables are solved in one call.  ``max_parents`` (None: no cap) and ``forbidden`` (int64
    [n], bit u of ``forbidden[v]`` bars u -> v) are those of ``hill_climb``.  A table with no admissible DAG (some variable
    may not even stand without parents) raises ``ValueError`` naming the rows."""
    what = "exact_from_tables"
    if not torch.is_tensor(tables):
        raise TypeError(f"{what}: tables must be a torch tensor")
    dl.need_cuda(what, tables.device)
    if tables.dtype != torch.float64 or tables.ndim != 3 or tables.shape[0] < 1 or tables.shape[2] < 1:
        raise ValueError(f"{what}: tables must be float64 [B >= 1, 2^n, n]")
    B, rows, n = tables.shape
    _refuse_size(what, n, B)
    if rows != 1 << n:
        raise ValueError(f"{what}: tables must be float64 [B, 2^n, n] (got {rows} rows for n = {n})")
    lib = dl.load() if lib is None else lib
    tables = tables.contiguous()
    dev = tables.device
    with torch.cuda.device(dev):
        forb = dl.forbidden_rows(forbidden, n, dev)
        ws_bytes = dl.workspace_bytes(lib, "dvs_exact_workspace_bytes", B, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        parents = torch.empty(B, n, dtype=torch.int64, device=dev)
        order = torch.empty(B, n, dtype=torch.int32, device=dev)
        scores = torch.empty(B, dtype=torch.float64, device=dev)
        flags = torch.empty(B, dtype=torch.int32, device=dev)
        p = dl.ptr
        dl.check(lib, lib.dvs_exact_search(B, n, p(tables), tables.numel() * 8, 0 if max_parents is None else int(max_parents),
                                           p(forb), p(ws), ws_bytes, p(parents), p(order), p(scores), p(flags), dl.stream()),
                 "dvs_exact_search")
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            raise ValueError(f"{what}: no admissible DAG (a variable's empty parent set is not available): rows "
                             f"{[int(b) for b in bad.cpu()]}")
    return ExactResult(parents, scores, order, flags)


def local_score_table(evaluator, *, max_parents: Optional[int] = None, chunk: int = 65536) -> torch.Tensor:
    """f64 [2^n, n] on the evaluator's device: cell [S, v] is the evaluator's local score of v with parent set
    ``S & ~(1 << v)``, bit for bit what ``score_masks(local=True)`` gives for a row holding that set — the scorer writes
    straight into the table, ``chunk`` rows a call.  A family the scorer refuses is NaN in its cell alone (not an error here:
    that parent set is not available).  With ``max_parents = k`` only the rows with ``popcount(S) <= k + 1`` are scored and
    the rest of the table is NaN."""
    what = "local_score_table"
    dl.need_unmixed(what, evaluator)
    dev, n = evaluator.device, evaluator.n_vars
    dl.need_cuda(what, dev)
    _refuse_size(what, n)
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    rows = 1 << n
    with torch.cuda.device(dev):
        table = torch.full((rows, n), float("nan"), dtype=torch.float64, device=dev)
        S = torch.arange(rows, dtype=torch.int64, device=dev)
        capped = max_parents is not None and int(max_parents) > 0 and int(max_parents) + 1 < n
        if capped:
            pop = torch.zeros(rows, dtype=torch.int64, device=dev)
            for u in range(n):
                pop += (S >> u) & 1
            S = S[pop <= int(max_parents) + 1]
        own = ~(torch.ones(n, dtype=torch.int64, device=dev) << torch.arange(n, dtype=torch.int64, device=dev))
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for r0 in range(0, S.numel(), chunk):
            sel = S[r0:r0 + chunk]
            m = sel.numel()
            parents = (sel[:, None] & own[None, :]).contiguous()
            # uncapped, the rows of a chunk are the table's rows r0 .. r0 + m - 1: the scorer's scratch is the table itself
            scratch = torch.empty(m, n, dtype=torch.float64, device=dev) if capped else table[r0:r0 + m]
            out = torch.empty(m, dtype=torch.float64, device=dev)
            evaluator.launch_scores(parents, scratch, out, status)
            if capped:
                table[sel] = scratch
    return table


def exact_search(evaluator, *, max_parents: Optional[int] = None, forbidden=None) -> ExactResult:
    """The optimal DAG for the evaluator's score and data under ``max_parents`` and ``forbidden`` (B = 1):
    ``local_score_table`` then ``exact_from_tables``.  ``scores`` is the dynamic programme's own value (the local scores
    added in sink order); ``rescored`` is ``evaluator.score_masks(parents)``, the same n terms added by variable index."""
    dl.need_unmixed("exact_search", evaluator)
    table = local_score_table(evaluator, max_parents=max_parents)
    res = exact_from_tables(table[None], max_parents=max_parents, forbidden=forbidden, lib=evaluator.lib)
    with torch.cuda.device(evaluator.device):
        res.rescored = evaluator.score_masks(res.parents)
    return res
