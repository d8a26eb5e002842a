"""Structure comparison on the device (csrc/dvs_cpdag.h): the CPDAG of a batch of DAGs, and SHD with the arc
confusion counts against a known network — what ``hill_climb``, ``tabu_search`` and ``latent_bo_search`` results are judged
by, without copying thousands of masks to the host.

Masks are int64 [B, n] on the GPU (``HillClimbResult.parents``): bit u of row v stands for u -> v.  A PDAG has the same
layout; an undirected edge u - v sets bit u of row v and bit v of row u (bnlearn's ``amat``).  No evaluator is needed.

The definitions are those of include/dvs.h (dvs_cpdag, dvs_pdag_compare).  Parity with bnlearn's ``cpdag``, ``shd`` and
``compare`` rests on them and is not pinned against an R run.
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import torch

from . import _lib as dl

FLAG_CYCLE, FLAG_ILLEGAL = 1, 2            # dvs_cpdag's flags
MAX_VARS = 48


class StructureComparison(NamedTuple):
    shd: torch.Tensor                      # int32 [B]: pairs whose states differ
    tp: torch.Tensor                       # int32 [B]: edges of `parents` with the same state in `target`
    fp: torch.Tensor                       # int32 [B]: edges of `parents` whose state differs in `target`
    fn: torch.Tensor                       # int32 [B]: edges of `target` whose state differs in `parents`
    hamming: torch.Tensor                  # int32 [B]: pairs adjacent in exactly one of the two


def cpdag_of(what, name, parents):
    """``cpdag`` of masks that ``_lib.parent_masks`` has checked; ``what`` and ``name`` word the refusal"""
    lib, p = dl.load(), dl.ptr
    B, n = parents.shape
    with torch.cuda.device(parents.device):
        out = torch.empty_like(parents)
        flags = torch.empty(B, dtype=torch.int32, device=parents.device)
        dl.check(lib, lib.dvs_cpdag(B, n, p(parents), p(out), out.numel() * 8, p(flags), dl.stream()), "dvs_cpdag")
        bad = torch.nonzero(flags).reshape(-1)
        if bad.numel():
            fl = flags.cpu()
            cyc = [int(b) for b in bad.cpu() if int(fl[b]) == FLAG_CYCLE]
            ill = [int(b) for b in bad.cpu() if int(fl[b]) == FLAG_ILLEGAL]
            raise ValueError(f"{what}: {name} with a cycle: rows {cyc}; {name} with a self-loop or a parent bit >= {n}: rows {ill}")
    return out


def cpdag(parents: torch.Tensor) -> torch.Tensor:
    """int64 [B, n] parent masks of DAGs (any variable order) -> int64 [B, n] CPDAGs: an edge is directed iff it has that
    direction in every DAG of the Markov equivalence class.  The rows are a canonical key of the class.  A row set with a
    cycle, a self-loop or a parent bit >= n raises ``ValueError`` naming the rows."""
    return cpdag_of("cpdag", "parents", dl.parent_masks("cpdag", "parents", parents))


def compare_structures(parents: torch.Tensor, target: torch.Tensor, *, equivalence: bool = True) -> StructureComparison:
    """``parents`` int64 [B, n] against ``target`` int64 [n] (one network for the whole batch) or [B, n].

    ``equivalence=True`` compares the CPDAGs of both sides: ``shd`` is the structural Hamming distance of Tsamardinos et al.
    (2006), zero exactly for DAGs of one Markov equivalence class, and tp / fp / fn are the counts of bnlearn's ``compare``
    on the CPDAGs.  ``False`` compares the masks as given (DAGs, or PDAGs the caller already has): a reversed arc is then
    shd 1, fp 1, fn 1.  ``hamming`` counts the skeleton differences either way.  All fields are int32 [B] on the device."""
    what = "compare_structures"
    a = dl.parent_masks(what, "parents", parents)
    B, n = a.shape
    if torch.is_tensor(target) and target.ndim == 1:
        target = target[None, :]
    t = dl.parent_masks(what, "target", target, n)
    if t.shape[0] not in (1, B) or t.device != a.device:
        raise ValueError(f"{what}: target must be [{n}] or [{B}, {n}] on {a.device}")
    if equivalence:
        a, t = cpdag_of(what, "parents", a), cpdag_of(what, "target", t)
    lib, p = dl.load(), dl.ptr
    with torch.cuda.device(a.device):
        counts = torch.empty(B, 5, dtype=torch.int32, device=a.device)
        dl.check(lib, lib.dvs_pdag_compare(B, n, p(a), p(t), t.shape[0], p(counts), counts.numel() * 4, dl.stream()), "dvs_pdag_compare")
    return StructureComparison(*(counts[:, k].contiguous() for k in range(5)))


def shd(parents: torch.Tensor, target: torch.Tensor, *, equivalence: bool = True) -> torch.Tensor:
    """``compare_structures(parents, target, equivalence=equivalence).shd``"""
    return compare_structures(parents, target, equivalence=equivalence).shd


def equivalence_classes(parents: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(class_of int64 [B], representatives int64 [K, n]): the CPDAG rows of the K Markov equivalence classes present in the
    batch, and for every structure the index of its class.  Two structures share a class iff their CPDAG rows are equal."""
    representatives, class_of = torch.unique(cpdag(parents), dim=0, return_inverse=True)
    return class_of, representatives
