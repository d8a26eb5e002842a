"""Bootstrap arc strengths and the averaged network on the device (csrc/dvs_strength.h).

bnlearn's model averaging: ``boot.strength`` learns one network per bootstrap replicate of the data, ``custom.strength``
counts how often each arc and each direction appears, ``inclusion.threshold`` picks the significance threshold and
``averaged.network`` builds the consensus DAG.  Here the replicates are one batch: ``bootstrap_rows`` draws the row sets,
``BNLearnWrapper.with_rows`` scores structure b on set b, and ``hill_climb`` / ``tabu_search`` climb all replicates in
lock-step.  ``arc_strength`` also summarises any other batch of structures (the rounds of ``hill_climb(restarts=)``, the
decoded candidates of ``latent_bo_search``).

The definitions are those of include/dvs.h (dvs_bootstrap_rows, dvs_arc_strength, dvs_averaged_network).  Two differences
from bnlearn, on purpose: a pair whose two directions are exactly tied is oriented (lower index -> higher first) where
bnlearn leaves it undirected, and the threshold is the closed form of the L1 estimator where bnlearn runs ``optimize``.
Parity with an R run is not pinned.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from fractions import Fraction
from typing import List, Optional, Sequence, Union

import torch

from . import _lib as dl
from .compare import cpdag_of
from .hillclimb import hill_climb
from .tabu import tabu_search


def bootstrap_rows(n_sets: int, set_size: int, n_samples: int, *, seed: int, set_offset: int = 0, device="cuda") -> torch.Tensor:
    """int32 [n_sets, set_size] row indices drawn with replacement from 0 .. n_samples - 1 (dvs_bootstrap_rows).  Set r is a
    function of (``seed``, ``set_offset`` + r) only, so a request may be cut into calls or shards."""
    device = torch.device(device)
    dl.need_cuda("bootstrap_rows", device)
    lib = dl.load()
    with torch.cuda.device(device):
        rows = torch.empty(int(n_sets), int(set_size), dtype=torch.int32, device=device)
        dl.check(lib, lib.dvs_bootstrap_rows(int(n_sets), int(set_size), int(n_samples), dl.seed64(seed),
                                             int(set_offset), dl.ptr(rows), dl.stream()), "dvs_bootstrap_rows")
    return rows


@dataclass
class ArcStrength:
    any: torch.Tensor                      # int32 [n, n]: networks in which u and v are adjacent (symmetric)
    dir2: torch.Tensor                     # int32 [n, n]: twice the direction count of u -> v (an undirected edge adds 1)
    n_networks: int                        # R
    exhausted: int = 0                     # boot_strength: replicates whose search ran out of max_steps
    networks: Optional[torch.Tensor] = None    # boot_strength(return_networks=True): int64 [R, n] learned parent masks

    @property
    def strength(self) -> torch.Tensor:
        """f64 [n, n]: any / R, each cell one correctly rounded division (a tensor divided by a Python scalar is multiplied
        by the reciprocal and can be an ulp off)"""
        num = self.any.to(torch.float64)
        return num / torch.full_like(num, float(self.n_networks))

    @property
    def direction(self) -> torch.Tensor:
        """f64 [n, n]: dir2 / (2 any), 0 where any = 0"""
        den = 2.0 * self.any.to(torch.float64)
        return torch.where(self.any > 0, self.dir2.to(torch.float64) / den.clamp(min=1.0), torch.zeros_like(den))

    def __add__(self, other: "ArcStrength") -> "ArcStrength":
        if not isinstance(other, ArcStrength) or other.any.shape != self.any.shape:
            return NotImplemented
        nets = None
        if self.networks is not None and other.networks is not None:
            nets = torch.cat([self.networks, other.networks])
        return ArcStrength(self.any + other.any, self.dir2 + other.dir2, self.n_networks + other.n_networks,
                           self.exhausted + other.exhausted, nets)


def _accumulate(counts: torch.Tensor, pdag: torch.Tensor):
    lib = dl.load()
    B, n = pdag.shape
    dl.check(lib, lib.dvs_arc_strength(B, n, dl.ptr(pdag), dl.ptr(counts), counts.numel() * 4, dl.stream()), "dvs_arc_strength")


def arc_strength(structures: torch.Tensor, *, cpdag: bool = True) -> ArcStrength:
    """Arc counts over a batch of networks (dvs_arc_strength): ``structures`` int64 [B, n] parent masks, or PDAGs with
    ``cpdag=False``.  ``cpdag=True`` (boot.strength's default) counts over the CPDAGs of the DAGs, so an arc that is
    reversible within its equivalence class counts half for either direction."""
    what = "arc_strength"
    x = dl.parent_masks(what, "structures", structures)
    if cpdag:
        x = cpdag_of(what, "structures", x)
    n = x.shape[1]
    with torch.cuda.device(x.device):
        counts = torch.zeros(n, n, 2, dtype=torch.int32, device=x.device)
        _accumulate(counts, x)
    return ArcStrength(counts[..., 0].contiguous(), counts[..., 1].contiguous(), int(x.shape[0]))


def boot_strength(evaluator, *, replicates: int = 200, m: Optional[int] = None, algorithm: str = "hc",
                  algorithm_args: Optional[dict] = None, cpdag: bool = True, seed: int = 0, set_offset: int = 0,
                  chunk: Optional[int] = None, return_networks: bool = False) -> ArcStrength:
    """bnlearn's ``boot.strength``: one structure search per bootstrap replicate of the evaluator's data, all replicates of
    a chunk in one lock-step batch, reduced to arc counts on the device.

    ``evaluator``: a ``BNLearnWrapper``.  ``m``: rows per replicate (default: the data set's).  ``algorithm``: ``"hc"``
    (``hill_climb``) or ``"tabu"`` (``tabu_search``), each from empty graphs with ``algorithm_args`` (``max_steps`` is
    required; ``starts`` / ``batch`` are not taken).  ``chunk``: replicates per batch (default: all).  Replicate r draws
    its rows from (``seed``, ``set_offset`` + r) and, with ``restarts=0``, depends on nothing else: the result is the same
    for every ``chunk``, and shards with different ``set_offset`` add up (``+``).  With ``restarts`` the perturbation is
    keyed by the replicate's index within its batch (``dvs_hc_perturb``, as in ``hill_climb``), so the result then
    depends on ``chunk``.  ``exhausted`` counts the replicates whose search ran out of ``max_steps``."""
    dl.need_unmixed("boot_strength", evaluator)
    if algorithm not in ("hc", "tabu"):
        raise ValueError(f"algorithm must be 'hc' or 'tabu' (got {algorithm!r})")
    args = dict(algorithm_args or {})
    if "starts" in args or "batch" in args:
        raise ValueError("boot_strength climbs from empty graphs: algorithm_args takes neither starts nor batch")
    if "max_steps" not in args:
        raise ValueError("algorithm_args needs max_steps")
    R = int(replicates)
    if R < 1:
        raise ValueError("replicates must be >= 1")
    size = evaluator.n_samples if m is None else int(m)
    step = R if chunk is None else int(chunk)
    if step < 1 or size < 1:
        raise ValueError("chunk and m must be >= 1")
    args.setdefault("seed", seed)
    search = hill_climb if algorithm == "hc" else tabu_search
    dev, n = evaluator.device, evaluator.n_vars
    nets, exhausted = [], 0
    with torch.cuda.device(dev):
        counts = torch.zeros(n, n, 2, dtype=torch.int32, device=dev)
        for at in range(0, R, step):
            b = min(step, R - at)
            rows = bootstrap_rows(b, size, evaluator.n_samples, seed=seed, set_offset=set_offset + at, device=dev)
            res = search(evaluator.with_rows(rows), batch=b, **args)
            exhausted += int((res.converged == 0).sum())
            _accumulate(counts, cpdag_of("boot_strength", "networks", res.parents) if cpdag else res.parents.contiguous())
            if return_networks:
                nets.append(res.parents)
    return ArcStrength(counts[..., 0].contiguous(), counts[..., 1].contiguous(), R, exhausted,
                       torch.cat(nets) if return_networks else None)


@dataclass
class AveragedNetwork:
    parents: torch.Tensor                  # int64 [n] parent masks of the consensus DAG ([T, n] for a threshold sweep)
    threshold: Union[float, List[float]]   # the threshold used, as a fraction: arcs with strength > threshold are significant
    placed: Union[int, List[int]]          # arcs in the network
    dropped: Union[int, List[int]]         # significant pairs left out because their arc would have closed a cycle
    ties: Union[int, List[int]]            # significant pairs whose two directions were exactly tied


def _averaged(strength: ArcStrength, min_any: Sequence[int]):
    lib, p = dl.load(), dl.ptr
    dev = strength.any.device
    dl.need_cuda("averaged_network", dev)
    n, G = strength.any.shape[0], len(min_any)
    with torch.cuda.device(dev):
        counts = torch.stack([strength.any, strength.dir2], -1).to(torch.int32)[None].expand(G, n, n, 2).contiguous()
        nn = torch.full((G,), int(strength.n_networks), dtype=torch.int32, device=dev)
        ma = torch.tensor([int(x) for x in min_any], dtype=torch.int32, device=dev)
        parents = torch.empty(G, n, dtype=torch.int64, device=dev)
        info = torch.empty(G, 4, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_averaged_network(G, n, p(counts), p(nn), p(ma), p(parents), parents.numel() * 8, p(info),
                                               dl.stream()), "dvs_averaged_network")
    return parents, info.cpu().tolist()


def inclusion_threshold(strength: ArcStrength) -> float:
    """bnlearn's ``inclusion.threshold``: the estimated significance threshold as a fraction of the networks (the L1
    estimator of Scutari and Nagarajan 2013 in closed form, include/dvs.h); arcs with strength above it are significant."""
    _, info = _averaged(strength, [-1])
    return (info[0][0] - 1) / float(strength.n_networks)


def averaged_network(strength: ArcStrength, threshold=None) -> AveragedNetwork:
    """bnlearn's ``averaged.network``: the consensus DAG of the arcs whose strength exceeds ``threshold`` (None: the
    estimated one), each in its majority direction, strongest first, skipping what would close a cycle.  ``threshold``
    may be a list of floats: a sweep in one launch, every field then a list (``parents`` [T, n])."""
    R = int(strength.n_networks)
    sweep = isinstance(threshold, (list, tuple))
    ts = list(threshold) if sweep else [threshold]
    min_any = []
    for t in ts:
        if t is None:
            min_any.append(-1)
        else:
            if not (math.isfinite(t) and 0.0 <= t <= 1.0):
                raise ValueError(f"threshold must be in [0, 1] (got {t!r})")
            min_any.append(math.floor(Fraction(t) * R) + 1)          # strength > t <=> any >= floor(t R) + 1, in integers
    parents, info = _averaged(strength, min_any)
    used = [(row[0] - 1) / float(R) if t is None else float(t) for row, t in zip(info, ts)]
    cols = [[row[k] for row in info] for k in (1, 2, 3)]
    if sweep:
        return AveragedNetwork(parents, used, *cols)
    return AveragedNetwork(parents[0], used[0], *(c[0] for c in cols))
