"""Order MCMC on the device (csrc/dvs_ordermc.h): posterior arc probabilities beyond n = 20, and a structure
search over variable orders, for everything the package scores (n <= 48).

``arc_posterior`` is exact but holds 2^n n cells; ``boot_strength`` works at any size but measures how often a greedy search
finds an arc.  This module is the standard answer in between, the Metropolis sampler over variable orders of Friedman and
Koller (2003): the state is a permutation, a step swaps two positions and re-sums the capped parent-set lists of the variables
in between, and P(u -> v | order) is a closed sum that is averaged over the sampled orders (Rao-Blackwellised).  Its input is
a *family list* (``FamilyScores``): per variable the admissible parent sets with their scores, in place of the 2^n table.
The sampler's stationary distribution is exactly what ``arc_posterior`` computes on the same cells, so for n <= 20 that
function is its yardstick, as ``exact_search`` is for ``best()``.

The prior is ORDER-MODULAR, not uniform over DAGs: uniform over the n! variable orders and, apart from ``parent_prior``,
uniform over the listed parent sets within an order, so a DAG's prior weight is proportional to its number of linear
extensions.  This is the known bias of the method, kept deliberately (see posterior.py).  The definitions are those of
include/dvs.h (dvs_order_mcmc); a chain is a function of (seed, global chain index, step index) only and every sum has a fixed
order, so two runs — or one run cut into calls (``state=``) or shards (``chain_offset=``) — give equal bytes.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib as dl
from .posterior import ArcProbabilities, _size_prior
from .strength import ArcStrength

FLAG_TEXT = {1: "offsets do not ascend from 0 to the number of families with at least one family per variable",
             2: "a variable's first family is not the empty set", 4: "a mask holds its own variable or a bit >= n",
             8: "a score is not finite", 16: "a start order is not a permutation"}


def _refuse_families(what, total):
    if total >= 1 << 31:
        raise ValueError(f"{what}: the list would hold {total:,} families; n_families must be < 2^31 (lower max_parents or "
                         f"narrow candidates)")


@dataclass
class FamilyScores:
    """A family list for n <= 48 variables: the families of v are the entries ``offsets[v] .. offsets[v + 1] - 1``; entry 0 of
    every variable is the empty set; a mask of v holds neither bit v nor a bit >= n; scores are finite.  The prior these
    scores imply over DAGs is order-modular (see the module docstring)."""
    n_vars: int
    offsets: torch.Tensor                  # int64 [n + 1] on the device
    sets: torch.Tensor                     # int64 [F]: parent masks (the library reads them as u64)
    scores: torch.Tensor                   # f64 [F]
    lib: object = None

    @property
    def n_families(self) -> int:
        return int(self.sets.numel())

    @property
    def device(self):
        return self.sets.device

    @classmethod
    def from_table(cls, table: torch.Tensor, max_parents: Optional[int] = None, forbidden=None, parent_prior=None) -> "FamilyScores":
        """The f64 [2^n, n] table of ``local_score_table`` as the list whose cells are, bit for bit, the f(v, P) of
        ``dvs_arc_posterior``: the same admissibility (not its own parent, within ``max_parents``, not ``forbidden``, not
        NaN) and the same one addition of the size prior; v's sets by size, then by mask.  On these lists ``order_mcmc``
        samples exactly the order-modular posterior ``arc_posterior`` sums."""
        what = "FamilyScores.from_table"
        if not torch.is_tensor(table) or table.dtype != torch.float64 or table.ndim != 2 or table.shape[1] < 1 or \
                table.shape[0] != 1 << table.shape[1]:
            raise ValueError(f"{what}: table must be float64 [2^n, n]")
        dl.need_cuda(what, table.device)
        rows, n = table.shape
        dev = table.device
        with torch.cuda.device(dev):
            forb = dl.forbidden_rows(forbidden, n, dev)
            prior = _size_prior(what, parent_prior, n, dev)
            S = torch.arange(rows, dtype=torch.int64, device=dev)
            pop = torch.zeros(rows, dtype=torch.int64, device=dev)
            for u in range(n):
                pop += (S >> u) & 1
            cap = 0 if max_parents is None else int(max_parents)
            sets, scores, counts = [], [], []
            for v in range(n):
                x = table[:, v]
                ok = ((S >> v) & 1 == 0) & (x == x)
                if cap > 0:
                    ok &= pop <= cap
                if forb is not None:
                    ok &= (S & forb[v]) == 0
                P = S[ok]
                P = P[torch.argsort(pop[P] * rows + P)]
                f = x[P]
                sets.append(P)
                scores.append(f if prior is None else f + prior[torch.clamp(pop[P], max=n - 1)])
                counts.append(int(P.numel()))
            if any(c == 0 for c in counts):
                raise ValueError(f"{what}: a variable has no admissible parent set")
            offsets = torch.tensor([0] + [sum(counts[:v + 1]) for v in range(n)], dtype=torch.int64, device=dev)
            return cls(n, offsets, torch.cat(sets).contiguous(), torch.cat(scores).contiguous())


def family_scores(evaluator, max_parents: int = 3, candidates=None, forbidden=None, parent_prior=None,
                  chunk: int = 65536) -> FamilyScores:
    """Per variable every subset of its candidate parents of size <= ``max_parents``, scored by the evaluator, as a family
    list on the device.  ``candidates``: int64 [n] mask rows (bit u of row v: u may be a parent of v; default all other
    variables); ``forbidden`` as in ``hill_climb`` (bit u of row v bars u -> v).  The enumeration order is fixed: by size,
    then by numeric mask.  Row r of a scorer call holds the r-th family of every variable, so n = 37 with 3 parents takes
    7 807 structure rows, ``chunk`` a call.  A family the scorer refuses (NaN) is dropped; ``parent_prior`` (None,
    ``"koivisto"`` or a float64 [n] tensor, as in ``arc_posterior``) is added by set size.  Over DAGs the resulting prior is
    order-modular, not uniform (see the module docstring)."""
    what = "family_scores"
    dl.need_unmixed(what, evaluator)
    dev, n = evaluator.device, evaluator.n_vars
    dl.need_cuda(what, dev)
    cap = int(max_parents)
    if cap < 0 or chunk < 1:
        raise ValueError(f"{what}: max_parents must be >= 0 and chunk >= 1")
    with torch.cuda.device(dev):
        everyone = (1 << n) - 1
        cand = [everyone & ~(1 << v) for v in range(n)]
        if candidates is not None:
            if not torch.is_tensor(candidates) or candidates.dtype != torch.int64 or candidates.shape != (n,):
                raise ValueError(f"{what}: candidates must be an int64 [{n}] tensor of mask rows")
            cand = [c & int(m) for c, m in zip(cand, candidates.cpu().tolist())]
        forb = dl.forbidden_rows(forbidden, n, dev)
        if forb is not None:
            cand = [c & ~int(m) for c, m in zip(cand, forb.cpu().tolist())]
        sizes = [bin(c).count("1") for c in cand]
        counts = [sum(math.comb(k, j) for j in range(min(cap, k) + 1)) for k in sizes]
        _refuse_families(what, sum(counts))
        prior = _size_prior(what, parent_prior, n, dev)
        R = max(counts)
        parents = torch.zeros(R, n, dtype=torch.int64, device=dev)
        pops = []
        for v in range(n):
            idx = torch.tensor([u for u in range(n) if (cand[v] >> u) & 1], dtype=torch.int64, device=dev)
            parts, pop = [torch.zeros(1, dtype=torch.int64, device=dev)], [torch.zeros(1, dtype=torch.int64, device=dev)]
            for k in range(1, min(cap, sizes[v]) + 1):
                masks = (torch.ones((), dtype=torch.int64, device=dev) << torch.combinations(idx, k)).sum(1)
                parts.append(torch.sort(masks).values)
                pop.append(torch.full_like(masks, k))
            parents[:counts[v], v] = torch.cat(parts)
            pops.append(torch.cat(pop))
        local = torch.empty(R, n, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        for r0 in range(0, R, chunk):
            m = min(chunk, R - r0)
            out = torch.empty(m, dtype=torch.float64, device=dev)
            evaluator.launch_scores(parents[r0:r0 + m], local[r0:r0 + m], out, status)
        sets, scores, keeps = [], [], []
        for v in range(n):
            x = local[:counts[v], v]
            keep = x == x
            f = x[keep]
            sets.append(parents[:counts[v], v][keep])
            scores.append(f if prior is None else f + prior[pops[v][keep]])
            keeps.append(keep[0].to(torch.int64))
            keeps.append(keep.sum())
        host = torch.stack(keeps).cpu().tolist()
        if not all(host[0::2]):
            raise ValueError(f"{what}: the scorer refuses the empty parent set of variable(s) {[v for v in range(n) if not host[2 * v]]}")
        kept = host[1::2]
        offsets = torch.tensor([0] + [sum(kept[:v + 1]) for v in range(n)], dtype=torch.int64, device=dev)
        return FamilyScores(n, offsets, torch.cat(sets).contiguous(), torch.cat(scores).contiguous(), evaluator.lib)


@dataclass
class OrderMCMCResult(ArcProbabilities):
    """What ``order_mcmc`` returns.  Every probability here is under the order-modular prior (see the module docstring)."""
    prob: torch.Tensor                     # f64 [n, n]: [u, v] = the chains' estimate of P(u -> v | data)
    per_chain: torch.Tensor                # f64 [C, n, n]: each chain's own estimate (0 where it kept nothing)
    std_error: torch.Tensor                # f64 [n, n]: the between-chain standard deviation / sqrt(C)
    accept_rate: torch.Tensor              # f64 [C]: accepted proposals / steps so far
    log_score: torch.Tensor                # f64 [C]: the score of each chain's last order
    orders: torch.Tensor                   # int32 [C, n]: each chain's last order, position -> variable
    best_parents: torch.Tensor             # int64 [C, n]: the best DAG each chain has seen (parent masks)
    best_score: torch.Tensor               # f64 [C]: its score
    trace: Optional[torch.Tensor]          # f64 [C, steps] or None: the order's score after each step of this call
    sums: torch.Tensor                     # f64 [C, n, n], kept int32 [C], accepted int32 [C]: what a continuation takes on
    kept: torch.Tensor
    accepted: torch.Tensor
    steps_done: int
    settings: dict                         # burn_in, thin, window, seed, chain_offset as used: a continuation takes them over

    def best(self):
        """(parent masks int64 [n], score) of the chain whose best DAG scores highest (the first of equals)"""
        c = int(torch.argmax(self.best_score))
        return self.best_parents[c], float(self.best_score[c])

    def to_arc_strength(self, resolution: int = 1_000_000) -> ArcStrength:
        """``prob`` as the counts of ``resolution`` imaginary networks, with the formulas of ``ArcPosterior``: what
        ``averaged_network`` and ``inclusion_threshold`` take"""
        return self.counts(self.prob, resolution)


def order_mcmc(families_or_evaluator, *, chains: int = 256, steps: int, burn_in: Optional[int] = None, thin: Optional[int] = None,
               window: Optional[int] = 1, seed: Optional[int] = None, chain_offset: Optional[int] = None,
               state: Optional[OrderMCMCResult] = None, trace: bool = False, **family_args) -> OrderMCMCResult:
    """``chains`` independent Metropolis chains over variable orders, ``steps`` steps each, one workgroup a chain.

    ``families_or_evaluator``: a ``FamilyScores``, or an evaluator that goes through ``family_scores(**family_args)``.
    ``burn_in`` (default ``steps // 5``) and ``thin`` (default n) choose the kept samples: every global step t >= burn_in with
    (t - burn_in) % thin == 0.  ``window``: a proposal swaps positions i and j with j - i <= window (default 1, adjacent;
    None means n - 1).  These defaults are unmeasured choices.  ``state``: an earlier result to continue; its
    burn_in, thin, seed and chain_offset are taken over unless given (window is per call), and the result equals, byte for
    byte, one run of the combined length with those settings.  ``chain_offset`` shards a run: chains g = chain_offset + c draw what chain g of
    one large call draws.  A malformed list raises ``ValueError`` naming what the device found.  The estimate is of the
    posterior under the ORDER-MODULAR prior, not a uniform prior over DAGs (see the module docstring)."""
    what = "order_mcmc"
    fam = families_or_evaluator
    if not isinstance(fam, FamilyScores):
        dl.need_unmixed(what, fam)
        fam = family_scores(fam, **family_args)
    elif family_args:
        raise TypeError(f"{what}: {sorted(family_args)} apply to an evaluator, not to a FamilyScores")
    dev, n, F = fam.device, fam.n_vars, fam.n_families
    dl.need_cuda(what, dev)
    _refuse_families(what, F)
    C, steps = int(chains), int(steps)
    if C < 1 or steps < 0:
        raise ValueError(f"{what}: chains must be >= 1 and steps >= 0")
    prev = state.settings if state is not None else {}
    burn_in = prev.get("burn_in", steps // 5) if burn_in is None else int(burn_in)
    thin = prev.get("thin", n) if thin is None else int(thin)
    window = max(1, n - 1) if window is None else int(window)
    seed = prev.get("seed", 0) if seed is None else int(seed)
    chain_offset = prev.get("chain_offset", 0) if chain_offset is None else int(chain_offset)
    if not 1 <= window <= max(1, n - 1):
        raise ValueError(f"{what}: window must be in [1, max(1, n - 1)] = [1, {max(1, n - 1)}] (got {window})")
    if thin < 1 or burn_in < 0:
        raise ValueError(f"{what}: thin must be >= 1 and burn_in >= 0")
    lib = fam.lib or dl.load()
    with torch.cuda.device(dev):
        if state is None:
            step_offset, init = 0, 1
            order = torch.empty(C, n, dtype=torch.int32, device=dev)
            accepted = torch.zeros(C, dtype=torch.int32, device=dev)
            sums = torch.zeros(C, n, n, dtype=torch.float64, device=dev)
            kept = torch.zeros(C, dtype=torch.int32, device=dev)
            best_score = torch.full((C,), float("-inf"), dtype=torch.float64, device=dev)
            best_parents = torch.zeros(C, n, dtype=torch.int64, device=dev)
        else:
            if state.orders.shape != (C, n):
                raise ValueError(f"{what}: state holds {tuple(state.orders.shape)} orders, the call asks for {(C, n)}")
            step_offset, init = state.steps_done, 0
            order, accepted, sums, kept = state.orders.clone(), state.accepted.clone(), state.sums.clone(), state.kept.clone()
            best_score, best_parents = state.best_score.clone(), state.best_parents.clone()
        log_score = torch.empty(C, dtype=torch.float64, device=dev)
        tr = torch.empty(C, steps, dtype=torch.float64, device=dev) if trace else None
        prob = torch.empty(n, n, dtype=torch.float64, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        p = dl.ptr
        dl.check(lib, lib.dvs_order_mcmc(C, n, F, steps, p(fam.offsets), p(fam.sets), dl.nbytes(fam.sets), p(fam.scores),
                                         dl.nbytes(fam.scores), dl.seed64(seed), chain_offset, step_offset, burn_in, thin, window,
                                         init, p(order), p(log_score), p(accepted), p(sums), dl.nbytes(sums), p(kept),
                                         p(best_score), p(best_parents), p(tr), 0 if tr is None else dl.nbytes(tr), p(flags),
                                         dl.stream()), "dvs_order_mcmc")
        dl.check(lib, lib.dvs_order_mcmc_finish(C, n, p(sums), dl.nbytes(sums), p(kept), p(prob), dl.stream()),
                 "dvs_order_mcmc_finish")
        bits = int(flags.item())
        if bits:
            raise ValueError(f"{what}: the family list is malformed: " + "; ".join(t for b, t in FLAG_TEXT.items() if bits & b))
        k = kept.to(torch.float64)[:, None, None]
        per_chain = torch.where(k > 0, sums / torch.where(k > 0, k, torch.ones_like(k)), torch.zeros_like(sums))
        std_error = per_chain.std(0, unbiased=True) / math.sqrt(C) if C > 1 else torch.zeros_like(prob)
        done = step_offset + steps
        rate = accepted.to(torch.float64) / max(done, 1)
    return OrderMCMCResult(prob, per_chain, std_error, rate, log_score, order, best_parents, best_score, tr, sums, kept, accepted,
                           done, dict(burn_in=burn_in, thin=thin, window=window, seed=seed, chain_offset=chain_offset))
