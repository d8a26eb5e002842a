"""Local and hybrid structure learning on the device (csrc/dvs_local.h): bnlearn's ``mmpc``, ``mmhc`` and
``rsmax2`` for discrete data and, with ``test`` in {"cor", "zf", "mi-g"} on a ``GaussianEvaluator``, for real-valued data
(csrc/dvs_gaussian_ci.h), next to ``pc.py`` and the score-based searches.

``ci_tests_group`` evaluates conditional-independence tests grouped by (target, conditioning set): one workgroup scans the
rows once for every candidate of its group, and each cell is byte for byte what ``ci_tests`` gives for the same test.
``mmpc`` is the max-min parents and children search of Tsamardinos, Brown and Aliferis (2006), all targets in lock-step, one
read-back of 3 n words per round.  ``rsmax2`` restricts a score-based search to a learned skeleton, and ``mmhc`` is
``rsmax2(restrict="mmpc", maximize="hc")``.

The definitions are those of include/dvs_local.h (dvs_ci_tests_group, dvs_mmpc_update).  Parity with bnlearn's ``mmpc``,
``mmhc`` and ``rsmax2`` rests on them and is not pinned against an R run.  Three differences from bnlearn are deliberate:

* ties of the max-min choice go to the larger minimum statistic, then to the lower index, and p-values below 2^-1022 compare
  as 0 (bnlearn compares the p-values as they come);
* the backward phase is one frozen pass — every Z within cpc(t) of at most ``max_cond`` variables tests all of cpc(t) \\ Z at
  once, in the spirit of PC-stable — where bnlearn removes members one after another, so that a removal changes the sets
  that later members are tested against;
* ``max_cond`` defaults to 3, a choice and not a measurement, where bnlearn's ``max.sx`` is unbounded.
"""
from __future__ import annotations

from itertools import combinations
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib as dl
from .hillclimb import hill_climb
from .pc import _evaluator, _gaussian, _one_set, pc_stable, skeleton_blacklist
from .pc import _test_type as _any_test_type
from .tabu import tabu_search

INDEX_RANGE = (1 << 31) - 1                # groups of one round: dvs_ci_tests_group's n_groups


def _test_type(what, test):
    """the dvs_ci_type of ``test``; the permutation tests (dvs_ci_perm_tests) are not built for the grouped kernel"""
    if test in dl.CI_PERM_TYPES:
        raise ValueError(f"{what}: permutation tests are not built for the grouped kernel (got {test!r}): "
                         f"ci_tests and pc_stable take them, and rsmax2(restrict=\"pc.stable\") through pc_stable")
    return _any_test_type(test)


class MMPCResult(NamedTuple):
    skeleton: torch.Tensor                 # int64 [n]: symmetric adjacency rows (the layout skeleton_blacklist and dvs_pc_orient take)
    cpc: torch.Tensor                      # int64 [n]: the parents and children of every target after the backward phase
    forward: torch.Tensor                  # int64 [n]: the same after the forward phase alone
    sepsets: torch.Tensor                  # int64 [n, n]: cell [t, x] the conditioning set that separated x from target t
    groups_per_round: List[int]            # (target, conditioning set) groups of forward round 0, 1, ..., then of the backward pass
    refused: int                           # tests that were refused (table too large; on real-valued data a conditioning set
                                           # beyond dl.GCI_MAX_COND or a collinear one): never counted as independence
    asymmetric: int                        # members removed by the symmetry correction (x in cpc(t), t not in cpc(x))


class RSMAX2Result(NamedTuple):
    search: object                         # the HillClimbResult or TabuResult of the maximise step
    restrict: object                       # the MMPCResult or PCResult of the restrict step
    skeleton: torch.Tensor                 # int64 [n]: the skeleton the search was kept to


def _tensor_arg(what, name, t, dtype, shape_text, ok):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: {name} must be a torch tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"dags_vae_search_amd: {what} runs on the GPU (got {name} on {t.device}); this package has no CPU path")
    if t.dtype != dtype or not ok(t):
        raise ValueError(f"{what}: {name} must be {shape_text}")
    return t.contiguous()


def _launch_group(evaluator, target, cond, candidates, typ, lds_cells, out, status, sets=None):
    lib, p, G = evaluator.lib, dl.ptr, target.numel()
    if _gaussian(evaluator):
        n_sets, set_of = (evaluator.moments.shape[0], None) if sets is None else sets
        dl.check(lib, lib.dvs_gbn_ci_tests_group(G, evaluator.n_vars, p(evaluator.moments), n_sets, p(set_of), p(target), p(cond),
                                                 p(candidates), typ, p(out), dl.nbytes(out), p(status), dl.stream()),
                 "dvs_gbn_ci_tests_group")
        return
    dl.check(lib, lib.dvs_ci_tests_group(G, evaluator.n_vars, evaluator.n_samples, p(evaluator.packed), p(evaluator.card), p(target),
                                         p(cond), p(candidates), typ, lds_cells, p(out), dl.nbytes(out), p(status), dl.stream()),
             "dvs_ci_tests_group")


def ci_tests_group(evaluator, targets, cond, candidates, test: str = "mi", *, lds_cells: Optional[int] = None,
                   return_status: bool = False):
    """``targets`` int32 [G], ``cond`` int64 [G] and ``candidates`` int64 [G] (bit masks), all on the evaluator's device ->
    float64 [G, n, 3] on the device: cell [g, x] is (statistic, df, p-value) of the test of x against ``targets[g]`` given the
    variables in ``cond[g]`` for every x in ``candidates[g]``, byte for byte what ``ci_tests`` returns for it, and three NaNs
    for every other x.  A candidate is refused (three NaNs, bit 4 of the status word) by the rules of ``ci_tests``, its table
    against ``lds_cells`` (None: 36 864, all of the LDS a workgroup can count in; the workgroup takes a group's candidates
    in as many passes over the rows as their tables need).

    On a ``GaussianEvaluator`` with ``test`` in {"cor", "zf", "mi-g"} (include/dvs_gaussian_ci.h) one lane factors the
    conditioning set and the target once and appends a row per candidate; the cells are ``ci_tests``' bytes for the pair
    (``targets[g]``, x), ``lds_cells`` is not read, and on a row-set view group g reads set g, or ``set_of[g]``."""
    what = "ci_tests_group"
    typ = _test_type(what, test)
    gaussian = _evaluator(what, evaluator, test) is None
    targets = _tensor_arg(what, "targets", targets, torch.int32, "int32 [G >= 1]", lambda t: t.ndim == 1 and t.numel() >= 1)
    G = targets.numel()
    cond = _tensor_arg(what, "cond", cond, torch.int64, f"int64 [{G}] bit masks", lambda t: t.shape == (G,))
    candidates = _tensor_arg(what, "candidates", candidates, torch.int64, f"int64 [{G}] bit masks", lambda t: t.shape == (G,))
    lds_cells = dl.CI_MAX_CELLS if lds_cells is None else int(lds_cells)
    if not 1 <= lds_cells <= dl.CI_MAX_CELLS:
        raise ValueError(f"{what}: lds_cells must be in [1, {dl.CI_MAX_CELLS}]")
    if G * evaluator.n_vars > INDEX_RANGE:
        raise ValueError(f"{what}: {G:,} groups of {evaluator.n_vars} cells are beyond the index range of one call ({INDEX_RANGE:,})")
    dev = evaluator.device
    with torch.cuda.device(dev):
        out = torch.empty(G, evaluator.n_vars, 3, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        _launch_group(evaluator, targets, cond, candidates, typ, lds_cells, out, status, evaluator.row_sets(G) if gaussian else None)
    return (out, status) if return_status else out


def _bits(m: int):
    while m:
        low = m & -m
        yield low.bit_length() - 1
        m ^= low


def _subsets(members: int, most: int):
    """the subsets of the set bits of ``members`` with at most ``most`` elements, as masks (any order)"""
    ids = list(_bits(members))
    for k in range(0, min(most, len(ids)) + 1):
        for sub in combinations(ids, k):
            yield sum(1 << u for u in sub)


def forward_groups(cpc: List[int], cand: List[int], last: List[int], max_cond: int):
    """The groups of a forward round after round 0, from the state read back: for a target t whose last member is F >= 0,
    Z = {F} | S' for every S' within cpc(t) \\ {F} with |Z| <= max_cond — exactly the conditioning sets that no earlier
    round has used — in ascending numeric order of Z, each testing all of cand(t).  A target without candidates keeps its
    groups, which ask nothing: the update that reads them is what sets its ``last`` to -1.
    -> (target, cond, candidates, offsets [n + 1])"""
    target, cond, candidates, offsets = [], [], [], [0]
    for t, F in enumerate(last):
        if F >= 0 and max_cond >= 1:
            zs = sorted((1 << F) | s for s in _subsets(cpc[t] & ~(1 << F), max_cond - 1))
            target += [t] * len(zs)
            cond += zs
            candidates += [cand[t]] * len(zs)
        offsets.append(len(target))
    return target, cond, candidates, offsets


def backward_groups(cpc: List[int], max_cond: int):
    """The groups of the backward pass: for every target t and every Z within cpc(t) with |Z| <= max_cond, (t, Z, cpc(t) \\ Z),
    in ascending numeric order of Z"""
    target, cond, candidates, offsets = [], [], [], [0]
    for t, members in enumerate(cpc):
        zs = sorted(_subsets(members, max_cond))
        target += [t] * len(zs)
        cond += zs
        candidates += [members & ~z for z in zs]
        offsets.append(len(target))
    return target, cond, candidates, offsets


def _lds_cells(card, target, cond, candidates):
    """what one pass over a round's largest group needs, within [its largest accepted table, 36 864]: LDS that no group would
    use only lowers the number of workgroups a compute unit holds"""
    need = 1
    for t, z, c in zip(target, cond, candidates):
        q = card[t]
        for u in _bits(z):
            q *= card[u]
        need = max(need, sum(q * card[x] for x in _bits(c)))
        if need >= dl.CI_MAX_CELLS:
            return dl.CI_MAX_CELLS
    return need


def mmpc(evaluator, *, alpha: float = 0.05, test: str = "mi", max_cond: int = 3, targets=None) -> MMPCResult:
    """Max-min parents and children (Tsamardinos, Brown and Aliferis 2006; bnlearn's ``mmpc``) of every target at once.

    Forward: round 0 tests every other variable against the target marginally; in every later round a target that has just
    taken the member F tests its open candidates given every subset of its members that holds F (at most ``max_cond``
    variables).  A candidate with a p-value above ``alpha`` leaves for good; of the rest, the one whose largest p-value so far
    is smallest joins (ties: the larger minimum statistic, then the lower index).  Backward: one frozen pass in which every
    Z within cpc(t) of at most ``max_cond`` variables tests all of cpc(t) \\ Z, and a member with a p-value above ``alpha``
    leaves — order-independent, where bnlearn removes members one after another.  Then the symmetry correction: x stays in
    the skeleton row of t iff x is in cpc(t) and t in cpc(x).

    ``max_cond=3`` is a choice, not a measurement: bnlearn's ``max.sx`` is unbounded.  ``targets`` (None: all) restricts the
    search to those targets; the symmetry correction then leaves edges among them only.  A refused test (a table beyond
    36 864 cells) is counted in ``refused`` and never read as independence.

    On a ``GaussianEvaluator`` ``test`` is "cor", "zf" or "mi-g" (``pc.ci_tests``).  ``cor`` and ``zf`` are signed, so the
    statistic column is replaced by its absolute value before the round's update reads it.  ``max_cond`` may exceed
    ``_lib.GCI_MAX_COND``: the tests beyond it, and those on a collinear conditioning set, are counted in ``refused``."""
    return _mmpc(evaluator, alpha, test, max_cond, targets)


def _mmpc(evaluator, alpha, test, max_cond, targets, rounds=None):
    """``mmpc``; ``rounds``, a list, receives (phase, target, cond, candidates, lds_cells) of every round as it is launched
    (bench_mmpc.py replays them)"""
    what = "mmpc"
    typ = _test_type(what, test)
    card = _evaluator(what, evaluator, test)
    _one_set(what, evaluator)
    gaussian = card is None
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha must be in [0, 1]")
    if int(max_cond) < 0:
        raise ValueError("max_cond must be >= 0")
    max_cond = int(max_cond)
    dev, n, lib, p = evaluator.device, evaluator.n_vars, evaluator.lib, dl.ptr
    chosen = list(range(n)) if targets is None else sorted({int(t) for t in targets})
    if not chosen or chosen[0] < 0 or chosen[-1] >= n:
        raise ValueError(f"{what}: targets must name variables in [0, {n})")
    card = None if gaussian else [int(c) for c in card]
    full = (1 << n) - 1

    def dev_u64(values):
        return torch.from_numpy(np.array(values, np.uint64).view(np.int64)).to(dev)

    def marginal_groups(cand):
        """round 0: one group (t, no conditioning, every other variable) per target"""
        ts = [t for t in range(n) if cand[t]]
        return ts, [0] * len(ts), [cand[t] for t in ts], [sum(1 for u in ts if u < t) for t in range(n + 1)]

    groups_per_round, refused_total = [], 0
    with torch.cuda.device(dev):
        cpc = [0] * n
        cand = [full & ~(1 << t) if t in chosen else 0 for t in range(n)]
        cur = torch.stack([dev_u64(cpc), dev_u64(cand)])                         # the state on the device: cpc and cand ...
        nxt = torch.empty_like(cur)
        last = torch.full((n,), -1, dtype=torch.int32, device=dev)               # ... the member added last ...
        pmax = torch.zeros(n, n, dtype=torch.float64, device=dev)                # ... and what every (t, x) has shown so far
        smin = torch.full((n, n), float("inf"), dtype=torch.float64, device=dev)
        sepsets = torch.zeros(n, n, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)                   # bit 4 says what `refused` counts: not read
        refused = torch.zeros(1, dtype=torch.int32, device=dev)
        result = torch.empty(n, 2, dtype=torch.int64, device=dev)

        def run_round(phase, groups):
            """the grouped tests of a round and what they decide -> (cpc, cand, last) as Python ints: the round's one read-back"""
            nonlocal cur, nxt, refused_total
            target, cond, candidates, offsets = groups
            G = len(target)
            if G * n > INDEX_RANGE:
                raise ValueError(f"{what}: a round has {G:,} groups, beyond the index range of one round ({INDEX_RANGE // n:,} at "
                                 f"{n} variables): lower max_cond (now {max_cond})")
            d_t = torch.tensor(target, dtype=torch.int32, device=dev)
            d_z, d_c = dev_u64(cond), dev_u64(candidates)
            d_off = torch.tensor(offsets, dtype=torch.int64, device=dev)
            out = torch.empty(G, n, 3, dtype=torch.float64, device=dev)
            lds_cells = 0 if gaussian else _lds_cells(card, target, cond, candidates)
            if rounds is not None:
                rounds.append((phase, target, cond, candidates, lds_cells))
            _launch_group(evaluator, d_t, d_z, d_c, typ, lds_cells, out, status)
            if gaussian:
                out[:, :, 0].abs_()              # cor and zf are signed; the tie rule takes the larger minimum statistic
            dl.check(lib, lib.dvs_mmpc_update(n, G, phase, p(d_t), p(d_z), p(d_c), p(d_off), p(out), dl.nbytes(out), float(alpha),
                                              p(cur[0]), p(cur[1]), p(nxt[0]), p(nxt[1]), p(last), p(pmax), p(smin), p(sepsets),
                                              n * n * 8, p(refused), p(result), n * 16, dl.stream()), "dvs_mmpc_update")
            back = torch.cat([nxt.reshape(-1), last.to(torch.int64), refused.to(torch.int64)]).cpu().numpy()
            cur, nxt = nxt, cur
            refused_total += int(back[3 * n])
            groups_per_round.append(G)
            words = back[:2 * n].view(np.uint64)
            return [int(w) for w in words[:n]], [int(w) for w in words[n:]], [int(v) for v in back[2 * n:3 * n]]

        groups = marginal_groups(cand)
        while groups[0]:
            cpc, cand, last_h = run_round(0, groups)
            groups = forward_groups(cpc, cand, last_h, max_cond)
        if max_cond == 0 and any(cand):
            # no conditional test is run: every candidate that the marginal test did not dismiss is a member
            cpc = [c | d for c, d in zip(cpc, cand)]
            cur = torch.stack([dev_u64(cpc), dev_u64([0] * n)])
        forward = cur[0].clone()
        groups = backward_groups(cpc, max_cond)
        if groups[0]:
            cpc, _, _ = run_round(1, groups)
        skeleton = [sum(1 << x for x in _bits(cpc[t]) if (cpc[x] >> t) & 1) for t in range(n)]
        asymmetric = sum(bin(cpc[t] & ~skeleton[t]).count("1") for t in range(n))
        return MMPCResult(dev_u64(skeleton), cur[0].clone(), forward, sepsets, groups_per_round, refused_total, asymmetric)


def rsmax2(evaluator, *, restrict: str = "mmpc", maximize: str = "hc", restrict_args: Optional[Dict] = None,
           maximize_args: Optional[Dict] = None) -> RSMAX2Result:
    """Restrict, then maximise (bnlearn's ``rsmax2``): learn a skeleton with ``mmpc`` ("mmpc") or ``pc_stable`` ("pc.stable") on
    the evaluator's packed data (on a ``GaussianEvaluator``: its moments, ``restrict_args`` naming ``test`` "cor", "zf" or
    "mi-g") with ``restrict_args``, then run ``hill_climb`` ("hc") or ``tabu_search`` ("tabu") on the
    evaluator's metric with ``maximize_args`` and ``forbidden=skeleton_blacklist(skeleton)``, so that every learned arc lies in
    the skeleton.  ``max_steps`` defaults to max(16, n^2); ``maximize_args`` may not name ``forbidden``.  A composition: it
    launches what its two halves launch."""
    what = "rsmax2"
    restrictors = {"mmpc": mmpc, "pc.stable": pc_stable}
    searches = {"hc": hill_climb, "tabu": tabu_search}
    if restrict not in restrictors:
        raise ValueError(f"{what}: restrict must be one of {sorted(restrictors)} (got {restrict!r})")
    if maximize not in searches:
        raise ValueError(f"{what}: maximize must be one of {sorted(searches)} (got {maximize!r})")
    if "forbidden" in (maximize_args or {}):
        raise ValueError(f"{what}: forbidden is the learned skeleton's blacklist and cannot be given in maximize_args")
    if not _gaussian(evaluator):             # a Gaussian evaluator is judged by the restrict step against the test it is given
        _evaluator(what, evaluator)
    restricted = restrictors[restrict](evaluator, **(restrict_args or {}))
    n = evaluator.n_vars
    search_args = {"max_steps": max(16, n * n), **(maximize_args or {})}
    if search_args.get("starts") is None:
        search_args.setdefault("batch", 1)
    found = searches[maximize](evaluator, forbidden=skeleton_blacklist(restricted.skeleton), **search_args)
    return RSMAX2Result(found, restricted, restricted.skeleton)


def mmhc(evaluator, *, restrict_args: Optional[Dict] = None, maximize_args: Optional[Dict] = None) -> RSMAX2Result:
    """Max-min hill climbing (Tsamardinos, Brown and Aliferis 2006; bnlearn's ``mmhc``): ``rsmax2(restrict="mmpc", maximize="hc")``"""
    dl.need_unmixed("mmhc", evaluator)
    return rsmax2(evaluator, restrict="mmpc", maximize="hc", restrict_args=restrict_args, maximize_args=maximize_args)
