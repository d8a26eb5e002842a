"""Constraint-based structure learning on the device (csrc/dvs_citest.h): bnlearn's ``ci.test`` and
``pc.stable`` for discrete data and, with ``test`` in {"cor", "zf", "mi-g"} on a ``GaussianEvaluator``, for real-valued data
(csrc/dvs_gaussian_ci.h), next to the score-based searches.

``ci_tests`` evaluates a batch of conditional-independence tests (G^2 ``mi``, Pearson ``x2`` and their ``-adf`` variants, and
the Monte Carlo permutation family ``mc-``, ``smc-``, ``sp-`` ``mi`` / ``x2`` of csrc/dvs_permtest.h) on the
evaluator's packed data set; ``pc_stable`` runs the order-independent PC skeleton search level by level (one read-back of the
48 adjacency words per level) and orients the result into a PDAG; ``skeleton_blacklist`` turns a learned skeleton into the
``forbidden`` rows that ``hill_climb``, ``tabu_search`` and ``exact_search`` accept — the restrict-then-maximise hybrid.

The definitions are those of include/dvs.h (dvs_ci_tests, dvs_pc_expand, dvs_pc_reduce, dvs_pc_orient).  Parity with
bnlearn's ``ci.test`` / ``pc.stable`` rests on them and is not pinned against an R run.  The permutation tests are defined in
include/dvs_permtest.h; their p-value is count / B, bnlearn's convention as recalled, and that too is not pinned against R.
The Gaussian tests are defined in include/dvs_gaussian_ci.h: one Cholesky factor of the moments per test, no pass over the
rows; Student's t for ``cor``, Fisher's z for ``zf``, the chi-square form for ``mi-g``, as bnlearn's are recalled and unpinned
against R as well.  A discrete test name on a Gaussian evaluator and a Gaussian test name on a discrete one raise ``ValueError``.
"""
from __future__ import annotations

from math import comb
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from . import _lib as dl

MAX_VARS = 48
INDEX_RANGE = (1 << 31) - 1                # tests of one level: dvs_pc_expand's n_tests
PERM_MAX = 1 << 20                         # permutations of one test: dvs_ci_perm_tests' n_perm
PERM_FILL = 4                              # a permutation launch is sliced until tests * slices reaches PERM_FILL workgroups per
                                           # CU: chosen before anything was measured; DESIGN.md §28 has what it costs


class PCResult(NamedTuple):
    pdag: torch.Tensor                     # int64 [n]: bit u of row v <=> u -> v or u - v (the layout of ``cpdag``)
    skeleton: torch.Tensor                 # int64 [n]: symmetric adjacency rows
    sepsets: torch.Tensor                  # int64 [n, n]: the separating set of every separated pair, as a bit mask
    tests_per_level: List[int]             # tests evaluated at level 0, 1, ...
    refused: int                           # tests that were refused (table too large; on real-valued data a conditioning set
                                           # beyond dl.GCI_MAX_COND or a collinear one): never counted as independence
    conflicts: int                         # edges that colliders claimed in both directions (left undirected)
    flags: int                             # 0, or 1 when the directed part of ``pdag`` has a cycle


def _gaussian(evaluator):
    """whether the evaluator holds real-valued data (gaussian.py): its tests are dl.GCI_TYPES over ``evaluator.moments``"""
    return dl.data_kind(evaluator) == "continuous"


def _evaluator(what, evaluator, test=None):
    """the level counts of a discrete evaluator, or None for a Gaussian one asked for one of its own tests (dl.GCI_TYPES); a
    test of the other kind of data is a ValueError"""
    dl.need_unmixed(what, evaluator)
    if test in dl.GCI_TYPES:
        if not _gaussian(evaluator):
            raise ValueError(f"{what}: test {test!r} reads real-valued data and the evaluator holds discrete levels: pass a "
                             f"GaussianEvaluator, or one of {sorted(dl.CI_TYPES) + sorted(dl.CI_PERM_TYPES)}")
        if getattr(evaluator, "ci_refusal", None):           # GaussianMomentsEvaluator (gaussian.py)
            raise ValueError(f"{what}: {evaluator.ci_refusal}")
        dl.need_cuda(what, evaluator.device)
        return None
    dl.need_discrete(what, evaluator)
    dl.need_cuda(what, evaluator.device)
    return evaluator.card_host


def _test_type(test):
    """the dvs_ci_type of an asymptotic test, the dvs_gci_type of a Gaussian one (dl.GCI_TYPES), or the name itself for a
    permutation test (dl.CI_PERM_TYPES)"""
    if test in dl.CI_PERM_TYPES:
        return test
    if test in dl.GCI_TYPES:
        return dl.GCI_TYPES[test]
    if test not in dl.CI_TYPES:
        raise ValueError(f"test must be one of {sorted(dl.CI_TYPES) + sorted(dl.CI_PERM_TYPES) + sorted(dl.GCI_TYPES)} (got {test!r})")
    return dl.CI_TYPES[test]


def _one_set(what, evaluator):
    """pc_stable and mmpc learn one structure: a row-set view of several sets has no single data set to learn it from"""
    if _gaussian(evaluator) and evaluator.moments.shape[0] != 1:
        raise ValueError(f"{what}: the evaluator is a view of {evaluator.moments.shape[0]} row sets and {what} learns from one: "
                         f"pass the base evaluator or a view of one set")


class _Perm(NamedTuple):
    """what a permutation test takes beyond the tests themselves"""
    B: int
    seed: int
    alpha: float
    test_offset: int

    @staticmethod
    def of(what, test, B, seed, alpha, test_offset=0):
        if not 1 <= int(B) <= PERM_MAX:
            raise ValueError(f"{what}: B must be in [1, 2^20]")
        if test.startswith("smc-") and not 0.0 < float(alpha) < 1.0:
            raise ValueError(f"{what}: alpha must be in (0, 1) for {test}")
        if not 0 <= int(test_offset) < 1 << 32:
            raise ValueError(f"{what}: test_offset must be in [0, 2^32)")
        return _Perm(int(B), dl.seed64(seed), float(alpha), int(test_offset))


def _max_cells(card, level):
    """the largest (z, x, y) table a test with `level` conditioning variables can have, capped at what LDS holds"""
    cells = 1
    for c in sorted(card, reverse=True)[:level + 2]:
        cells *= c
    return max(1, min(cells, dl.CI_MAX_CELLS))


def _run_perm_tests(evaluator, pairs, cond, test, perm, max_cells, out, status, used, chunk):
    """dvs_ci_perm_tests in chunks; test t of the batch draws as global test perm.test_offset + t (mod 2^32)"""
    lib, T, p = evaluator.lib, cond.numel(), dl.ptr
    blocks = (perm.B + 255) // 256
    chunk = max(1, min(chunk, INDEX_RANGE // blocks))
    cus = torch.cuda.get_device_properties(evaluator.device).multi_processor_count
    work = torch.empty(dl.workspace_bytes(lib, "dvs_ci_perm_workspace_bytes", min(chunk, T), perm.B), dtype=torch.uint8,
                       device=evaluator.device)                  # sized for the largest chunk: a smaller one needs less
    for t0 in range(0, T, chunk):
        m = min(chunk, T - t0)
        slices = max(1, min(blocks, -(-PERM_FILL * cus // m)))
        dl.check(lib, lib.dvs_ci_perm_tests(m, evaluator.n_vars, evaluator.n_samples, p(evaluator.packed), p(evaluator.card),
                                            p(pairs[t0:]), p(cond[t0:]), dl.CI_PERM_TYPES[test], perm.B, perm.alpha, perm.seed,
                                            (perm.test_offset + t0) & 0xFFFFFFFF, slices, max_cells, p(work), dl.nbytes(work),
                                            p(out[t0:]), m * 24, p(used[t0:]), p(status), dl.stream()), "dvs_ci_perm_tests")


def _run_gaussian_tests(evaluator, pairs, cond, typ, out, status, chunk, sets=None):
    """dvs_gbn_ci_tests over the evaluator's moments in chunks; ``sets`` = (n_sets, set_of int32 [T] or None: set 0)"""
    lib, T, p = evaluator.lib, cond.numel(), dl.ptr
    n_sets, set_of = (evaluator.moments.shape[0], None) if sets is None else sets
    for t0 in range(0, T, chunk):
        m = min(chunk, T - t0)
        dl.check(lib, lib.dvs_gbn_ci_tests(m, evaluator.n_vars, p(evaluator.moments), n_sets, None if set_of is None else p(set_of[t0:]),
                                           p(pairs[t0:]), p(cond[t0:]), typ, p(out[t0:]), m * 24, p(status), dl.stream()),
                 "dvs_gbn_ci_tests")


def _run_tests(evaluator, pairs, cond, typ, max_cells, out, status, chunk, perm=None, used=None):
    if _gaussian(evaluator):
        return _run_gaussian_tests(evaluator, pairs, cond, typ, out, status, chunk)
    if perm is not None:
        if used is None:
            used = torch.empty(cond.numel(), dtype=torch.int32, device=evaluator.device)
        return _run_perm_tests(evaluator, pairs, cond, typ, perm, max_cells, out, status, used, chunk)
    lib, T, p = evaluator.lib, cond.numel(), dl.ptr
    for t0 in range(0, T, chunk):
        m = min(chunk, T - t0)
        dl.check(lib, lib.dvs_ci_tests(m, evaluator.n_vars, evaluator.n_samples, p(evaluator.packed), p(evaluator.card),
                                       p(pairs[t0:]), p(cond[t0:]), typ, max_cells, p(out[t0:]), m * 24, p(status), dl.stream()),
                 "dvs_ci_tests")


def ci_tests(evaluator, pairs, cond, test: str = "mi", *, return_status: bool = False, chunk: int = 65536, B: int = 5000,
             seed: int = 0, alpha: float = 0.05, test_offset: int = 0, return_used: bool = False):
    """``pairs`` int32 [T, 2] (x, y) and ``cond`` int64 [T] (bit z: z is conditioned on), both on the evaluator's device ->
    float64 [T, 3] on the device: (statistic, df, p-value) of ``test`` in {"mi", "x2", "mi-adf", "x2-adf"}.  A test whose
    table exceeds 36 864 cells, with x = y, with x or y in its conditioning set or with an index outside the data set comes
    back as three NaNs (``return_status=True`` also returns the status word: bit 4 says that some test was refused).

    ``test`` in {"mc-mi", "mc-x2", "smc-mi", "smc-x2", "sp-mi", "sp-x2"} is a permutation test (include/dvs_permtest.h) with
    ``B`` permutations (5000 is bnlearn's default as recalled: an unmeasured choice) drawn from ``seed``; test t of the batch
    draws as global test ``test_offset + t``, so a batch cut into calls gives the bytes of the whole.  ``alpha`` is the
    threshold of the sequential ``smc-`` tests' early stop and is not read otherwise.  p = count / B follows bnlearn's
    convention as recalled; parity with an R run is not pinned.  ``return_used=True`` (permutation tests only) also returns
    int32 [T], the permutations each test counted: B, fewer where an ``smc-`` test stopped early, 0 for a refused test.  The
    returns come in the order (out, status, used).

    On a ``GaussianEvaluator``, ``test`` in {"cor", "zf", "mi-g"} (include/dvs_gaussian_ci.h) reads the evaluator's moments:
    (Student's t, m - k - 2, two-sided p), (Fisher's z, m - k - 3, two-sided p) or (-m log(1 - r^2), 1, p) with r the partial
    correlation of x and y given the k conditioning variables and m the rows.  Refused (three NaNs): x = y, x or y in the
    conditioning set, an index outside the data, more than ``_lib.GCI_MAX_COND`` conditioning variables, df < 1, and a
    collinear set (a Cholesky pivot within rounding of zero).  On a row-set view test t reads set t, or ``set_of[t]``."""
    what = "ci_tests"
    typ = _test_type(test)
    card = _evaluator(what, evaluator, test)
    perm = _Perm.of(what, test, B, seed, alpha, test_offset) if test in dl.CI_PERM_TYPES else None
    if return_used and perm is None:
        raise ValueError(f"{what}: return_used goes with a permutation test (got {test!r})")
    for name, t in (("pairs", pairs), ("cond", cond)):
        if not torch.is_tensor(t):
            raise TypeError(f"{what}: {name} must be a torch tensor")
        if t.device.type != "cuda":
            raise RuntimeError(f"dags_vae_search_amd: {what} runs on the GPU (got {name} on {t.device}); this package has no CPU path")
    if pairs.dtype != torch.int32 or pairs.ndim != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1:
        raise ValueError(f"{what}: pairs must be int32 [T >= 1, 2]")
    if cond.dtype != torch.int64 or cond.shape != (pairs.shape[0],):
        raise ValueError(f"{what}: cond must be int64 [{pairs.shape[0]}] bit masks")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    dev = evaluator.device
    with torch.cuda.device(dev):
        pairs, cond = pairs.contiguous(), cond.contiguous()
        if card is None:
            out = torch.empty(cond.numel(), 3, dtype=torch.float64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            _run_gaussian_tests(evaluator, pairs, cond, typ, out, status, chunk, evaluator.row_sets(cond.numel()))
            return (out, status) if return_status else out
        # the largest conditioning set sizes the LDS table: a popcount of the bits below n_vars (a higher bit is refused anyway)
        x = cond & ((1 << evaluator.n_vars) - 1)
        x = x - ((x >> 1) & 0x5555555555555555)
        x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
        x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
        level = int(((x * 0x0101010101010101) >> 56).max())
        out = torch.empty(cond.numel(), 3, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        used = torch.empty(cond.numel(), dtype=torch.int32, device=dev) if perm is not None else None
        _run_tests(evaluator, pairs, cond, typ, _max_cells(card, level), out, status, chunk, perm, used)
    ret = (out,) + ((status,) if return_status else ()) + ((used,) if return_used else ())
    return ret if len(ret) > 1 else out


def ci_test(evaluator, x: int, y: int, cond=(), test: str = "mi", *, B: int = 5000, seed: int = 0, alpha: float = 0.05,
            test_offset: int = 0, return_used: bool = False):
    """one test of x against y given the variables in ``cond`` -> float64 [3] on the device: (statistic, df, p-value); the
    keywords are those of ``ci_tests`` for a permutation test (with ``return_used`` the result is (float64 [3], int32 [], the
    permutations counted))"""
    _evaluator("ci_test", evaluator, test)
    mask = 0
    for z in cond:
        if not 0 <= int(z) < 63:
            raise ValueError(f"ci_test: conditioning variable {z} out of range")
        mask |= 1 << int(z)
    dev = evaluator.device
    pairs = torch.tensor([[int(x), int(y)]], dtype=torch.int32, device=dev)
    got = ci_tests(evaluator, pairs, torch.tensor([mask], dtype=torch.int64, device=dev), test, B=B, seed=seed, alpha=alpha,
                   test_offset=test_offset, return_used=return_used)
    return (got[0][0], got[1][0]) if return_used else got[0]


def level_tests(adj: List[int], level: int):
    """The pairs of a PC-stable level and where their tests start: (pair_xy [[x, y], ...] with x < y adjacent and at least one
    test, offsets [P + 1]) for the adjacency rows ``adj`` (Python ints) — the host half of dvs_pc_expand."""
    n = len(adj)
    pair_xy, offsets = [], [0]
    for x in range(n):
        for y in range(x + 1, n):
            if not (adj[x] >> y) & 1:
                continue
            kx, ky = bin(adj[x] & ~(1 << y)).count("1"), bin(adj[y] & ~(1 << x)).count("1")
            count = 1 if level == 0 else comb(kx, level) + comb(ky, level)
            if count:
                pair_xy.append([x, y])
                offsets.append(offsets[-1] + count)
    return pair_xy, offsets


def pc_stable(evaluator, *, alpha: float = 0.05, test: str = "mi", max_cond: Optional[int] = None, chunk: int = 65536,
              B: int = 5000, seed: int = 0) -> PCResult:
    """The PC-stable algorithm (Colombo and Maathuis 2014) on the evaluator's data set: the skeleton by levels of conditional
    independence tests of growing conditioning-set size, every level working on the adjacency rows frozen at its start, then
    colliders from the separating sets and Meek's rules.  ``max_cond`` caps the size of the conditioning sets (None: no cap,
    the search stops at the first level where no adjacent pair has enough neighbours left).  ``chunk``: tests per launch.
    With a permutation ``test`` (``ci_tests``), ``B`` permutations per test are drawn from ``seed``, ``alpha`` is also the
    ``smc-`` tests' stopping threshold, and the tests are numbered on across the levels (test t of a level draws as global test
    ``tests of the earlier levels + t``), so the result is a function of the seed alone, not of ``chunk``.
    On a ``GaussianEvaluator`` ``test`` is "cor", "zf" or "mi-g" (``ci_tests``); ``max_cond`` may exceed
    ``_lib.GCI_MAX_COND``: the tests beyond it come back refused and are counted in ``refused``, never as independence."""
    what = "pc_stable"
    typ = _test_type(test)
    card = _evaluator(what, evaluator, test)
    _one_set(what, evaluator)
    if not 0.0 <= float(alpha) <= 1.0:
        raise ValueError("alpha must be in [0, 1]")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    if max_cond is not None and int(max_cond) < 0:
        raise ValueError("max_cond must be >= 0 or None")
    perm = _Perm.of(what, test, B, seed, alpha) if test in dl.CI_PERM_TYPES else None
    dev, n, lib, p = evaluator.device, evaluator.n_vars, evaluator.lib, dl.ptr
    full = (1 << n) - 1
    adj = [full & ~(1 << v) for v in range(n)]
    tests_per_level, refused_total = [], 0

    def dev_u64(values):
        return torch.from_numpy(np.array(values, np.uint64).view(np.int64)).to(dev)

    with torch.cuda.device(dev):
        sepsets = torch.zeros(n, n, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        refused = torch.zeros(1, dtype=torch.int32, device=dev)
        level = 0
        while max_cond is None or level <= int(max_cond):
            pair_xy, offsets = level_tests(adj, level)
            T = offsets[-1]
            if T == 0:
                break
            if T > INDEX_RANGE:
                raise ValueError(f"{what}: level {level} has {T:,} tests, beyond the index range of one level ({INDEX_RANGE:,}): "
                                 f"set max_cond below {level}")
            P = len(pair_xy)
            d_adj, d_next = dev_u64(adj), torch.empty(n, dtype=torch.int64, device=dev)
            d_xy = torch.tensor(pair_xy, dtype=torch.int32, device=dev)
            d_off = torch.tensor(offsets, dtype=torch.int64, device=dev)
            pairs = torch.empty(T, 2, dtype=torch.int32, device=dev)
            cond = torch.empty(T, dtype=torch.int64, device=dev)
            out = torch.empty(T, 3, dtype=torch.float64, device=dev)
            result = torch.empty(P, 2, dtype=torch.int64, device=dev)
            dl.check(lib, lib.dvs_pc_expand(P, n, level, p(d_adj), p(d_xy), p(d_off), T, p(pairs), p(cond), T * 8, dl.stream()),
                     "dvs_pc_expand")
            _run_tests(evaluator, pairs, cond, typ, 0 if card is None else _max_cells(card, level), out, status, chunk,
                       perm and perm._replace(test_offset=sum(tests_per_level) & 0xFFFFFFFF))
            dl.check(lib, lib.dvs_pc_reduce(P, n, p(d_xy), p(d_off), T, p(cond), p(out), float(alpha), p(d_adj), p(d_next),
                                            p(sepsets), n * n * 8, p(result), P * 16, p(refused), dl.stream()), "dvs_pc_reduce")
            adj = [int(a) for a in d_next.cpu().numpy().view(np.uint64)]        # the level's one read-back
            refused_total += int(refused.cpu()[0])
            tests_per_level.append(T)
            level += 1
        skeleton = dev_u64(adj)
        pdag = torch.empty(n, dtype=torch.int64, device=dev)
        conflicts = torch.empty(1, dtype=torch.int32, device=dev)
        flags = torch.empty(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_pc_orient(1, n, p(skeleton), p(sepsets), n * n * 8, p(pdag), n * 8, p(conflicts), p(flags),
                                        dl.stream()), "dvs_pc_orient")
        conflicts, flags = int(conflicts.cpu()[0]), int(flags.cpu()[0])
    return PCResult(pdag, skeleton, sepsets, tests_per_level, refused_total, conflicts, flags)


def skeleton_blacklist(skeleton: torch.Tensor) -> torch.Tensor:
    """int64 [n] adjacency rows on the device -> the ``forbidden`` rows of ``hill_climb``, ``tabu_search`` and
    ``exact_search``: bit u of row v is set for every u != v that is not adjacent to v, so a search keeps to the skeleton."""
    what = "skeleton_blacklist"
    if not torch.is_tensor(skeleton):
        raise TypeError(f"{what}: skeleton must be a torch tensor of adjacency rows")
    dl.need_cuda(what, skeleton.device)
    if skeleton.dtype != torch.int64 or skeleton.ndim != 1 or not 1 <= skeleton.shape[0] <= MAX_VARS:
        raise ValueError(f"{what}: skeleton must be int64 [n <= 48] adjacency rows")
    n = skeleton.shape[0]
    own = torch.ones(n, dtype=torch.int64, device=skeleton.device) << torch.arange(n, dtype=torch.int64, device=skeleton.device)
    return (~skeleton & ((1 << n) - 1) & ~own).contiguous()
