"""Conditional Gaussian networks on data sets that hold factors and real columns (csrc/dvs_mixed.h).

The reference hands ``metric_name`` to ``bnlearn::score`` unseen; on a mixed data frame that means ``loglik-cg``, ``aic-cg`` and
``bic-cg``.  ``MixedEvaluator`` is their evaluator.  A discrete variable takes discrete parents only and is scored as
``BNLearnWrapper`` scores it (``loglik`` / ``aic`` / ``bic``, equal bytes); a continuous variable has one linear regression on
its continuous parents for every configuration of its discrete parents D.  What the scorer reads for D is a *table*: the
moments of the real columns of every configuration (``dvs_cg_partition`` sorts the rows by configuration, ``dvs_cg_moments`` runs
``dvs_gbn_moments``' summation over every segment).  The evaluator keeps tables in a cache keyed by D under a byte budget
(``table_bytes=``, default 1 GiB): a pass collects its distinct masks (``torch.unique``), reads them back (the cache's one
synchronisation per pass), builds the misses and hands the kernels a table index per cell.

It is an ``Evaluator`` (evaluator.py), so ``hill_climb`` and ``tabu_search`` run on it unchanged: a continuous -> discrete arc is a NaN toggle cell, which the move
selection treats as "not available"; ``illegal`` holds the same arcs as ``forbidden=`` rows.  ``cg_fit`` gives the parameters of
a structure (``dvs_cg_fit``, and ``bn_fit`` on the discrete columns).  What is done with the fitted network (csrc/dvs_mixed_params.h,
DESIGN.md §33): ``cg_sample`` draws mixed rows (bnlearn's ``rbn``), ``cg_log_likelihood`` scores rows the parameters were not
fitted on (``logLik``), ``cg_predict`` predicts a real column or a class (``predict``) and ``cg_cross_validate`` composes them
(``bn.cv``); the discrete half of each is the discrete entry point on ``fitted.discrete``, the continuous half one ``dvs_cgbn_*``
call.  Not built on mixed data, each raising ``ValueError`` that says so: ``with_rows`` / ``boot_strength``, ``exact_search``,
``arc_posterior``, ``order_mcmc``, ``bn_fit``, ``gaussian_fit``, the CI-test family, ``cross_validate`` (the discrete one) and
``available_case``; nor are a batch of CG networks per call, likelihood weighting on a ``FittedCGBN`` and incomplete mixed data.

The definitions are those of include/dvs_mixed.h.  Three things follow bnlearn as recalled and are unpinned against an R run:
the unbiased residual variance of every configuration, the parameter count q (p + 2), and the treatment of sparse
configurations (an empty one adds nothing and counts in q; one with 1 .. p + 1 rows refuses the family).  Parity of the four
functions on a fitted network with bnlearn's ``rbn``, ``logLik``, ``predict`` and ``bn.cv`` on mixed data is unpinned as well.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib as dl
from .bic import BNLearnWrapper
from .evaluator import Evaluator, check_k, pack_levels, score_arg
from .gaussian import load_real_csv

PENALISED = ("aic-cg", "bic-cg")           # take k
DISCRETE_METRIC = {"loglik-cg": "loglik", "aic-cg": "aic", "bic-cg": "bic"}      # what a discrete node's cell is, as bytes


def _kinds(discrete, n):
    """``discrete``: n entries (a level count 1..16 for a factor; 0 or None for a real column) or {column: level count} -> [n] ints"""
    if isinstance(discrete, dict):
        if any(not 0 <= int(c) < n for c in discrete):
            raise ValueError(f"discrete names a column outside [0, {n})")
        card = [int(discrete.get(i, 0) or 0) for i in range(n)]
    else:
        card = [int(c or 0) for c in discrete]
    if len(card) != n or any(not 0 <= c <= 16 for c in card):
        raise ValueError(f"discrete must give {n} entries: a level count in 1..16 for a factor, 0 for a real column")
    return card


class MixedEvaluator(Evaluator):
    """``packed`` (int64 [S, ceil(n / 16)]: the level codes of the factors), ``x`` (f64 [S, n_cont]: the real columns in ascending
    variable order) and ``card`` (uint8 [n]: a factor's level count, 0 for a real column) are the data set."""
    data_kind = "mixed"

    def __init__(self, dataset_name: str, metric_name: str = "bic-cg", data=None, discrete=None, device="cuda", *, k=None,
                 table_bytes: int = 1 << 30):
        """``data``: path of a CSV with a header row, or a real array [S, n <= 48] whose factor columns hold level codes 0 ..
        levels - 1.  ``discrete``: n entries, a level count (1..16) for a factor and 0 for a real column, or {column: level
        count}.  ``metric_name``: ``loglik-cg``, ``aic-cg`` or ``bic-cg``; ``k``: the penalty coefficient of aic-cg (default 1) /
        bic-cg (default log(S) / 2).  ``table_bytes``: the budget of the table cache."""
        if data is None or discrete is None:
            raise ValueError("pass data=<csv path or real array [S, n]> and discrete=<level counts, 0 for a real column>")
        arr = load_real_csv(data)[1] if isinstance(data, str) else np.asarray(data)
        if arr.ndim != 2 or arr.shape[0] < 1 or not 1 <= arr.shape[1] <= dl.MAX_TOKENS or arr.dtype.kind not in "fiu":
            raise ValueError("data must be a real array [samples >= 1, 1 <= n_vars <= 48]")
        n = arr.shape[1]
        card = _kinds(discrete, n)
        dcols = [v for v in range(n) if card[v]]
        ccols = [v for v in range(n) if not card[v]]
        codes = arr[:, dcols]
        if dcols and (not np.array_equal(codes, np.floor(codes)) or codes.min() < 0 or (codes.max(0) >= np.asarray([card[v] for v in dcols])).any()):
            raise ValueError("a factor column must hold integer level codes in [0, its level count)")
        device = torch.device(device)
        dl.need_cuda("MixedEvaluator", device)
        self._set_score(dataset_name, metric_name, k, table_bytes)
        packed = torch.from_numpy(pack_levels(codes.astype(np.int64), dcols, n)).to(device)
        x = torch.from_numpy(np.array(arr[:, ccols], np.float64, order="C")).to(device)
        self._set_data(packed, x, card)

    @classmethod
    def from_device(cls, dataset_name: str, metric_name: str, packed: torch.Tensor, x: Optional[torch.Tensor], card, *, k=None,
                    table_bytes: int = 1 << 30):
        """An evaluator around rows that are already on the device: ``packed`` int64 [S, ceil(n / 16)] (the nibbles of real
        columns are not read), ``x`` float64 or float32 [S, n_cont] (None without real columns), ``card`` as ``discrete``."""
        card = _kinds(card, len(card))
        n, nc = len(card), sum(1 for c in card if not c)
        if not torch.is_tensor(packed) or packed.device.type != "cuda":
            raise RuntimeError("dags_vae_search_amd: from_device takes rows on the GPU; this package has no CPU path")
        if not 1 <= n <= dl.MAX_TOKENS or packed.dtype != torch.int64 or packed.ndim != 2 or packed.shape[0] < 1 or packed.shape[1] != (n + 15) // 16:
            raise ValueError(f"packed must be int64 [S >= 1, {(n + 15) // 16}] for {n} variables")
        S = packed.shape[0]
        if x is None:
            x = torch.empty(S, 0, dtype=torch.float64, device=packed.device)
        if not torch.is_tensor(x) or x.device != packed.device or x.dtype not in (torch.float32, torch.float64) or tuple(x.shape) != (S, nc):
            raise ValueError(f"x must be float64 or float32 [{S}, {nc}] on {packed.device}")
        self = cls.__new__(cls)
        self._set_score(dataset_name, metric_name, k, table_bytes)
        self._set_data(packed.contiguous(), x.to(torch.float64).contiguous(), card)
        return self

    def _set_score(self, dataset_name, metric_name, k, table_bytes):
        if metric_name not in dl.CGSCORE_TYPES:
            raise NotImplementedError(f"built mixed-data scores: {', '.join(sorted(dl.CGSCORE_TYPES))} (got {metric_name!r})")
        check_k(k, metric_name, PENALISED)
        if int(table_bytes) < 1:
            raise ValueError("table_bytes must be >= 1")
        self.dataset_name, self.metric_name, self.k = dataset_name, metric_name, k
        self.score_arg, self.table_bytes = score_arg(k), int(table_bytes)

    def _set_data(self, packed, x, card):
        self.lib, self.device, self.packed, self.x = dl.load(), packed.device, packed, x
        self.n_samples, self.n_vars, self.n_cont = int(packed.shape[0]), len(card), int(x.shape[1])
        self.card_host = card
        self.kind = ["discrete" if c else "continuous" for c in card]
        self.disc_mask = sum(1 << v for v in range(self.n_vars) if card[v])
        self.cont_mask = sum(1 << v for v in range(self.n_vars) if not card[v])
        self._cache: "OrderedDict[int, torch.Tensor]" = OrderedDict()
        self._cached_bytes = 0
        self.cache_stats = {"passes": 0, "hits": 0, "misses": 0, "built": 0, "evicted": 0}
        with torch.cuda.device(self.device):
            dev = self.device
            self.card = torch.tensor(card, dtype=torch.uint8, device=dev)
            self.illegal = torch.tensor([self.cont_mask if c else 0 for c in card], dtype=torch.int64, device=dev)
            self._is_cont = torch.tensor([not c for c in card], dtype=torch.bool, device=dev)
            # bit u for a discrete u, 0 for a continuous one: what flipping u does to a family's D
            self._flip = torch.tensor([(1 << v) if card[v] else 0 for v in range(self.n_vars)], dtype=torch.int64, device=dev)

    # ---- tables ------------------------------------------------------------------------------------------------------------
    def configurations(self, mask: int) -> int:
        """q of the set D = ``mask`` of discrete variables: the product of their level counts"""
        q = 1
        for v in range(self.n_vars):
            if (mask >> v) & 1:
                q *= self.card_host[v]
        return q

    def _table_nbytes(self, q):
        return q * dl.gbn_stride(self.n_cont) * 8

    def build_tables(self, masks: List[int]) -> List[torch.Tensor]:
        """dvs_cg_partition + dvs_cg_moments for the sets ``masks`` (each within ``_lib.CG_MAX_CONFIGS`` configurations) ->
        their tables f64 [q, stride], each its own allocation.  The requests run in launches of equal q_pitch whose buffers
        stay within a quarter of the budget."""
        lib, p, dev, S, nc = self.lib, dl.ptr, self.device, self.n_samples, self.n_cont
        stride = dl.gbn_stride(nc)
        order_of = sorted(range(len(masks)), key=lambda i: self.configurations(masks[i]))
        out: List[Optional[torch.Tensor]] = [None] * len(masks)
        at = 0
        while at < len(order_of):
            # the requests are sorted by q: a launch takes requests while its buffers at the last one's pitch stay in the slice
            take = 1
            while at + take < len(order_of):
                pitch = self.configurations(masks[order_of[at + take]])
                per = pitch * stride * 8 + 8 * pitch + 4 * S + ((S + dl.GBN_CHUNK - 1) // dl.GBN_CHUNK + pitch) * (nc + nc * (nc + 1) // 2) * 8
                slots, tri = (S + dl.GBN_CHUNK - 1) // dl.GBN_CHUNK + pitch, nc * (nc + 1) // 2
                if (take + 1) * per > max(self.table_bytes // 4, per) or (take + 1) * max(pitch, S, slots * tri) >= 1 << 30:
                    break                                    # the buffers' slice of the budget; the index ranges of the two calls
                take += 1
            mine = order_of[at:at + take]
            at += take
            pitch = self.configurations(masks[mine[-1]])
            R = len(mine)
            req = torch.tensor([masks[i] for i in mine], dtype=torch.int64, device=dev)
            count = torch.empty(R, pitch, dtype=torch.int32, device=dev)
            start = torch.empty(R, pitch, dtype=torch.int32, device=dev)
            order = torch.empty(R, S, dtype=torch.int32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            dl.check(lib, lib.dvs_cg_partition(self.n_vars, S, p(self.packed), p(self.card), R, p(req), pitch, p(count), dl.nbytes(count),
                                               p(start), p(order), dl.nbytes(order), p(status), dl.stream()), "dvs_cg_partition")
            ws = torch.empty(dl.workspace_bytes(lib, "dvs_cg_moments_workspace_bytes", nc, S, R, pitch), dtype=torch.uint8, device=dev)
            mom = torch.empty(R, pitch, stride, dtype=torch.float64, device=dev)
            dl.check(lib, lib.dvs_cg_moments(nc, S, p(self.x), R, pitch, p(count), p(start), p(order), p(ws), dl.nbytes(ws), p(mom),
                                             dl.nbytes(mom), dl.stream()), "dvs_cg_moments")
            for j, i in enumerate(mine):
                out[i] = mom[j, :self.configurations(masks[i])].clone()
        self.cache_stats["built"] += len(masks)
        return out

    def tables_of(self, cell_masks: torch.Tensor):
        """``cell_masks``: int64, the set D of every continuous family a pass scores, -1 where no table is read -> (tables int64
        [T] device addresses, table_of int32 like cell_masks; -1: none, or D beyond ``_lib.CG_MAX_CONFIGS`` configurations:
        refused on the device).  Reads the distinct masks back: the pass's one synchronisation."""
        dev = self.device
        uniq = torch.unique(cell_masks)
        host = [int(m) for m in uniq.cpu().tolist()]
        self.cache_stats["passes"] += 1
        wanted = [m for m in host if m >= 0 and self.configurations(m) <= dl.CG_MAX_CONFIGS]
        misses = [m for m in wanted if m not in self._cache]
        self.cache_stats["hits"] += len(wanted) - len(misses)
        self.cache_stats["misses"] += len(misses)
        need = sum(self._table_nbytes(self.configurations(m)) for m in wanted)
        if need > self.table_bytes:
            raise ValueError(f"MixedEvaluator: the {len(wanted)} tables of one pass take {need:,} bytes, beyond table_bytes = "
                             f"{self.table_bytes:,}: raise the budget or score fewer structures per call")
        for m in wanted:
            if m in self._cache:
                self._cache.move_to_end(m)
        incoming = sum(self._table_nbytes(self.configurations(m)) for m in misses)
        keep = set(wanted)
        for m in list(self._cache):
            if self._cached_bytes + incoming <= self.table_bytes:
                break
            if m not in keep:
                self._cached_bytes -= dl.nbytes(self._cache.pop(m))
                self.cache_stats["evicted"] += 1
        if misses:
            for m, t in zip(misses, self.build_tables(misses)):
                self._cache[m] = t
                self._cached_bytes += dl.nbytes(t)
        slot, addresses = {}, []
        for m in wanted:
            slot[m] = len(addresses)
            addresses.append(self._cache[m].data_ptr())
        tables = torch.tensor(addresses or [0], dtype=torch.int64, device=dev)
        lookup = torch.tensor([slot.get(m, -1) for m in host], dtype=torch.int32, device=dev)
        return tables, lookup[torch.searchsorted(uniq, cell_masks)].contiguous()

    def clear_cache(self):
        self._cache.clear()
        self._cached_bytes = 0

    def _family_masks(self, parents):
        """D of every family [B, n]; -1 on the rows of discrete variables"""
        return torch.where(self._is_cont[None, :], parents & self.disc_mask, torch.full_like(parents, -1))

    def _score_args(self):
        return dl.CGSCORE_TYPES[self.metric_name], self.score_arg

    # ---- the scorer's surface ------------------------------------------------------------------------------------------------
    def _launch_scores(self, parents, scratch, out, status, used):
        B, n, lib, p = parents.shape[0], self.n_vars, self.lib, dl.ptr
        tables = table_of = None
        if self.n_cont:
            tables, table_of = self.tables_of(self._family_masks(parents))
        ws = torch.empty(dl.workspace_bytes(lib, "dvs_cg_scores_workspace_bytes", B, n), dtype=torch.uint8, device=self.device)
        dl.check(lib, lib.dvs_cg_scores(B, n, self.n_cont, self.n_samples, p(self.packed), p(self.card), p(tables), p(table_of),
                                        p(parents), *self._score_args(), p(ws), dl.nbytes(ws), p(scratch), p(out), p(status),
                                        dl.stream()), "dvs_cg_scores")

    def _refusal(self, scratch):
        bad = torch.nonzero(torch.isnan(scratch)).cpu().tolist()
        return (f"refused families (structure, variable): {bad[:8]}: "
                f"a continuous parent of a discrete variable, more than {dl.CG_MAX_CONFIGS} configurations of the discrete parents, "
                f"more than {dl.GBN_MAX_PARENTS} continuous parents, a parent bit >= {self.n_vars}, a configuration with 1 .. p + 1 "
                f"rows, a Cholesky pivot within rounding of zero (a duplicated or collinear column) in some configuration, or a "
                f"discrete family the counting paths cannot hold")

    def _launch_toggles(self, parents, worklist, L, T, status):
        """dvs_cg_toggle_scores; a cell (v, u) with a discrete v and a continuous u is NaN: the move is not available"""
        (B, n), lib, p = parents.shape, self.lib, dl.ptr
        tables = table_of = None
        if self.n_cont:
            if worklist is None:
                D = self._family_masks(parents).reshape(B * n)
            else:
                wl = worklist.to(torch.int64)
                v = wl.clamp(0, n - 1)
                rows = parents[torch.arange(2 * B, device=self.device) // 2, v]
                live = (wl >= 0) & (wl < n) & self._is_cont[v]
                D = torch.where(live, rows & self.disc_mask, torch.full_like(rows, -1))
            cells = torch.where(D[:, None] >= 0, D[:, None] ^ self._flip[None, :], D[:, None].expand(-1, n))
            tables, table_of = self.tables_of(cells.contiguous())
        ws = torch.empty(dl.workspace_bytes(lib, "dvs_cg_toggle_workspace_bytes", B, n), dtype=torch.uint8, device=self.device)
        dl.check(lib, lib.dvs_cg_toggle_scores(B, n, self.n_cont, self.n_samples, p(self.packed), p(self.card), p(tables),
                                               p(table_of), p(parents), *self._score_args(), p(worklist), p(ws), dl.nbytes(ws),
                                               p(L), L.numel() * 8, p(T), T.numel() * 8, p(status), dl.stream()),
                 "dvs_cg_toggle_scores")

    def with_rows(self, *args, **kwargs):
        dl.need_unmixed("with_rows / boot_strength", self)

    def available_case(self, *args, **kwargs):
        dl.need_unmixed("available_case", self)


@dataclass
class FittedCGBN:
    parents: torch.Tensor                  # int64 [n]: the structure
    kind: List[str]                        # "discrete" / "continuous" per variable
    card: List[int]                        # a factor's level count, 0 for a real column
    coef: List[Optional[torch.Tensor]]     # per continuous v: f64 [q_v, n], coef[v][z, u] the coefficient of u in configuration z, 0 off the continuous parents
    intercept: List[Optional[torch.Tensor]]    # per continuous v: f64 [q_v]
    sd: List[Optional[torch.Tensor]]       # per continuous v: f64 [q_v], sqrt(RSS_z / (m_z - p - 1))
    count: List[Optional[torch.Tensor]]    # per continuous v: f64 [q_v], the rows of every configuration
    discrete: object                       # params.FittedBN over the discrete columns in ascending order (None without factors)
    discrete_vars: List[int]               # the variable of every column of ``discrete``
    # the layout of include/dvs_mixed_params.h, kept so that nothing is concatenated per call (None: built on first use)
    offset: Optional[torch.Tensor] = None          # int64 [n + 1]: the exclusive prefix of q_v, 0 for a discrete v
    coef_flat: Optional[torch.Tensor] = None       # f64 [cells, n]: the rows of ``coef`` in ascending variable order
    intercept_flat: Optional[torch.Tensor] = None  # f64 [cells]
    sd_flat: Optional[torch.Tensor] = None         # f64 [cells]

    @property
    def n_vars(self) -> int:
        return len(self.card)

    @property
    def continuous_vars(self) -> List[int]:
        return [v for v, c in enumerate(self.card) if not c]

    def flat(self):
        """(card uint8 [n], offset int64 [n + 1], coef [cells, n], intercept [cells], sd [cells]) on the device"""
        dev = self.parents.device
        if self.offset is None:
            qs = [0 if c else int(self.sd[v].shape[0]) for v, c in enumerate(self.card)]
            self.offset = torch.tensor(np.concatenate([[0], np.cumsum(qs)]).astype(np.int64), device=dev)
            cv = self.continuous_vars
            self.coef_flat = torch.cat([self.coef[v].reshape(-1, self.n_vars) for v in cv]).contiguous()
            self.intercept_flat = torch.cat([self.intercept[v].reshape(-1) for v in cv]).contiguous()
            self.sd_flat = torch.cat([self.sd[v].reshape(-1) for v in cv]).contiguous()
        if getattr(self, "_card_dev", None) is None:
            self._card_dev = torch.tensor(self.card, dtype=torch.uint8, device=dev)
        return self._card_dev, self.offset, self.coef_flat, self.intercept_flat, self.sd_flat

    @classmethod
    def from_parameters(cls, parents: Sequence[int], card: Sequence[int], coef, intercept, sd, tables, device="cuda") -> "FittedCGBN":
        """A hand-written network.  ``parents``: n parent masks (ints); ``card``: a factor's level count, 0 for a real column;
        ``coef[v]`` [q_v, n], ``intercept[v]`` and ``sd[v]`` [q_v] for a real v (None for a factor), configuration z of the
        discrete parents with the lowest variable id fastest, ``coef[v][z, u]`` read at the real parents u; a configuration
        whose sd is NaN is empty.  ``tables[v]``: the [q, r] table of a factor v (None for a real column), rows the
        configurations of its parents.  A ``ValueError`` names the rule a network breaks."""
        what = "FittedCGBN.from_parameters"
        dl.need_cuda(what, device)
        dev = torch.device(device)
        card = _kinds(card, len(card))
        n = len(card)
        host = [int(m) & ~(1 << v) for v, m in enumerate(parents)]
        if not 1 <= n <= dl.MAX_TOKENS or len(host) != n or any(len(a) != n for a in (coef, intercept, sd, tables)):
            raise ValueError(f"{what}: parents, card, coef, intercept, sd and tables must have one entry per variable (1 .. 48)")
        dvars = [v for v in range(n) if card[v]]
        cvars = [v for v in range(n) if not card[v]]
        cont_mask = sum(1 << v for v in cvars)
        cf: List[Optional[torch.Tensor]] = [None] * n
        ic, s0, cnt = list(cf), list(cf), list(cf)
        for v, m in enumerate(host):
            if m >> n or m < 0:
                raise ValueError(f"{what}: variable {v} has a parent bit >= {n}")
            if card[v] and m & cont_mask:
                raise ValueError(f"{what}: the discrete variable {v} has a continuous parent")
            if card[v]:
                continue
            q = int(np.prod([card[u] for u in range(n) if (m >> u) & 1 and card[u]], dtype=np.int64))
            if q > dl.CG_MAX_CONFIGS:
                raise ValueError(f"{what}: variable {v} has {q} configurations of its discrete parents, beyond {dl.CG_MAX_CONFIGS}")
            c, i, s = (np.asarray(a[v], np.float64) for a in (coef, intercept, sd))
            if c.shape != (q, n) or i.shape != (q,) or s.shape != (q,):
                raise ValueError(f"{what}: variable {v} needs coef [{q}, {n}], intercept [{q}] and sd [{q}] (got {c.shape}, {i.shape}, {s.shape})")
            live = ~np.isnan(s)
            pa = [u for u in cvars if (m >> u) & 1]
            if not (np.isfinite(i[live]).all() and np.isfinite(s[live]).all() and (s[live] > 0).all() and np.isfinite(c[live][:, pa]).all()):
                raise ValueError(f"{what}: variable {v} has a non-empty configuration whose intercept, sd or a coefficient at a "
                                 f"continuous parent is not finite, or whose sd is not > 0")
            cf[v], ic[v], s0[v] = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (c, i, s))
        placed, left = 0, set(range(n))
        while left:
            free = [v for v in sorted(left) if not host[v] & ~placed]
            if not free:
                raise ValueError(f"{what}: the structure has a cycle")
            placed |= 1 << free[0]
            left.remove(free[0])
        fitted = None
        if dvars:
            from .params import FittedBN
            rank = {v: j for j, v in enumerate(dvars)}
            fitted = FittedBN.from_tables([sum(1 << rank[u] for u in dvars if (host[v] >> u) & 1) for v in dvars],
                                          [card[v] for v in dvars], [tables[v] for v in dvars], device=dev)
        return cls(torch.tensor(np.asarray(host, np.uint64).view(np.int64), device=dev), ["discrete" if c else "continuous" for c in card],
                   card, cf, ic, s0, cnt, fitted, dvars)


def cg_fit(evaluator: MixedEvaluator, parents: torch.Tensor) -> FittedCGBN:
    """bnlearn's ``bn.fit`` on a conditional Gaussian network: ``parents`` int64 [n] parent masks -> for every continuous
    variable one regression per configuration of its discrete parents (dvs_cg_fit: NaN in an empty configuration), for the
    discrete ones the tables of ``bn_fit`` on the discrete columns.  A refusal raises ``ValueError`` naming (variable,
    configuration)."""
    from .params import bn_fit
    what = "cg_fit"
    if not isinstance(evaluator, MixedEvaluator):
        raise ValueError(f"{what}: takes a MixedEvaluator (bn_fit and gaussian_fit fit discrete and real-valued data)")
    ev, n, dev = evaluator, evaluator.n_vars, evaluator.device
    if not torch.is_tensor(parents) or parents.dtype != torch.int64 or tuple(parents.shape) != (n,):
        raise ValueError(f"{what}: parents must be an int64 tensor [{n}] of parent masks")
    host = [int(m) & ~(1 << v) for v, m in enumerate(parents.cpu().tolist())]
    for v, m in enumerate(host):
        if m >> n or m < 0:
            raise ValueError(f"{what}: variable {v} has a parent bit >= {n}")
        if ev.card_host[v] and m & ev.cont_mask:
            raise ValueError(f"{what}: the discrete variable {v} has a continuous parent")
    cvars = [v for v in range(n) if not ev.card_host[v]]
    dvars = [v for v in range(n) if ev.card_host[v]]
    coef: List[Optional[torch.Tensor]] = [None] * n
    icpt, sd, cnt = list(coef), list(coef), list(coef)
    flat = {}
    with torch.cuda.device(dev):
        if cvars:
            qs = [ev.configurations(host[v] & ev.disc_mask) for v in cvars]
            for v, q in zip(cvars, qs):
                if q > dl.CG_MAX_CONFIGS:
                    raise ValueError(f"{what}: variable {v} has {q} configurations of its discrete parents, beyond {dl.CG_MAX_CONFIGS}")
            masks = torch.tensor([host[v] & ev.disc_mask for v in cvars], dtype=torch.int64, device=dev)
            tables, table_of = ev.tables_of(masks)
            offset = np.concatenate([[0], np.cumsum(qs)]).astype(np.int64)
            cells, F, p = int(offset[-1]), len(cvars), dl.ptr
            var = torch.tensor(cvars, dtype=torch.int32, device=dev)
            par = torch.tensor([host[v] for v in cvars], dtype=torch.int64, device=dev)
            table = tables[table_of.to(torch.int64)].contiguous()
            off = torch.from_numpy(offset).to(dev)
            c = torch.empty(cells, n, dtype=torch.float64, device=dev)
            i0, s0, m0 = (torch.empty(cells, dtype=torch.float64, device=dev) for _ in range(3))
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            dl.check(ev.lib, ev.lib.dvs_cg_fit(F, cells, n, ev.n_cont, p(ev.card), p(var), p(par), p(table), p(off), p(c), dl.nbytes(c),
                                               p(i0), p(s0), p(m0), p(status), dl.stream()), "dvs_cg_fit")
            if int(status.item()) & dl.STATUS_REFUSED:
                bad_cells = torch.nonzero(torch.isnan(s0) & (m0 != 0)).flatten().cpu().tolist()
                bad = [(cvars[int(np.searchsorted(offset, b, side="right")) - 1], int(b - offset[int(np.searchsorted(offset, b, side="right")) - 1]))
                       for b in bad_cells]
                raise ValueError(f"{what}: refused (variable, configuration): {bad[:8]}: more than {dl.GBN_MAX_PARENTS} continuous "
                                 f"parents, a configuration with 1 .. p + 1 rows, or collinear columns in that configuration")
            for j, v in enumerate(cvars):
                a, b = int(offset[j]), int(offset[j + 1])
                coef[v], icpt[v], sd[v], cnt[v] = c[a:b], i0[a:b], s0[a:b], m0[a:b]
            # dvs_cg_fit was given the continuous families in ascending variable order: its arrays are dvs_cgbn_*'s
            full_off = np.zeros(n + 1, np.int64)
            full_off[1:] = np.cumsum([qs[cvars.index(v)] if not ev.card_host[v] else 0 for v in range(n)])
            flat = dict(offset=torch.from_numpy(full_off).to(dev), coef_flat=c, intercept_flat=i0, sd_flat=s0)
        fitted = None
        if dvars:
            # the discrete columns as a data set of their own, in ascending variable order; repacked on the device and not
            # by evaluator.pack_levels, which would take the rows through the host
            sub = BNLearnWrapper.from_packed(ev.dataset_name, DISCRETE_METRIC[ev.metric_name], _sub_rows(ev.packed, dvars),
                                             [ev.card_host[v] for v in dvars])
            rank = {v: j for j, v in enumerate(dvars)}
            fitted = bn_fit(sub, torch.tensor([sum(1 << rank[u] for u in dvars if (host[v] >> u) & 1) for v in dvars],
                                              dtype=torch.int64, device=dev))
    return FittedCGBN(parents.to(dev), list(ev.kind), list(ev.card_host), coef, icpt, sd, cnt, fitted, dvars, **flat)


# ---- what is done with a fitted network (csrc/dvs_mixed_params.h) ----------------------------------------------
CG_CV_LOSSES = ("logl-cg", "mse", "mse-exact", "pred", "pred-exact")


def _sub_rows(packed, dvars):
    """the discrete columns ``dvars`` of packed rows as a data set of their own, in that order, on the device"""
    out = torch.zeros(packed.shape[0], (len(dvars) + 15) // 16, dtype=torch.int64, device=packed.device)
    for j, v in enumerate(dvars):
        out[:, j // 16] |= ((packed[:, v // 16] >> (4 * (v % 16))) & 15) << (4 * (j % 16))
    return out


def _spread_rows(sub, dvars, n):
    """the reverse: column j of ``sub`` becomes the nibble of variable dvars[j] among n; every other nibble is zero"""
    out = torch.zeros(sub.shape[0], (n + 15) // 16, dtype=torch.int64, device=sub.device)
    for j, v in enumerate(dvars):
        out[:, v // 16] |= ((sub[:, j // 16] >> (4 * (j % 16))) & 15) << (4 * (v % 16))
    return out


def _fitted(what, fitted):
    if not isinstance(fitted, FittedCGBN):
        raise ValueError(f"{what}: takes a FittedCGBN (cg_fit or FittedCGBN.from_parameters)")
    dl.need_cuda(what, fitted.parents.device)
    return fitted.n_vars, len(fitted.continuous_vars), fitted.parents.device


def _rows(what, fitted, data):
    """``data``: a MixedEvaluator or a (packed, x) pair over the network's variables -> (packed, x), contiguous"""
    n, nc, dev = _fitted(what, fitted)
    if isinstance(data, MixedEvaluator):
        if data.card_host != list(fitted.card):
            raise ValueError(f"{what}: the evaluator's kinds and level counts are not the network's")
        data = (data.packed, data.x)
    if not isinstance(data, (tuple, list)) or len(data) != 2:
        raise ValueError(f"{what}: data must be a MixedEvaluator or a (packed, x) pair")
    packed, x = data
    S = packed.shape[0] if torch.is_tensor(packed) and packed.ndim == 2 else -1
    if S < 1 or packed.dtype != torch.int64 or packed.shape[1] != (n + 15) // 16 or packed.device != dev:
        raise ValueError(f"{what}: packed must be int64 [S >= 1, {(n + 15) // 16}] on {dev}")
    if x is None and nc == 0:
        x = torch.empty(S, 0, dtype=torch.float64, device=dev)
    if not torch.is_tensor(x) or x.dtype != torch.float64 or tuple(x.shape) != (S, nc) or x.device != dev:
        raise ValueError(f"{what}: x must be float64 [{S}, {nc}] on {dev}")
    return packed.contiguous(), x.contiguous()


def _network_status(what, st, rows=False):
    """the refusals of include/dvs_mixed_params.h as ValueError; bit 7 (an empty configuration met: NaN) is information"""
    if st & dl.STATUS_CYCLE:
        raise ValueError(f"{what}: the structure has a cycle")
    if st & dl.STATUS_REFUSED:
        row = "a row has a level code at or above its variable's level count, or " if rows else ""
        raise ValueError(f"{what}: {row}the network breaks a rule: a parent bit at or above n_vars, a discrete variable with a "
                         f"continuous parent, a level count above 16, more than {dl.CG_MAX_CONFIGS} configurations of a variable's "
                         f"discrete parents, or parameter arrays that do not match the structure")
    if st & dl.STATUS_NOT_PROBABILITY:
        raise ValueError(f"{what}: a non-empty configuration has an intercept, an sd or a coefficient at a continuous parent that is "
                         f"not finite, or an sd that is not > 0")


def _net_args(fitted):
    card, offset, coef, icpt, sd = fitted.flat()
    p = dl.ptr
    return (fitted.n_vars, len(fitted.continuous_vars), int(sd.shape[0]), card, offset, coef, icpt, sd), \
        (p(card), p(fitted.parents), p(offset), p(coef), p(icpt), p(sd))


def cg_sample(fitted: FittedCGBN, n_rows: int, *, seed: int, row_offset: int = 0):
    """bnlearn's ``rbn`` on a conditional Gaussian network: ``n_rows`` rows -> (packed int64 [n_rows, ceil(n / 16)], x float64
    [n_rows, n_cont]) on the device, what ``MixedEvaluator.from_device`` takes.  The levels are, as bytes, ``sample(fitted.discrete,
    ...)`` spread to their variables' nibbles on the device; dvs_cgbn_sample then fills the real columns.  Row i is a function
    of (seed, row_offset + i) and the network alone, so a request may be cut into calls with consecutive ``row_offset``.  A
    row that meets an empty configuration (sd NaN) has NaN in that column and in what is computed from it."""
    from .params import sample
    what = "cg_sample"
    n, nc, dev = _fitted(what, fitted)
    if int(n_rows) < 1 or int(row_offset) < 0:
        raise ValueError(f"{what}: n_rows must be >= 1 and row_offset >= 0")
    S, lib, p = int(n_rows), dl.load(), dl.ptr
    with torch.cuda.device(dev):
        if fitted.discrete is not None:
            packed = _spread_rows(sample(fitted.discrete, S, seed=seed, row_offset=row_offset), fitted.discrete_vars, n)
        else:
            packed = torch.zeros(S, (n + 15) // 16, dtype=torch.int64, device=dev)
        x = torch.empty(S, nc, dtype=torch.float64, device=dev)
        if nc:
            (_, _, cells, *keep), net = _net_args(fitted)
            ws = torch.empty(dl.workspace_bytes(lib, "dvs_cgbn_sample_workspace_bytes", n), dtype=torch.uint8, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            dl.check(lib, lib.dvs_cgbn_sample(n, nc, S, cells, *net, p(packed), dl.seed64(seed), int(row_offset), p(ws), dl.nbytes(ws),
                                              p(x), p(status), dl.stream()), "dvs_cgbn_sample")
            _network_status(what, int(status.item()))
    return packed, x


def cg_log_likelihood(fitted: FittedCGBN, data, *, per_row: bool = False):
    """bnlearn's ``logLik(fitted, newdata)`` on a conditional Gaussian network: ``data`` a ``MixedEvaluator`` or a (packed, x)
    pair -> a float64 scalar on the device, with ``per_row`` (total, row terms [S]).  A row term is the discrete term
    (``log_likelihood`` on ``fitted.discrete``) plus the continuous term (dvs_cgbn_loglik), one addition; the total is the
    discrete total plus the continuous total, one addition: each half is summed by its own tree, so the total is NOT a tree
    over the summed row terms.  Without factors or without real columns only the half that applies runs.  A row that meets an
    empty configuration is NaN (and so is the total); a level code at or above its level count raises ValueError."""
    from .params import log_likelihood
    what = "cg_log_likelihood"
    n, nc, dev = _fitted(what, fitted)
    packed, x = _rows(what, fitted, data)
    S, lib, p = packed.shape[0], dl.load(), dl.ptr
    out = rows = None
    with torch.cuda.device(dev):
        if fitted.discrete is not None:
            got = log_likelihood(fitted.discrete, _sub_rows(packed, fitted.discrete_vars), per_row=per_row)
            out, rows = (got[0][0], got[1][0]) if per_row else (got[0], None)
        if nc:
            (_, _, cells, *keep), net = _net_args(fitted)
            ws = torch.empty(dl.workspace_bytes(lib, "dvs_cgbn_loglik_workspace_bytes", n, S, cells), dtype=torch.uint8, device=dev)
            crow = torch.empty(S, dtype=torch.float64, device=dev) if per_row else None
            cout = torch.empty(1, dtype=torch.float64, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            dl.check(lib, lib.dvs_cgbn_loglik(n, nc, S, cells, *net, p(packed), p(x), p(crow), p(cout), p(ws), dl.nbytes(ws), p(status),
                                              dl.stream()), "dvs_cgbn_loglik")
            _network_status(what, int(status.item()), rows=True)
            out = cout[0] if out is None else out + cout[0]
            if per_row:
                rows = crow if rows is None else rows + crow
    return (out, rows) if per_row else out


def cg_predict(fitted: FittedCGBN, target: int, data, *, method: str = "parents", prob: bool = False, var: bool = False):
    """bnlearn's ``predict`` on a conditional Gaussian network; the target's own column or nibble is never read.
    A real ``target``: float64 [S], from its parents (``method="parents"``: the conditional mean at the row's configuration) or
    given every other variable (``"exact"``: the closed form over the Markov blanket); with ``var`` (predictions, the
    conditional variance [S]).  A discrete ``target``: uint8 [S], with ``prob`` (predictions, posterior [S, levels]);
    ``"parents"`` is ``infer.predict`` on ``fitted.discrete``; ``"exact"`` takes that sub-network's exact posterior over the
    discrete Markov blanket as the prior of dvs_cgbn_predict's mode 2, which multiplies in the densities of the target's real
    children in the log domain (a target without real children returns the sub-network's answer as it is).  The lowest level
    wins a tie; a row whose posterior is NaN predicts 255; a row that meets an empty configuration is NaN / 255."""
    from . import infer
    what = "cg_predict"
    n, nc, dev = _fitted(what, fitted)
    if method not in ("parents", "exact"):
        raise ValueError(f"{what}: method must be 'parents' or 'exact' (got {method!r})")
    if not 0 <= int(target) < n:
        raise ValueError(f"{what}: target must be in [0, {n})")
    t = int(target)
    discrete = bool(fitted.card[t])
    if (prob and not discrete) or (var and discrete):
        raise ValueError(f"{what}: prob is the argument of a discrete target, var of a continuous one")
    packed, x = _rows(what, fitted, data)
    S, lib, p = packed.shape[0], dl.load(), dl.ptr
    with torch.cuda.device(dev):
        prior = None
        if discrete:
            rank = fitted.discrete_vars.index(t)
            sub = _sub_rows(packed, fitted.discrete_vars)
            host = [int(m) for m in fitted.parents.cpu().tolist()]
            kids = any((host[c] >> t) & 1 for c in fitted.continuous_vars)
            if method == "parents" or not kids:
                return infer.predict(fitted.discrete, rank, sub, method=method, prob=prob)
            _, prior = infer.predict(fitted.discrete, rank, sub, method="exact", prob=True)
            prior = prior.contiguous()
        (_, _, cells, *keep), net = _net_args(fitted)
        ws = torch.empty(dl.workspace_bytes(lib, "dvs_cgbn_predict_workspace_bytes", n, cells), dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        if discrete:
            pred = torch.empty(S, dtype=torch.uint8, device=dev)
            post = torch.empty(S, fitted.card[t], dtype=torch.float64, device=dev) if prob else None
            variance = None
            mode = dl.CGBN_PREDICT_MODES["class"]
        else:
            pred, variance, post = torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev), None
            mode = dl.CGBN_PREDICT_MODES[method]
        dl.check(lib, lib.dvs_cgbn_predict(n, nc, S, cells, *net, p(packed), p(x), t, mode, p(prior), p(pred), p(variance), p(post), p(ws),
                                           dl.nbytes(ws), p(status), dl.stream()), "dvs_cgbn_predict")
        _network_status(what, int(status.item()), rows=True)
    if discrete:
        return (pred, post) if prob else pred
    return (pred, variance) if var else pred


def cg_cross_validate(evaluator: MixedEvaluator, parents: torch.Tensor, *, folds: int = 10, seed: int = 0, loss: str = "logl-cg",
                      target=None) -> torch.Tensor:
    """bnlearn's ``bn.cv`` for one fixed structure on mixed data -> a float64 scalar on the device.  A composition, no kernel of
    its own: the rows are permuted (``params.cv_folds``), each part is held out in turn, the parameters are fitted on the rest
    (``MixedEvaluator.from_device`` and ``cg_fit``) and the part is scored; the parts' values are added in order and divided
    by the number of rows.  ``loss``: "logl-cg", minus the held-out ``cg_log_likelihood``; "mse" / "mse-exact", the squared
    error of ``cg_predict`` (method "parents" / "exact") for the real ``target``; "pred" / "pred-exact", the share of rows
    whose level of the discrete ``target`` is predicted wrongly (255 counts as wrong).  A part in which a held-out row meets a
    configuration the rest never showed is NaN under "logl-cg" and the mse losses, and so is the result; ``cg_fit``'s
    refusals (a configuration with 1 .. p + 1 training rows) are raised as they are."""
    from .params import cv_folds
    what = "cg_cross_validate"
    if not isinstance(evaluator, MixedEvaluator):
        raise ValueError(f"{what}: takes a MixedEvaluator (cross_validate and gaussian_cross_validate take discrete and real-valued data)")
    ev, S, n = evaluator, evaluator.n_samples, evaluator.n_vars
    if not 2 <= int(folds) <= S:
        raise ValueError(f"{what}: folds must be in [2, {S}]")
    if loss not in CG_CV_LOSSES:
        raise ValueError(f"{what}: loss must be one of {CG_CV_LOSSES} (got {loss!r})")
    if (loss == "logl-cg") != (target is None):
        raise ValueError(f"{what}: target is the argument of the prediction losses, and they need it")
    if target is not None:
        if not 0 <= int(target) < n:
            raise ValueError(f"{what}: target must be in [0, {n})")
        if bool(ev.card_host[int(target)]) != loss.startswith("pred"):
            raise ValueError(f"{what}: 'mse' and 'mse-exact' take a real target, 'pred' and 'pred-exact' a discrete one")
    method = "exact" if loss.endswith("-exact") else "parents"
    dev = ev.device
    with torch.cuda.device(dev):
        parts = [torch.from_numpy(p).to(dev) for p in cv_folds(S, int(folds), seed)]
        total = None
        for f, part in enumerate(parts):
            rest = torch.cat([p for g, p in enumerate(parts) if g != f])
            train = MixedEvaluator.from_device(ev.dataset_name, ev.metric_name, ev.packed[rest], ev.x[rest], ev.card_host, k=ev.k,
                                               table_bytes=ev.table_bytes)
            fitted = cg_fit(train, parents)
            held = (ev.packed[part].contiguous(), ev.x[part].contiguous())
            if loss == "logl-cg":
                value = cg_log_likelihood(fitted, held)
            else:
                t = int(target)
                pred = cg_predict(fitted, t, held, method=method)
                if loss.startswith("mse"):
                    err = pred - held[1][:, fitted.continuous_vars.index(t)]
                    value = (err * err).sum()
                else:
                    truth = ((held[0][:, t // 16] >> (4 * (t % 16))) & 15).to(torch.uint8)
                    value = (pred != truth).sum().to(torch.float64)
            total = value if total is None else total + value
    return (-total if loss == "logl-cg" else total) / torch.full_like(total, float(S))
