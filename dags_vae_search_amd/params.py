"""Parameters of a discrete Bayesian network on the device (csrc/dvs_params.h): bnlearn's ``bn.fit``, ``rbn``,
``logLik(fitted, newdata)`` and ``bn.cv`` next to the structure searches.

``bn_fit`` turns parent masks into conditional probability tables on the evaluator's data set, ``sample`` draws packed rows
from one fitted network, ``log_likelihood`` scores rows the tables were not fitted on, and ``cross_validate`` composes the three
into k-fold cross-validation.  ``BNLearnWrapper.from_packed`` closes the loop: a sample becomes an evaluator that every search
of this package accepts, without leaving the device.

The definitions are those of include/dvs.h (dvs_bn_fit, dvs_bn_sample, dvs_bn_loglik).  Parity with bnlearn rests on them and
is not pinned against an R run.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch

from . import _lib as dl
from .bic import BNLearnWrapper

UNOBSERVED = {"nan": 0, "uniform": 1}      # an unobserved parent configuration under mle: NaN cells, or 1 / r


def _family(card, row, v):
    """(q, r) of variable v under the parent row (a Python int); the self bit is ignored"""
    q = 1
    for u in range(len(card)):
        if u != v and (row >> u) & 1:
            q *= card[u]
    return q, card[v]


def _offsets(card, parents_host):
    n = len(card)
    off = [0]
    for row in parents_host:
        for v in range(n):
            if int(row[v]) >> n:
                raise ValueError(f"a parent row of variable {v} has a bit at or above n_vars = {n}")
            q, r = _family(card, int(row[v]), v)
            off.append(off[-1] + q * r)
    return off


class FittedBN:
    """The conditional probability tables of a batch of structures over one set of variables, on the device.

    ``parents`` int64 [B, n] (bit u of [b, v] <=> u -> v), ``card`` uint8 [n], ``offsets`` int64 [B * n + 1] and ``cpt``
    float64: theta(v = k | configuration key) of structure b is ``cpt[offsets[b * n + v] + key * r + k]``, key the mixed-radix
    parent configuration with the lowest variable id fastest (include/dvs.h).  ``parents_host`` (uint64 [B, n]), ``card_host``
    and ``offsets_host`` are the host copies."""

    def __init__(self, parents: torch.Tensor, card: torch.Tensor, offsets: torch.Tensor, cpt: torch.Tensor,
                 parents_host: np.ndarray, card_host: Sequence[int], offsets_host: Sequence[int]):
        self.parents, self.card, self.offsets, self.cpt = parents, card, offsets, cpt
        self.parents_host, self.card_host, self.offsets_host = parents_host, list(card_host), list(offsets_host)
        self.batch, self.n_vars = parents.shape
        self.device = cpt.device

    def table(self, v: int, b: int = 0) -> torch.Tensor:
        """the [q, r] view of variable v's table in structure b"""
        q, r = _family(self.card_host, int(self.parents_host[b, v]), v)
        lo = self.offsets_host[b * self.n_vars + v]
        return self.cpt[lo:lo + q * r].view(q, r)

    def n_params(self, b: int = 0) -> int:
        """sum over the variables of (r - 1) q: bnlearn's nparams"""
        total = 0
        for v in range(self.n_vars):
            q, r = _family(self.card_host, int(self.parents_host[b, v]), v)
            total += (r - 1) * q
        return total

    @classmethod
    def from_tables(cls, parents, card, tables, device="cuda") -> "FittedBN":
        """One network from hand-written tables: ``parents`` n parent rows (ints), ``card`` n level counts, ``tables[v]`` the
        [q, r] table of variable v (rows: parent configurations, lowest parent id fastest)."""
        dl.need_cuda("FittedBN.from_tables", device)
        card = dl.level_counts(card)
        n = len(card)
        host = np.array([[int(r) for r in parents]], np.uint64)
        if host.shape != (1, n) or len(tables) != n:
            raise ValueError(f"parents and tables must have one entry per variable ({n})")
        off = _offsets(card, host)
        flat = []
        for v in range(n):
            t = np.asarray(tables[v], np.float64)
            if t.shape != _family(card, int(host[0, v]), v):
                raise ValueError(f"table of variable {v} must be [q, r] = {_family(card, int(host[0, v]), v)} (got {t.shape})")
            flat.append(t.reshape(-1))
        dev = torch.device(device)
        return cls(torch.from_numpy(host.view(np.int64)).to(dev), torch.tensor(card, dtype=torch.uint8, device=dev),
                   torch.tensor(off, dtype=torch.int64, device=dev), torch.from_numpy(np.concatenate(flat)).to(dev), host, card, off)


def bn_fit(evaluator, parents, *, method: str = "mle", iss=None, unobserved: str = "nan") -> FittedBN:
    """bnlearn's ``bn.fit`` for a batch: ``parents`` int64 [n] or [B, n] parent masks over the evaluator's variables -> the
    tables of every structure, fitted on the evaluator's data set.  ``method`` "mle" (theta = N_jk / N_j; an unobserved
    configuration is NaN, or 1 / r with ``unobserved="uniform"``: bnlearn's replace.unidentifiable) or "bayes" (theta =
    (N_jk + a) / (N_j + r a), a = iss / (r q); ``iss`` defaults to 1).  The rows are read back once to lay out the tables; a
    family of more than 36 864 cells raises ValueError before anything is launched."""
    what = "bn_fit"
    dl.need_discrete(what, evaluator)
    dl.need_cuda(what, evaluator.device)
    if method not in dl.FIT_METHODS:
        raise ValueError(f"method must be one of {sorted(dl.FIT_METHODS)} (got {method!r})")
    if unobserved not in UNOBSERVED:
        raise ValueError(f"unobserved must be one of {sorted(UNOBSERVED)} (got {unobserved!r})")
    if iss is not None and method != "bayes":
        raise ValueError("iss is the argument of method='bayes'")
    iss = 1.0 if iss is None else float(iss)
    if not (math.isfinite(iss) and iss > 0):
        raise ValueError(f"iss must be finite and > 0 (got {iss!r})")
    if not torch.is_tensor(parents) or parents.dtype != torch.int64 or parents.ndim not in (1, 2):
        raise ValueError(f"{what}: parents must be an int64 tensor [n] or [B, n] of parent masks")
    n, card = evaluator.n_vars, evaluator.card_host
    dev = evaluator.device
    parents = parents.reshape(-1, parents.shape[-1]).to(dev).contiguous()
    if parents.shape[1] != n or parents.shape[0] < 1:
        raise ValueError(f"{what}: expected {n} variables per structure, got {tuple(parents.shape)}")
    host = parents.cpu().numpy().view(np.uint64)                    # the one read-back
    if (host >> np.uint64(n)).any():
        raise ValueError(f"{what}: a parent row has a bit at or above n_vars = {n}")
    levels = np.asarray(card, np.float64)
    bits = ((host[:, :, None] >> np.arange(n, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    bits[:, np.arange(n), np.arange(n)] = False                     # the self bit is ignored
    cells = np.where(bits, levels, 1.0).prod(-1) * levels           # [B, n]: q r, exact wherever it is within the limit
    if (cells > dl.FIT_MAX_CELLS).any():
        b, v = (int(i) for i in np.argwhere(cells > dl.FIT_MAX_CELLS)[0])
        raise ValueError(f"{what}: variable {v} of structure {b} has a table of {cells[b, v]:,.0f} cells; the on-chip counting "
                         f"table holds {dl.FIT_MAX_CELLS:,} and no sorted-samples path exists for bn_fit")
    off = [0] + np.cumsum(cells.astype(np.int64).reshape(-1)).tolist()
    B = parents.shape[0]
    with torch.cuda.device(dev):
        offsets = torch.tensor(off, dtype=torch.int64, device=dev)
        cpt = torch.empty(max(off[-1], B * n), dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib, p = evaluator.lib, dl.ptr
        dl.check(lib, lib.dvs_bn_fit(B, n, evaluator.n_samples, p(evaluator.packed), p(evaluator.card), p(parents),
                                     dl.FIT_METHODS[method], iss, UNOBSERVED[unobserved], p(offsets), p(cpt), cpt.numel() * 8,
                                     p(status), dl.stream()), "dvs_bn_fit")
    return FittedBN(parents, evaluator.card, offsets, cpt[:off[-1]], host, card, off)


def sample(fitted: FittedBN, n_rows: int, *, seed: int, row_offset: int = 0, index: int = 0) -> torch.Tensor:
    """bnlearn's ``rbn``: ``n_rows`` rows drawn by forward sampling from structure ``index`` of ``fitted`` -> packed int64
    [n_rows, ceil(n / 16)] on the device, the layout ``BNLearnWrapper.from_packed`` and ``log_likelihood`` take.  Row i is a
    function of (seed, row_offset + i) and the tables only, so a request may be cut into calls with consecutive
    ``row_offset`` — or spread over devices — and gives the same rows.  A cycle, or a table row that is not a probability
    vector (a NaN or negative cell, a sum further than 1e-9 from 1), raises ValueError."""
    what = "sample"
    dl.need_cuda(what, fitted.device)
    if not 0 <= int(index) < fitted.batch:
        raise ValueError(f"{what}: index must be in [0, {fitted.batch})")
    if int(n_rows) < 1 or int(row_offset) < 0:
        raise ValueError(f"{what}: n_rows must be >= 1 and row_offset >= 0")
    n, dev, lib, p = fitted.n_vars, fitted.device, dl.load(), dl.ptr
    lo, hi = fitted.offsets_host[index * n], fitted.offsets_host[(index + 1) * n]
    with torch.cuda.device(dev):
        ws_bytes = dl.workspace_bytes(lib, "dvs_bn_sample_workspace_bytes", hi - lo, n)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        out = torch.empty(int(n_rows), (n + 15) // 16, dtype=torch.int64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_sample(n, int(n_rows), p(fitted.card), p(fitted.parents[index]), p(fitted.offsets[index * n:]),
                                        p(fitted.cpt), hi - lo, dl.seed64(seed), int(row_offset), p(ws), ws_bytes,
                                        p(out), p(status), dl.stream()), "dvs_bn_sample")
        st = int(status.item())
    dl.check_network_status(what, st)
    if st:
        raise ValueError(f"{what}: the tables do not match the structure (status {st})")
    return out


def log_likelihood(fitted: FittedBN, data, *, per_row: bool = False):
    """bnlearn's ``logLik(fitted, newdata)`` for every structure of ``fitted``: ``data`` an evaluator over the same variables
    or packed int64 rows [S, ceil(n / 16)] on the device -> float64 [B] on the device, with ``per_row`` (total [B], row terms
    [B, S]).  A row that meets theta = 0 counts -inf and one that meets a NaN cell NaN; a level code at or above a variable's
    level count raises ValueError."""
    what = "log_likelihood"
    dl.need_cuda(what, fitted.device)
    n, B, dev, lib, p = fitted.n_vars, fitted.batch, fitted.device, dl.load(), dl.ptr
    data = dl.packed_rows(what, data, n)
    S = data.shape[0]
    up = lambda x: (x + 255) & ~255
    chunks = (S + 255) // 256
    ws_bytes = up(B * chunks * 8) + up(B * n * 4) + max(fitted.offsets_host[-1] - fitted.offsets_host[0], B * n) * 8
    with torch.cuda.device(dev):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        rows = torch.empty(B, S, dtype=torch.float64, device=dev) if per_row else None
        out = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        dl.check(lib, lib.dvs_bn_loglik(B, n, S, p(data), p(fitted.card), p(fitted.parents), p(fitted.offsets), p(fitted.cpt),
                                        p(rows), p(out), p(ws), ws_bytes, p(status), dl.stream()), "dvs_bn_loglik")
        if int(status.item()) & dl.STATUS_REFUSED:
            raise ValueError(f"{what}: a row has a level code at or above its variable's level count, or the tables do not match the structure")
    return (out, rows) if per_row else out


def cv_folds(n_rows: int, folds: int, seed: int) -> List[np.ndarray]:
    """The held-out parts of ``cross_validate``: numpy's ``default_rng(seed).permutation(n_rows)`` cut into ``folds``
    contiguous parts, part f being positions [f * n_rows // folds, (f + 1) * n_rows // folds)."""
    perm = np.random.default_rng(seed).permutation(n_rows)
    return [perm[f * n_rows // folds:(f + 1) * n_rows // folds] for f in range(folds)]


CV_LOSSES = {"logl": None, "pred": "parents", "pred-exact": "exact", "pred-lw": "bayes-lw"}   # loss -> predict's method


def cross_validate(evaluator, parents, *, folds: int = 10, seed: int = 0, method: str = "mle", iss=None, loss: str = "logl",
                   target=None, n=None) -> torch.Tensor:
    """bnlearn's ``bn.cv`` for fixed structures: the rows are permuted (``cv_folds``), each part is held out in turn, the tables
    are fitted on the rest (``bn_fit``) and the part is scored.  -> float64 [B] on the device.

    ``loss="logl"`` (the default): minus the held-out log-likelihood (``log_likelihood``) per row, summed over the parts and
    divided by the number of rows.  Under "mle" a held-out row whose configuration the rest never showed makes the loss NaN,
    and one whose level the rest never showed under its configuration +inf, as with bnlearn's defaults; "bayes" keeps it finite.

    ``loss="pred" | "pred-exact" | "pred-lw"``: the share of held-out rows whose level of variable ``target`` is predicted
    wrongly (``infer.predict`` with method "parents", "exact" or "bayes-lw" with ``n`` particles per row, 500 by default, and ``seed``; ``n``
    is the argument of "pred-lw" alone; a row that predicts 255 counts as wrong).  "pred-lw" runs one likelihood-weighting call
    per structure and part; the other two take the whole batch of structures in one call per part.  bnlearn has "pred" and "pred-lw"; "pred-exact" is what "pred-lw" approximates."""
    what = "cross_validate"
    dl.need_discrete(what, evaluator)
    dl.need_cuda(what, evaluator.device)
    S = evaluator.n_samples
    if not 2 <= int(folds) <= S:
        raise ValueError(f"{what}: folds must be in [2, {S}]")
    if loss not in CV_LOSSES:
        raise ValueError(f"{what}: loss must be one of {sorted(CV_LOSSES)} (got {loss!r})")
    if (loss == "logl") != (target is None):
        raise ValueError(f"{what}: target is the argument of the prediction losses, and they need it")
    if n is not None and (loss != "pred-lw" or int(n) < 1):
        raise ValueError(f"{what}: n (>= 1) is the argument of loss='pred-lw'")
    n = 500 if n is None else int(n)
    if target is not None and not 0 <= int(target) < evaluator.n_vars:
        raise ValueError(f"{what}: target must be in [0, {evaluator.n_vars})")
    dev = evaluator.device
    with torch.cuda.device(dev):
        parts = [torch.from_numpy(p).to(dev) for p in cv_folds(S, int(folds), seed)]
        total = None
        done = 0
        for f, part in enumerate(parts):
            rest = torch.cat([p for g, p in enumerate(parts) if g != f])
            train = BNLearnWrapper.from_packed(evaluator.dataset_name, evaluator.metric_name, evaluator.packed[rest],
                                               evaluator.card_host, iss=evaluator.iss, k=evaluator.k)
            fitted = bn_fit(train, parents, method=method, iss=iss)
            held = evaluator.packed[part]
            if loss == "logl":
                ll = log_likelihood(fitted, held)
            else:
                ll = _wrong_predictions(fitted, held, int(target), CV_LOSSES[loss], n, seed, done)
            done += held.shape[0]
            total = ll if total is None else total + ll
    if loss == "logl":
        return -total / S
    return total / torch.full_like(total, float(S))          # tensor by tensor: one correctly rounded division of the count


def _wrong_predictions(fitted, held, target, method, n, seed, query_offset):
    """float64 [B]: the held-out rows whose level of `target` structure b predicts wrongly"""
    from . import infer
    truth = ((held[:, target // 16] >> (4 * (target % 16))) & 15).to(torch.uint8)
    if method != "bayes-lw":
        pred, _ = infer._blanket(fitted, held.contiguous(), target, method == "exact", False, None, "cross_validate")
    else:
        pred = torch.stack([infer.predict(fitted, target, held, method=method, n=n, seed=seed, index=b, query_offset=query_offset)
                            for b in range(fitted.batch)])
    return (pred != truth[None, :]).sum(1).to(torch.float64)
