"""Latent-space Bayesian optimisation over labelled DAGs: encode -> GP -> expected improvement -> decode -> BIC.

The search that gives the project its name (encode a labelled DAG into a latent vector with a VAE, regress
the BIC score from the latent, search in latent space).  The reference stops before it (experiments/01_bn_asia/main.py ends
at ``train_predictor``), so there is no reference run to match; its parts are pinned separately (tests/test_gpu_search.py:
the GP maths against a float64 restatement, every returned score against the BIC oracle).

One iteration, all numerical work on the device:
  1. the GP takes the current (latent, BIC) rows (``set_train_data``; optionally a few warm-started hyper-parameter steps)
     and solves its posterior once (``fit_posterior``);
  2. ``n_starts`` starts in the box spanned by the training latents: half around the best-scoring latents, half uniform;
  3. ``optimize_acquisition``: multi-start gradient ascent on EI — per step one ``dvs_gp_acquire`` (EI and dEI/dx) and one
     fused Adam (``dvs_clip_adam``), then a clamp to the box;
  4. the ``batch_size`` candidates of highest EI are decoded ``decode_tries`` times each (``PaceVaeV3.decode``);
  5. valid, new structures (a DAG on n vertices whose labels are a permutation of 0..n-1, not seen before) are scored
     (``BNLearnWrapper.score_compact``) and encoded (``encode_direct``), and their rows join the data.
Maximisation: bnlearn's BIC is higher-is-better.  Batch selection is plain top-EI (no Kriging believer / q-EI).

Steps 4-5 have two implementations that give the same result draw for draw.  ``candidates="host"`` (the default) turns
every draw into a graph object and keeps the seen structures in a Python set.  ``candidates="device"`` keeps the decoded
rows on the device: ``decoded_structures`` (dvs_decoded_structures: validity, row codec, label-space structure key,
hash) -> ``StructureSet.filter`` (dvs_structset_filter: exact, first occurrence in draw order) -> a gather of the new rows
-> ``score_masks`` / ``encode_direct``; graph objects are made for the new rows only.  Both are defined for
label-permutation data sets (every vertex stands for its own variable: asia, sachs, alarm, n = card synthetic).
"""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as dl
from ._lib import nbytes, ptr, require_cuda, stream
from .features import LabeledDag, _as_labels_edges
from .predictor import expected_improvement_host
from .records import CompactBatch, decode_graphs, encode_graphs

STRUCT_VALID, STRUCT_SHORT, STRUCT_LABEL_RANGE, STRUCT_LABEL_REPEAT = 1, 2, 4, 8     # flags of decoded_structures
FILTER_NEW, FILTER_SEEN, FILTER_DUPLICATE = 1, 2, 4                                   # verdicts of dvs_structset_filter
MAX_DECODE_ROWS = 65536      # rows per decode_states call of generation_metrics


@dataclass
class SearchStep:
    iteration: int
    n_candidates: int          # decoded draws (batch_size x decode_tries)
    n_valid: int               # draws that are valid DAGs with permutation labels
    n_new: int                 # distinct structures not in the data before, scored and appended
    best_score: float          # best BIC in the data after this iteration
    seconds: float
    ei_max: float = 0.0        # largest EI among the selected candidates (host restatement of the kernel's mean / var)
    timings_ms: Dict[str, float] = field(default_factory=dict)     # fit / ascent / decode / score / encode


@dataclass
class SearchResult:
    best_graph: object
    best_score: float
    history: List[SearchStep]
    evaluated: List[Tuple[object, float]]      # every (graph, BIC) pair: the initial graphs first, then the search's
    n_initial: int


def structure_key(graph) -> Tuple[Tuple[int, int], ...]:
    """Identity of a labelled DAG as a Bayesian-network structure: its edges in label space (label u -> label v), sorted.
    The same network under another vertex order or edge order has the same key (BIC depends on nothing else)."""
    labels, edges = _as_labels_edges(graph)
    return tuple(sorted((int(labels[u]), int(labels[v])) for u, v in edges))


def is_search_valid(graph, dag: LabeledDag) -> bool:
    """A decoded draw the scorer can take: ``LabeledDag.is_valid_graph`` (a DAG, n vertices, labels in range) and labels
    that are a permutation of 0..n-1 (bnlearn.py:35 asserts it; ``is_valid_graph`` does not check it)."""
    if graph is None or not dag.is_valid_graph(graph):
        return False
    labels, _ = _as_labels_edges(graph)
    return sorted(int(v) for v in labels) == list(range(dag.num_vertices))


def new_structures(graphs: Sequence, dag: LabeledDag, seen: set) -> Tuple[list, int]:
    """(valid draws whose structure is not in ``seen`` — first occurrence kept, draw order —, number of valid draws).
    ``seen`` is updated with the keys of the returned graphs."""
    out, n_valid = [], 0
    for g in graphs:
        if not is_search_valid(g, dag):
            continue
        n_valid += 1
        k = structure_key(g)
        if k in seen:
            continue
        seen.add(k)
        out.append(g)
    return out, n_valid


# ---- the same stage on the device (csrc/dvs_structs.h) ----------------------------------------------------------------
_ALL_ONES = 0xFFFFFFFFFFFFFFFF


def _s64(x: int) -> int:
    """The int64 with the bit pattern of the unsigned 64-bit ``x``."""
    x &= _ALL_ONES
    return x - (1 << 64) if x >> 63 else x


def _mix64(x: torch.Tensor) -> torch.Tensor:
    """splitmix64's finaliser on int64 bit patterns (structs_mix64): logical shifts, wrapping products."""
    x = x ^ ((x >> 30) & ((1 << 34) - 1))
    x = x * _s64(0xBF58476D1CE4E5B9)
    x = x ^ ((x >> 27) & ((1 << 37) - 1))
    x = x * _s64(0x94D049BB133111EB)
    return x ^ ((x >> 31) & ((1 << 33) - 1))


def hash_keys(keys: torch.Tensor, hash_mask: int = _ALL_ONES) -> torch.Tensor:
    """The hash ``dvs_decoded_structures`` gives a valid row, from its key alone (int64 [B, n_vars] -> int64 [B]), for keys
    that do not come from decoded rows (``StructureSet.add_graphs`` / ``contains``).  Plain tensor arithmetic on the
    keys' device; pinned to the kernel's value in tests/test_emu_structures.py."""
    n = keys.shape[1]
    salt = torch.arange(1, n + 1, dtype=torch.int64, device=keys.device) * _s64(0x9E3779B97F4A7C15)
    total = _mix64(keys ^ salt).sum(1, dtype=torch.int64)
    return _mix64(total) & _s64(hash_mask) & dl.STRUCT_HASH_INVALID


def _decoded_structures(states: torch.Tensor, n: int, hash_mask: int = _ALL_ONES):
    require_cuda(states, "states")
    if states.dtype != torch.uint8 or states.dim() != 2 or states.shape[1] != dl.DECODE_STATE_BYTES:
        raise AssertionError(f"Expected states uint8 [B, {dl.DECODE_STATE_BYTES}], got {states.dtype} {tuple(states.shape)}")
    lib = dl.load()
    dev = states.device
    B = states.shape[0]
    wide = n > 13                        # the CompactBatch convention (records.py)
    states = states.contiguous()
    flags = torch.empty(B, dtype=torch.uint8, device=dev)
    labels = torch.empty(B, n, dtype=torch.uint8, device=dev)
    preds = torch.empty(B, n, dtype=torch.int64 if wide else torch.int16, device=dev)
    keys = torch.empty(B, n, dtype=torch.int64, device=dev)
    hashes = torch.empty(B, dtype=torch.int64, device=dev)
    if B:
        dl.check(lib, lib.dvs_decoded_structures(B, n, 1 if wide else 0, ptr(states), nbytes(states), hash_mask & _ALL_ONES,
                                                 ptr(flags), ptr(labels), ptr(preds), ptr(keys), nbytes(keys),
                                                 ptr(hashes), stream()), "dvs_decoded_structures")
    return flags, CompactBatch(labels, preds), keys, hashes


def _n_vars(vae) -> int:
    n = vae.max_num_vertices - 3
    if vae.vertex_label_cardinality - 3 < n:
        raise ValueError(f"structure keys need a label-permutation data set: {n} vertices but only "
                         f"{vae.vertex_label_cardinality - 3} labels")
    return n


def decoded_structures(vae, states: torch.Tensor, hash_mask: int = _ALL_ONES):
    """What steps 4-5 need of every decoded row, computed on the device from ``vae.decode_states`` output (uint8
    [B, DECODE_STATE_BYTES]) -> (flags uint8 [B], CompactBatch, keys int64 [B, n], hashes int64 [B]):
    ``flags & 1`` equals ``is_search_valid`` of the row's graph object (other bits: why not, STRUCT_*); the CompactBatch is
    ``encode_graphs`` of the graph objects (zeros on invalid rows), ready for ``encode_direct``; ``keys`` are the parent
    masks in data-set variable indices, ready for ``BNLearnWrapper.score_masks`` and equal between two rows iff their
    ``structure_key`` are equal; ``hashes`` order the rows for ``StructureSet``.  Label-permutation data sets only."""
    return _decoded_structures(states, _n_vars(vae), hash_mask)


class StructureSet:
    """The structures seen so far, on the device: (hash, key) rows kept sorted by hash.  Membership is decided on the full
    key by ``dvs_structset_filter`` (exact whatever the hashes collide on; deterministic: no atomics).  ``hash_mask``
    must be the one the hashes passed to ``filter`` were made with."""

    def __init__(self, n_vars: int, device="cuda", hash_mask: int = _ALL_ONES):
        self.n_vars = int(n_vars)
        self.device = torch.device(device)
        self.hash_mask = hash_mask & _ALL_ONES
        self.hashes = torch.empty(0, dtype=torch.int64, device=self.device)
        self.keys = torch.empty(0, self.n_vars, dtype=torch.int64, device=self.device)

    def __len__(self) -> int:
        return self.hashes.shape[0]

    def _verdicts(self, keys: torch.Tensor, hashes: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
        """FILTER_NEW / FILTER_SEEN / FILTER_DUPLICATE / 0 per row (uint8 [B]); the set is not changed."""
        require_cuda(keys, "keys")
        B = keys.shape[0]
        if tuple(keys.shape) != (B, self.n_vars) or keys.dtype != torch.int64 or tuple(hashes.shape) != (B,) or \
                hashes.dtype != torch.int64 or tuple(flags.shape) != (B,) or flags.dtype != torch.uint8:
            raise AssertionError(f"Expected keys int64 [B, {self.n_vars}], hashes int64 [B], flags uint8 [B]")
        out = torch.zeros(B, dtype=torch.uint8, device=keys.device)
        if B == 0:
            return out
        lib = dl.load()
        keys, flags = keys.contiguous(), flags.contiguous()
        sorted_hashes, order = torch.sort(hashes, stable=True)      # equal hashes stay in draw order
        S = len(self)
        dl.check(lib, lib.dvs_structset_filter(B, self.n_vars, ptr(sorted_hashes), ptr(order), ptr(keys), nbytes(keys),
                                               ptr(flags), S, ptr(self.hashes) if S else None,
                                               ptr(self.keys) if S else None, nbytes(self.keys), ptr(out), stream()),
                 "dvs_structset_filter")
        return out

    def _insert(self, keys: torch.Tensor, hashes: torch.Tensor):
        """Rows known to be distinct and not in the set."""
        merged, order = torch.sort(torch.cat([self.hashes, hashes]), stable=True)
        self.hashes = merged
        self.keys = torch.cat([self.keys, keys])[order].contiguous()

    def _filter_rows(self, keys, hashes, flags, insert: bool, also: Optional[torch.Tensor] = None):
        """(new mask bool [B], indices of the new rows in row order int64 [n_new], ``also`` as a list).  ONE read-back: the
        number of new rows, with the values of ``also`` (a small device int64 tensor the caller wants on the host) in the same
        copy.  The indices come from a stable sort of the mask cut at that number, not from a second synchronising call."""
        mask = self._verdicts(keys, hashes, flags) == FILTER_NEW
        count = mask.sum().reshape(1)
        n_new, *rest = (count if also is None else torch.cat([count, also.reshape(-1)])).tolist()
        idx = torch.sort(mask.to(torch.uint8), descending=True, stable=True).indices[:n_new]
        if insert and n_new:
            self._insert(keys[idx], hashes[idx])
        return mask, idx, rest

    def filter(self, keys: torch.Tensor, hashes: torch.Tensor, flags: torch.Tensor, insert: bool = True) -> torch.Tensor:
        """The rows ``new_structures`` would return, as a device bool mask [B]: valid (``flags & 1``), key not in the set, and
        no earlier row of the batch with the same key.  ``insert``: those rows join the set."""
        if not insert:
            return self._verdicts(keys, hashes, flags) == FILTER_NEW
        return self._filter_rows(keys, hashes, flags, True)[0]

    def contains(self, keys: torch.Tensor) -> torch.Tensor:
        """Device bool [B]: is each key (int64 [B, n_vars]) in the set."""
        flags = torch.ones(keys.shape[0], dtype=torch.uint8, device=keys.device)
        return self._verdicts(keys, hash_keys(keys, self.hash_mask), flags) == FILTER_SEEN

    def add_graphs(self, graphs: Sequence) -> int:
        """Insert host graph objects (the initial data); returns how many were not in the set yet."""
        n = self.n_vars
        masks = np.zeros((len(graphs), n), np.uint64)
        for b, g in enumerate(graphs):
            labels, edges = _as_labels_edges(g)
            if sorted(int(v) for v in labels) != list(range(n)):
                raise ValueError(f"Expected graph labels to be a permutation of 0..{n - 1}, but got {list(labels)}")
            for u, v in edges:
                masks[b, labels[v]] |= np.uint64(1) << np.uint64(labels[u])
        keys = torch.from_numpy(masks.view(np.int64)).to(self.device)
        flags = torch.ones(len(graphs), dtype=torch.uint8, device=self.device)
        return int(self._filter_rows(keys, hash_keys(keys, self.hash_mask), flags, True)[1].numel())


def generation_latents(vae, n_samples: int, seed: int) -> torch.Tensor:
    """The latents ``generation_metrics`` decodes: float32 [n_samples, latent] from N(0, I), a seeded CPU generator."""
    gen = torch.Generator(device="cpu")
    gen.manual_seed(int(seed))
    return torch.randn(int(n_samples), vae.latent_layer_size, generator=gen)


def generation_metrics(vae, train_graphs: Sequence, n_samples: int = 4096, seed: int = 0,
                       latents: Optional[torch.Tensor] = None) -> Dict[str, float]:
    """Validity / uniqueness / novelty of the VAE as a generator, the triple usual for DAG VAEs, counted on the device:
    ``vae.seed(seed)``, then ``generation_latents`` (N(0, I); or ``latents`` [n_samples, latent] when given, e.g. draws
    around the training posteriors) decoded in ``decode_states`` calls of at most 65 536 rows.
    validity: share of search-valid draws; uniqueness: share of distinct structures among the valid draws; novelty: share
    of those distinct structures that are not in ``train_graphs``.  Structures are compared as Bayesian networks
    (``structure_key``), so this is defined for label-permutation data sets only (asia, sachs, alarm, n = card
    synthetic); with repeated labels (card < n) identity is an isomorphism class, which keys cannot express."""
    dev = vae.flat_params.device
    n = _n_vars(vae)
    vae.seed(int(seed))
    z = generation_latents(vae, n_samples, seed) if latents is None else latents
    n_samples = z.shape[0]
    parts = [_decoded_structures(vae.decode_states(z[s:s + MAX_DECODE_ROWS].to(dev)), n)
             for s in range(0, int(n_samples), MAX_DECODE_ROWS)]
    flags = torch.cat([p[0] for p in parts])
    keys = torch.cat([p[2] for p in parts])
    hashes = torch.cat([p[3] for p in parts])
    distinct = StructureSet(n, dev).filter(keys, hashes, flags, insert=False)
    train = StructureSet(n, dev)
    train.add_graphs(list(train_graphs))
    novel = train.filter(keys, hashes, flags, insert=False)
    n_valid, n_unique, n_novel = torch.stack([(flags & STRUCT_VALID).sum(), distinct.sum(), novel.sum()]).tolist()
    return {"n_samples": int(n_samples), "n_valid": n_valid, "n_unique": n_unique, "n_novel": n_novel,
            "validity": n_valid / max(int(n_samples), 1), "uniqueness": n_unique / max(n_valid, 1),
            "novelty": n_novel / max(n_unique, 1)}


def optimize_acquisition(gp, starts: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor, best: float, steps: int = 50,
                         lr: float = 0.05, xi: float = 0.0, variance: str = "sor"):
    """Multi-start gradient ascent on EI, all on the device: per step one ``dvs_gp_acquire`` (EI, dEI/dx) and one fused
    Adam (``dvs_clip_adam``, no clipping) on the flat candidate vector with the negated gradient, then a clamp to
    [lo, hi].  ``starts`` [S, dim]; ``lo`` / ``hi`` [dim].  Returns (candidates float32 [S, dim], their EI float64 [S])."""
    dev = gp.device
    x = starts.to(dev, torch.float32).clone().contiguous()
    lo = lo.to(dev, torch.float32).reshape(1, -1)
    hi = hi.to(dev, torch.float32).reshape(1, -1)
    torch.maximum(torch.minimum(x, hi), lo, out=x)
    S, D = x.shape
    f64 = dict(dtype=torch.float64, device=dev)
    bufs = (torch.empty(S, **f64), torch.empty(S, **f64), torch.empty(S, **f64),
            torch.empty(S, D, dtype=torch.float32, device=dev))
    m = torch.zeros_like(x)
    v = torch.zeros_like(x)
    scratch = torch.zeros(dl.CLIP_SCRATCH_FLOATS, dtype=torch.float32, device=dev)
    for it in range(1, steps + 1):
        _, _, _, g = gp._acquire(x, best, xi, variance, grad=True, out=bufs)
        g.neg_()
        dl.check(gp.lib, gp.lib.dvs_clip_adam(x.numel(), ptr(x), ptr(g), ptr(m), ptr(v), lr, 0.9, 0.999, 1e-8, it, -1.0,
                                              ptr(scratch), None, stream()), "dvs_clip_adam")
        torch.maximum(torch.minimum(x, hi), lo, out=x)
    ei = gp.expected_improvement(x, best, xi, variance)
    return x, ei


def _encode_score(vae, evaluator, graphs: Sequence, n: int, timings: Optional[Dict[str, float]] = None):
    """(mu float32 [B, latent], BIC float64 [B]) of ``graphs``, both on the device (score_compact + encode_direct)."""
    dev = vae.flat_params.device
    batch = encode_graphs(list(graphs), n, vae.graph_label_key).to(dev)
    t0 = time.perf_counter()
    y = evaluator.score_compact(batch)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    was_training = vae.training
    vae.eval()
    try:
        mu, _ = vae.encode_direct(batch)
    finally:
        vae.train(was_training)
    torch.cuda.synchronize(dev)
    if timings is not None:
        timings["score"] = (t1 - t0) * 1e3
        timings["encode"] = (time.perf_counter() - t1) * 1e3
    return mu.detach(), y


def _encode_score_rows(vae, evaluator, rows: CompactBatch, keys: torch.Tensor, timings: Dict[str, float]):
    """``_encode_score`` of rows that are on the device already: ``score_masks`` of their keys (the masks ``score_compact``
    would derive from the codec) and ``encode_direct`` of their codec."""
    dev = vae.flat_params.device
    t0 = time.perf_counter()
    y = evaluator.score_masks(keys)
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    was_training = vae.training
    vae.eval()
    try:
        mu, _ = vae.encode_direct(rows)
    finally:
        vae.train(was_training)
    torch.cuda.synchronize(dev)
    timings["score"] = (t1 - t0) * 1e3
    timings["encode"] = (time.perf_counter() - t1) * 1e3
    return mu.detach(), y


def _device_candidates(vae, evaluator, seen: StructureSet, z: torch.Tensor, decode_tries: int, X: torch.Tensor,
                       Y: torch.Tensor, evaluated: list, tm: Dict[str, float], t2: float):
    """Steps 4-5 of one iteration with the draws kept on the device -> (draws, valid, new, X, Y); ``evaluated`` grows by
    the new rows' graph objects and scores, in draw order."""
    dev = vae.flat_params.device
    states = vae.decode_states(z.repeat_interleave(decode_tries, 0))
    torch.cuda.synchronize(dev)
    t3 = time.perf_counter()
    tm["decode"] = (t3 - t2) * 1e3
    flags, compact, keys, hashes = decoded_structures(vae, states)
    _, idx, (n_valid,) = seen._filter_rows(keys, hashes, flags, True, also=(flags & STRUCT_VALID).sum())
    new_rows, new_keys = compact[idx], keys[idx]
    torch.cuda.synchronize(dev)
    tm["candidates"] = (time.perf_counter() - t3) * 1e3
    n_new = int(idx.numel())
    if n_new:
        mu, y = _encode_score_rows(vae, evaluator, new_rows, new_keys, tm)
        X = torch.cat([X, mu.to(torch.float64)])
        Y = torch.cat([Y, y])
        evaluated.extend(zip(decode_graphs(new_rows), y.cpu().tolist()))
    else:
        tm["score"] = tm["encode"] = 0.0
    return states.shape[0], n_valid, n_new, X, Y


def latent_bo_search(vae, gp, evaluator, graphs: Sequence, iterations: int = 10, batch_size: int = 32, n_starts: int = 256,
                     steps: int = 50, lr: float = 0.05, decode_tries: int = 4, xi: float = 0.0, variance: str = "sor",
                     hyper_steps: int = 0, seed: int = 0, start_noise: float = 0.05,
                     candidates: str = "host") -> SearchResult:
    """Bayesian optimisation of the BIC in the VAE's latent space (module docstring).  ``vae``: a ``PaceVaeV3`` on the
    device; ``gp``: a ``GPRegressionModel`` (its inducing points and hyper-parameters are kept; ``hyper_steps`` > 0 runs
    that many warm-started ``train_hyperparameters(from_defaults=False)`` steps per iteration); ``evaluator``: a
    ``BNLearnWrapper`` (device scoring through ``score_compact``); ``graphs``: the initial data, encoded (posterior
    mean) and scored here.  ``start_noise``: the Gaussian noise of the starts around the best latents, as a fraction of
    the box's width per dimension.  Deterministic for a fixed ``seed`` (every device kernel on the path has a fixed
    summation order; the starts come from a seeded ``torch.Generator``; the VAE's sampler is re-seeded per iteration).
    ``candidates``: where steps 4-5 judge the draws — "host" (graph objects and a Python set) or "device"
    (``decoded_structures`` + ``StructureSet``; module docstring).  Same result either way: history, evaluated graphs in
    the same order, bitwise equal scores.  "device" reads back one small vector per iteration (the number of new rows,
    with the number of valid ones), adds ``timings_ms["candidates"]`` (decoded rows -> gathered new rows) and makes graph
    objects only for the rows that were new."""
    if candidates not in ("host", "device"):
        raise ValueError(f"candidates must be 'host' or 'device', got {candidates!r}")
    dev = vae.flat_params.device
    n = vae.max_num_vertices - 3
    dag = LabeledDag(n, vae.vertex_label_cardinality - 3)
    graphs = list(graphs)
    for g in graphs:
        if not is_search_valid(g, dag):
            raise ValueError("every initial graph must be a valid DAG whose labels are a permutation of 0..n-1")
    X, Y = _encode_score(vae, evaluator, graphs, n)
    X = X.to(torch.float64)
    evaluated: List[Tuple[object, float]] = list(zip(graphs, Y.cpu().tolist()))
    seen = {structure_key(g) for g in graphs}
    if candidates == "device":
        seen_device = StructureSet(_n_vars(vae), dev)
        seen_device.add_graphs(graphs)
    gen = torch.Generator(device="cpu")
    history: List[SearchStep] = []
    D = X.shape[1]
    for it in range(1, iterations + 1):
        t_start = time.perf_counter()
        tm: Dict[str, float] = {}
        # 1. posterior on the current data
        gp.set_train_data(X, Y)
        if hyper_steps > 0:
            gp.train_hyperparameters(hyper_steps, from_defaults=False, log_every=0)
        gp.fit_posterior()
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        tm["fit"] = (t1 - t_start) * 1e3
        # 2. starts: half around the best latents, half uniform in the box of the training latents
        lo, hi = X.min(0).values.float(), X.max(0).values.float()
        width = (hi - lo).cpu()
        gen.manual_seed((int(seed) * 1000003 + it) & 0x7FFFFFFFFFFFFFFF)
        n_top = n_starts // 2
        order = torch.sort(Y.cpu(), descending=True, stable=True).indices
        top = X.cpu().float()[order[torch.arange(n_top) % len(order)]]
        near = top + torch.randn(n_top, D, generator=gen) * (start_noise * width)
        unif = lo.cpu() + torch.rand(n_starts - n_top, D, generator=gen) * width
        starts = torch.cat([near, unif]).to(dev)
        best = float(Y.max())
        # 3. ascent, then the batch_size candidates of highest EI (ties: lower index first)
        cand, ei = optimize_acquisition(gp, starts, lo, hi, best, steps, lr, xi, variance)
        sel = torch.sort(ei.cpu(), descending=True, stable=True).indices[:batch_size]
        z = cand[sel.to(dev)]
        post = gp.posterior(z, variance)
        ei_sel = expected_improvement_host(post.mean.cpu().numpy(), post.stddev.cpu().numpy(), best, xi,
                                           1e-12 * gp.outputscale)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        tm["ascent"] = (t2 - t1) * 1e3
        # 4. decode every candidate decode_tries times from a seeded sampler
        vae.seed((int(seed) * 7919 + it) & 0xFFFFFFFF)
        if candidates == "device":
            n_draws, n_valid, n_new, X, Y = _device_candidates(vae, evaluator, seen_device, z, decode_tries, X, Y,
                                                               evaluated, tm, t2)
            history.append(SearchStep(it, n_draws, n_valid, n_new, float(Y.max()), time.perf_counter() - t_start,
                                      float(ei_sel.max()) if len(ei_sel) else 0.0, tm))
            continue
        draws = vae.decode(z.repeat_interleave(decode_tries, 0), strict=False)
        t3 = time.perf_counter()
        tm["decode"] = (t3 - t2) * 1e3
        # 5. new valid structures -> BIC and latent rows
        new, n_valid = new_structures(draws, dag, seen)
        if new:
            mu, y = _encode_score(vae, evaluator, new, n, tm)
            X = torch.cat([X, mu.to(torch.float64)])
            Y = torch.cat([Y, y])
            evaluated.extend(zip(new, y.cpu().tolist()))
        else:
            tm["score"] = tm["encode"] = 0.0
        history.append(SearchStep(it, len(draws), n_valid, len(new), float(Y.max()), time.perf_counter() - t_start,
                                  float(ei_sel.max()) if len(ei_sel) else 0.0, tm))
    b = max(range(len(evaluated)), key=lambda i: (evaluated[i][1], -i))
    return SearchResult(evaluated[b][0], evaluated[b][1], history, evaluated, len(graphs))
