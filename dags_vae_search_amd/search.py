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
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib as dl
from .features import LabeledDag, _as_labels_edges
from .predictor import expected_improvement_host
from .records import encode_graphs


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
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for it in range(1, steps + 1):
        _, _, _, g = gp._acquire(x, best, xi, variance, grad=True, out=bufs)
        g.neg_()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        dl.check(gp.lib, gp.lib.dvs_clip_adam(x.numel(), p(x), p(g), p(m), p(v), lr, 0.9, 0.999, 1e-8, it, -1.0, p(scratch),
                                              None, stream), "dvs_clip_adam")
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


def latent_bo_search(vae, gp, evaluator, graphs: Sequence, iterations: int = 10, batch_size: int = 32, n_starts: int = 256,
                     steps: int = 50, lr: float = 0.05, decode_tries: int = 4, xi: float = 0.0, variance: str = "sor",
                     hyper_steps: int = 0, seed: int = 0, start_noise: float = 0.05) -> SearchResult:
    """Bayesian optimisation of the BIC in the VAE's latent space (module docstring).  ``vae``: a ``PaceVaeV3`` on the
    device; ``gp``: a ``GPRegressionModel`` (its inducing points and hyper-parameters are kept; ``hyper_steps`` > 0 runs
    that many warm-started ``train_hyperparameters(from_defaults=False)`` steps per iteration); ``evaluator``: a
    ``BNLearnWrapper`` (device scoring through ``score_compact``); ``graphs``: the initial data, encoded (posterior
    mean) and scored here.  ``start_noise``: the Gaussian noise of the starts around the best latents, as a fraction of
    the box's width per dimension.  Deterministic for a fixed ``seed`` (every device kernel on the path has a fixed
    summation order; the starts come from a seeded ``torch.Generator``; the VAE's sampler is re-seeded per iteration)."""
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
