#!/usr/bin/env python3
"""Latent-space search measurements (dags_vae_search_amd/search.py):
  1. dvs_gp_acquire (mean, variance, EI and dEI/dx of Q candidates, M = 500 inducing points, D = 32, the shipped asia
     predictor) against the float64 torch composition of the same maths (cdist -> exp -> matmul -> row sums -> gradient
     matmul) timed in the same process: ms, candidates/s, fp64 TFLOP/s of the two contractions, max difference;
  2. one asia search iteration broken down into fit / ascent / decode / score / encode (ms).
    python bench_search.py [--reps 20] [--iterations 3]
Prints one JSON line.  (The driver's metric is bench.py; this is the measurement of the search path.)"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def _gp(x, y):
    from dags_vae_search_amd.predictor import GPRegressionModel
    from tests.helpers import load_npz
    fix = load_npz("asia_predictor.npz")
    gp = GPRegressionModel(x, y)
    gp.load_state_dict({"likelihood.noise_covar.raw_noise": torch.from_numpy(fix["raw_noise"]),
                        "mean_module.raw_constant": torch.from_numpy(fix["raw_constant"]),
                        "base_covar_module.raw_outputscale": torch.from_numpy(fix["raw_outputscale"]),
                        "base_covar_module.base_kernel.raw_lengthscale": torch.from_numpy(fix["raw_lengthscale"]),
                        "covar_module.inducing_points": torch.from_numpy(fix["inducing_points"])})
    return gp


def torch_acquire(gp, x, best, xi=0.0, kind="sor"):
    """The same maths as dvs_gp_acquire as a float64 torch composition (library dgemm + elementwise passes)."""
    W, c0 = gp._post[kind]
    M = W.shape[0]
    Z = gp.inducing_points.double()
    x64 = x.double()
    o, l, c = gp.outputscale, gp.lengthscale, gp.constant
    K = o * torch.exp(torch.cdist(x64, Z).pow(2) * (-0.5 / l ** 2))
    Y = K @ W
    quad = (K * Y[:, :M]).sum(1)
    mean = c + Y[:, M]
    var = torch.clamp(c0 + quad, min=0.0)
    sig = var.sqrt()
    ok = sig > 1e-12 * o
    ss = torch.where(ok, sig, torch.ones_like(sig))
    imp = mean - best - xi
    u = imp / ss
    Phi = torch.special.ndtr(u)
    phi = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    ei = torch.where(ok, imp * Phi + ss * phi, torch.relu(imp))
    wa = torch.where(ok, Phi, (imp > 0).double())
    wp = torch.where(ok, phi / ss, torch.zeros_like(ss))
    WK = (wa[:, None] * W[:, M][None, :] + wp[:, None] * Y[:, :M]) * K
    s = wa * (mean - c) + wp * quad
    grad = ((WK @ Z - x64 * s[:, None]) / l ** 2).float()
    return mean, var, ei, grad


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--metric", default="bic", help="the evaluator's score type (BNLearnWrapper metric_name)")
    args = ap.parse_args()
    from tests.helpers import graphs_from, load_npz
    fix = load_npz("asia_predictor.npz")
    x, y = torch.from_numpy(fix["x"]), torch.from_numpy(fix["y"])
    ntr = int(np.floor(0.8 * len(x)))
    gp = _gp(x[:ntr], y[:ntr])
    gp.fit_posterior()
    M, D = gp.inducing_points.shape
    best = float(y[:ntr].median())                 # EI and its gradient well away from 0 at part of the candidates
    lo, hi = x.min(0).values, x.max(0).values
    g = torch.Generator().manual_seed(0)
    rows = []
    for Q in (4096, 16384, 65536):
        q = (lo + (hi - lo) * torch.rand(Q, D, generator=g)).float().cuda()
        f64 = dict(dtype=torch.float64, device="cuda")
        bufs = (torch.empty(Q, **f64), torch.empty(Q, **f64), torch.empty(Q, **f64),
                torch.empty(Q, D, dtype=torch.float32, device="cuda"))
        ms_grad = timed(lambda: gp._acquire(q, best, 0.0, "sor", grad=True, out=bufs), args.reps)
        ms_nograd = timed(lambda: gp._acquire(q, best, 0.0, "sor", grad=False, out=bufs), args.reps)
        ms_torch = timed(lambda: torch_acquire(gp, q, best), args.reps)
        k = gp._acquire(q, best, 0.0, "sor", grad=True)
        t = torch_acquire(gp, q, best)
        flop_nograd = 2.0 * Q * M * (M + 1)
        flop_grad = flop_nograd + 2.0 * Q * M * D
        rows.append({"Q": Q, "M": M, "D": D,
                     "kernel_ms": ms_grad, "kernel_ms_no_grad": ms_nograd, "torch_f64_ms": ms_torch,
                     "speedup_vs_torch": ms_torch / ms_grad,
                     "candidates_per_s": Q / (ms_grad * 1e-3),
                     "kernel_fp64_tflops": flop_grad / (ms_grad * 1e-3) / 1e12,
                     "kernel_fp64_tflops_no_grad": flop_nograd / (ms_nograd * 1e-3) / 1e12,
                     "torch_fp64_tflops": flop_grad / (ms_torch * 1e-3) / 1e12,
                     "max_abs_diff_mean": float((k[0] - t[0]).abs().max()),
                     "max_abs_diff_ei": float((k[2] - t[2]).abs().max()),
                     "max_rel_diff_grad": float((k[3] - t[3]).double().abs().max() / t[3].double().abs().max().clamp(min=1e-300)),
                     "max_abs_grad": float(t[3].abs().max())})
    # one asia search iteration
    from dags_vae_search_amd import BNLearnWrapper, LabeledGraph, PaceVaeV3, latent_bo_search
    ck = load_npz("asia_ckpt110.npz")
    graphs = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_predictor_graphs.npz"), 8)][:1024]
    vae = PaceVaeV3(8, 8, 32, 8, 3, 64, 32, 32, 0.15)
    vae.load_state_dict({k: torch.from_numpy(ck[k]) for k in ck.files})
    vae = vae.to("cuda:0").eval()
    ev = BNLearnWrapper("asia", args.metric, data=load_npz("bn_asia_data.npz")["data"])
    sgp = _gp(x[:1024], y[:1024])
    cfg = dict(iterations=args.iterations, batch_size=64, n_starts=1024, steps=50, lr=0.02, decode_tries=4, seed=0)
    t0 = time.perf_counter()
    res = latent_bo_search(vae, sgp, ev, graphs, **cfg)
    total = time.perf_counter() - t0
    last = res.history[-1]
    out = {"metric": "dvs_gp_acquire ms (Q = 16384, M = 500, D = 32, with dEI/dx)", "value": rows[1]["kernel_ms"],
           "unit": "ms", "acquire": rows,
           "search_iteration": {"config": dict(cfg, initial_graphs=len(graphs), metric=args.metric), "iteration": last.iteration,
                                "ms": {k: round(v, 3) for k, v in last.timings_ms.items()},
                                "seconds": last.seconds, "n_candidates": last.n_candidates, "n_valid": last.n_valid,
                                "n_new": last.n_new, "best_score": last.best_score, "ei_max": last.ei_max,
                                "total_seconds_all_iterations": total,
                                "new_structures_total": sum(h.n_new for h in res.history),
                                "best_score_initial": max(s for _, s in res.evaluated[:res.n_initial])}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
