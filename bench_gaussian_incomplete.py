"""Gaussian networks on incomplete data (include/dvs_gaussian_incomplete.h) at n = 8 / 11 / 37, the sizes of
bench_gaussian.py, on 10^5 and 10^6 rows drawn with ``gaussian_sample``, under three workloads: no cell missing (one pattern), 10 %
of the cells missing completely at random (at n = 37 nearly every row is its own pattern) and four fixed patterns.  The one-pattern
and the all-unique workloads are the two ends of the kernel's mapping: one factorisation per 256 rows, or one per row.

Times ``gaussian_condition`` with and without ``cov``, and one EM iteration split into E-step (joint + conditioning), moments and
fit.  The yardstick is the same computation in torch ops on the same device: the rows grouped by ``torch.unique`` of the mask, one
``torch.linalg.cholesky`` and triangular solves per pattern.  Its cost grows with the number of patterns, so where the rows hold
more than ``--patterns`` of them it is given the first ``--patterns`` rows, and the kernel is timed on those rows beside it,
alternately (``bench_gaussian_params.alternating_s``).  The two must agree to 1e-12 relative before anything is timed, or the run stops.
Writes profiles/gaussian_incomplete_bench.json.

    python bench_gaussian_incomplete.py [--rows 100000 1000000] [--repeats 5]
"""
import argparse
import json
import os

import numpy as np
import torch

from bench_gaussian_params import alternating_s, median_s, network
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd import gaussian_condition, gaussian_fit, gaussian_joint, gaussian_sample
from dags_vae_search_amd.gaussian import GaussianMomentsEvaluator, _moments
from dags_vae_search_amd.gaussian_incomplete import _condition, _joint, _order

HERE = os.path.dirname(os.path.abspath(__file__))
# Both sides factor the same well-conditioned blocks in fp64 in different orders; the relative difference of their cells is a
# few hundred u at n = 37.  1e-12 is ten thousand u: a wrong index or a missed update is many orders above it.
AGREEMENT = 1e-12
HALF_LOG_2PI = 0.9189385332046727


def masks_of(workload, S, n, seed=0):
    """int64 [S] on the device"""
    g = torch.Generator(device="cuda").manual_seed(3400 + n + seed)
    low = (1 << n) - 1
    if workload == "complete":
        return torch.full((S,), low, dtype=torch.int64, device="cuda")
    if workload == "mcar10":
        seen = torch.rand(S, n, device="cuda", generator=g) >= 0.1
        return (seen.long() << torch.arange(n, device="cuda")).sum(1)
    if workload == "four":
        rng = np.random.default_rng(3400 + n)
        pats = torch.tensor([low] + [int(rng.integers(0, 1 << n)) & low for _ in range(3)], dtype=torch.int64, device="cuda")
        return pats[torch.randint(0, 4, (S,), device="cuda", generator=g)]
    raise KeyError(workload)


SOLVE_COLUMNS = 65536


def solve_lower(L, B):
    """L^-1 B by torch.linalg.solve_triangular, the right-hand sides taken SOLVE_COLUMNS at a time: one call with 10^6 of them
    at n = 37 ended in an allocation failure of the BLAS underneath, one with 10^5 did not"""
    if B.shape[1] <= SOLVE_COLUMNS:
        return torch.linalg.solve_triangular(L, B, upper=False)
    return torch.cat([torch.linalg.solve_triangular(L, B[:, c:c + SOLVE_COLUMNS], upper=False) for c in range(0, B.shape[1], SOLVE_COLUMNS)], dim=1)


def torch_condition(mean, cov, x, observed, want_cov):
    """the conditioning a user would write in torch ops -> (completed, var or None, log_density, cov_sum or None)"""
    S, n = x.shape
    pats, inv = torch.unique(observed, return_inverse=True)
    order = torch.argsort(inv, stable=True)
    counts = torch.bincount(inv, minlength=pats.numel()).tolist()
    completed, logp = x.clone(), torch.empty(S, dtype=torch.float64, device=x.device)
    var = torch.zeros_like(x) if want_cov else None
    ccov = torch.zeros(n, n, dtype=torch.float64, device=x.device) if want_cov else None
    at = 0
    for m, cnt in zip(pats.tolist(), counts):
        rows = order[at:at + cnt]
        at += cnt
        O = torch.tensor([v for v in range(n) if (m >> v) & 1], dtype=torch.int64, device=x.device)
        M = torch.tensor([v for v in range(n) if not (m >> v) & 1], dtype=torch.int64, device=x.device)
        k = O.numel()
        if k:
            L = torch.linalg.cholesky(cov[O][:, O])
            y = solve_lower(L, (x[rows][:, O] - mean[O]).T)
            logp[rows] = -(k * HALF_LOG_2PI + torch.log(torch.diagonal(L)).sum() + 0.5 * (y * y).sum(0))
        else:
            logp[rows] = 0.0
        if M.numel():
            if k:
                R = solve_lower(L, cov[O][:, M])
                completed[rows[:, None], M[None, :]] = mean[M] + (R.T @ y).T
                T = cov[M][:, M] - R.T @ R
            else:
                completed[rows[:, None], M[None, :]] = mean[M].expand(cnt, -1)
                T = cov[M][:, M]
            if want_cov:
                var[rows[:, None], M[None, :]] = torch.diagonal(T).expand(cnt, -1)
                ccov[M[:, None], M[None, :]] += cnt * T
    return completed, var, logp, ccov


def agreement(got, want):
    """the largest difference of two tensors relative to the largest magnitude of the reference"""
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / scale if scale else float((got - want).abs().max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100000, 1000000])
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 11, 37])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--patterns", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gaussian_incomplete_bench.json"))
    args = ap.parse_args()
    lib = dl.load()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "yardstick_pattern_cap": args.patterns,
           "timing": "host clock around windows of back-to-back calls (about 50 ms each, sized from a probe call) that end in a "
                     "device synchronise; the median window of the repeats divided by its calls, after one warm-up call of every "
                     "shape; the kernel and the torch composition take their windows alternately",
           "condition": [], "em_iteration": []}
    for n in args.sizes:
        fitted = network(n, 1)
        mean, cov = (t[0] for t in gaussian_joint(fitted))
        net = (fitted.parents, fitted.coef, fitted.intercept, fitted.sd)
        for S in args.rows:
            x = gaussian_sample(fitted, S, seed=3)
            for workload in ("complete", "mcar10", "four"):
                observed = masks_of(workload, S, n)
                patterns = int(torch.unique(observed).numel())
                Sb = S if patterns <= args.patterns else args.patterns
                xb, ob = x[:Sb].contiguous(), observed[:Sb].contiguous()
                got = gaussian_condition(fitted, (xb, ob))
                want = torch_condition(mean, cov, xb, ob, True)
                worst = max(agreement(got.completed, want[0]), agreement(got.var, want[1]), agreement(got.log_density, want[2]),
                            agreement(got.cov_sum, want[3]) if float(want[3].abs().max()) else 0.0)
                if not worst < AGREEMENT or int(got.refused):
                    raise SystemExit(f"dvs_gbn_condition and the torch composition disagree at n {n} S {Sb} {workload}: {worst}")
                tk, tt = alternating_s(lambda: gaussian_condition(fitted, (xb, ob)), lambda: torch_condition(mean, cov, xb, ob, True),
                                       args.repeats)
                t_cov = tk if Sb == S else median_s(lambda: gaussian_condition(fitted, (x, observed)), args.repeats)
                t_lean = median_s(lambda: gaussian_condition(fitted, (x, observed), cov=False), args.repeats)
                t_unsorted = median_s(lambda: gaussian_condition(fitted, (x, observed), order=None), args.repeats)
                row = {"n": n, "rows": S, "workload": workload, "patterns": patterns, "ms": round(t_cov * 1e3, 4),
                       "ms_without_cov": round(t_lean * 1e3, 4), "ms_unsorted": round(t_unsorted * 1e3, 4), "rows_per_s": round(S / t_cov),
                       "baseline_rows": Sb, "baseline_patterns": int(torch.unique(ob).numel()),
                       "kernel_ms_at_baseline_rows": round(tk * 1e3, 4), "torch_ms_at_baseline_rows": round(tt * 1e3, 4),
                       "torch_over_kernel": round(tt / tk, 3), "largest_relative_difference": worst}
                res["condition"].append(row)
                print("condition", row, flush=True)
                # ---- one EM iteration, split: the E-step (joint + conditioning), the moments of the completed rows, the fit
                order = _order("bench", "sorted", observed)

                def e_step():
                    m, c, _ = _joint(lib, n, net, x.device)
                    return _condition(lib, n, m, c, x, observed, order, quad=False)[0]
                out = e_step()
                mom = _moments(lib, out.completed, None)
                mom[0, 1 + n:] += out.cov_sum.reshape(-1)
                ev = GaussianMomentsEvaluator("bench", "bic-g", mom)
                te = median_s(e_step, args.repeats)
                tm = median_s(lambda: _moments(lib, out.completed, None), args.repeats)
                tf = median_s(lambda: gaussian_fit(ev, fitted.parents), args.repeats)
                ts = median_s(lambda: torch.sort(observed, stable=True), args.repeats)
                row = {"n": n, "rows": S, "workload": workload, "e_step_ms": round(te * 1e3, 4), "moments_ms": round(tm * 1e3, 4),
                       "fit_ms": round(tf * 1e3, 4), "sort_ms_once_per_fit": round(ts * 1e3, 4)}
                res["em_iteration"].append(row)
                print("em_iteration", row, flush=True)
    res["not_measured"] = ["kernel times by rocprofv3 (only end-to-end call times are taken)", "n = 48", "the torch composition beyond "
                           "--patterns patterns", "gaussian_em_fit end to end (its iterations are the three parts above plus one read-back)"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
