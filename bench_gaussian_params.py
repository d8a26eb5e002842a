"""A fitted Gaussian network (include/dvs_gaussian_params.h) at n = 8 / 11 / 37, the sizes of bench_gaussian.py:
rows and bytes per second of ``dvs_gbn_sample`` at 10^6 rows beside the HBM write bound (8 n bytes a row); row·structures per
second of ``dvs_gbn_loglik`` at 10^6 rows and B = 1 / 16 / 256 beside the same computation written in torch ops on the device,
timed alternately in the same call; ``gaussian_cross_validate(folds=10)`` at 5000 rows beside the per-fold composition
``from_device`` + ``gaussian_fit`` + ``gaussian_log_likelihood``.  Seeded networks.  The kernel's result must agree with the torch
composition to 1e-12 relative at every shape, or the run stops.
Writes profiles/gaussian_params_bench.json.

    python bench_gaussian_params.py [--rows 1000000] [--cv-rows 5000] [--repeats 5]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import (FittedGBN, GaussianEvaluator, cv_folds, gaussian_cross_validate, gaussian_fit, gaussian_log_likelihood,
                                 gaussian_sample)

HERE = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK = 8.0e12            # bytes per second, the specification's peak
HBM_COPY = 6.29e12           # bytes per second, the measured float4 copy


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def window_of(fn, window=0.05):
    fn()                                                     # warm-up: code objects, allocations
    return max(1, min(2000, int(window / max(wall(fn)[0], 1e-6))))


def median_s(fn, repeats, window=0.05):
    """seconds per call: after a warm-up call, the median over ``repeats`` windows of back-to-back calls that end in a synchronise"""
    inner = window_of(fn, window)

    def many():
        for _ in range(inner):
            fn()
    return float(np.median([wall(many)[0] for _ in range(repeats)])) / inner


def alternating_s(fa, fb, repeats, window=0.05):
    """(seconds per call of fa, of fb): their windows taken alternately, so both see the same clocks and the same neighbours"""
    ia, ib = window_of(fa, window), window_of(fb, window)

    def many(fn, k):
        for _ in range(k):
            fn()
    ta, tb = [], []
    for _ in range(repeats):
        ta.append(wall(lambda: many(fa, ia))[0] / ia)
        tb.append(wall(lambda: many(fb, ib))[0] / ib)
    return float(np.median(ta)), float(np.median(tb))


def network(n, B, seed=0):
    """B seeded networks on n variables: a random order, up to three earlier variables as parents, coefficients in +-[0.3, 0.9]"""
    rng = np.random.default_rng(7000 + n + seed)
    par, coef = np.zeros((B, n), np.uint64), np.zeros((B, n, n))
    for b in range(B):
        order = rng.permutation(n)
        for k in range(1, n):
            v = int(order[k])
            for u in rng.choice(order[:k], size=min(k, int(rng.integers(0, 4))), replace=False):
                par[b, v] |= np.uint64(1 << int(u))
                coef[b, v, int(u)] = rng.uniform(0.3, 0.9) * rng.choice([-1.0, 1.0])
    return FittedGBN(torch.from_numpy(par.view(np.int64)).cuda(), torch.from_numpy(coef).cuda(),
                     torch.from_numpy(rng.uniform(-2.0, 2.0, (B, n))).cuda(), torch.from_numpy(rng.uniform(0.5, 2.0, (B, n))).cuda())


# The two log-likelihoods are sums of S n terms of like sign in fp64 in different orders: each is within (log2(S n) + n + 8) u of
# the exact sum relative to the sum of magnitudes, which here is the sum itself; 1e-12 is a thousand times that at S n = 4e7.
LOGLIK_AGREEMENT = 1e-12


def torch_loglik(fitted, x):
    """the log-likelihood a user would write in torch ops: one matrix product per call for the conditional means"""
    mu = fitted.intercept[:, None, :] + torch.matmul(x[None], fitted.coef.transpose(1, 2))           # [B, S, n]
    e = (x[None] - mu) / fitted.sd[:, None, :]
    return -(torch.log(fitted.sd).sum(1) * x.shape[0] + 0.9189385332046727 * x.shape[0] * x.shape[1] + 0.5 * (e * e).sum((1, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--cv-rows", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 11, 37])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gaussian_params_bench.json"))
    args = ap.parse_args()
    S = args.rows
    res = {"device": torch.cuda.get_device_name(0), "rows": S, "cv_rows": args.cv_rows, "repeats": args.repeats,
           "timing": "host clock around windows of back-to-back calls (about 50 ms each, sized from a probe call) that end in a "
                     "device synchronise; the median window of the repeats divided by its calls, after one warm-up call of every "
                     "shape; a kernel and its baseline take their windows alternately",
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_copy_bytes_per_s": HBM_COPY, "sample": [], "loglik": [], "cross_validate": []}
    for n in args.sizes:
        one = network(n, 1)
        t = median_s(lambda: gaussian_sample(one, S, seed=1), args.repeats)
        row = {"n": n, "rows": S, "ms": round(t * 1e3, 4), "rows_per_s": round(S / t), "bytes_per_s": round(8 * n * S / t),
               "share_of_hbm_peak": round(8 * n * S / t / HBM_PEAK, 4), "share_of_measured_copy": round(8 * n * S / t / HBM_COPY, 4),
               "write_bound_ms": round(8 * n * S / HBM_PEAK * 1e3, 4)}
        res["sample"].append(row)
        print("sample", row, flush=True)
        x = gaussian_sample(one, S, seed=2)
        for B in args.batches:
            fitted = network(n, B)
            # the torch composition holds [B, S, n] doubles twice over: it is given as many rows as fit in about 2 GB
            Sb = min(S, max(1000, int(2e9 / (16 * B * n))))
            xb = x[:Sb]
            a = gaussian_log_likelihood(fitted, xb)
            b = torch_loglik(fitted, xb)
            rel = float(((a - b) / b).abs().max())
            if not rel < LOGLIK_AGREEMENT:
                raise SystemExit(f"dvs_gbn_loglik and the torch composition disagree at n {n} B {B}: relative difference {rel}")
            tk, tt = alternating_s(lambda: gaussian_log_likelihood(fitted, xb), lambda: torch_loglik(fitted, xb), args.repeats)
            tfull = tk if Sb == S else median_s(lambda: gaussian_log_likelihood(fitted, x), args.repeats)
            row = {"n": n, "batch": B, "rows": S, "ms": round(tfull * 1e3, 4), "row_structures_per_s": round(B * S / tfull),
                   "data_bytes_per_s": round(8 * n * S / tfull), "baseline_rows": Sb, "kernel_ms_at_baseline_rows": round(tk * 1e3, 4),
                   "torch_ms_at_baseline_rows": round(tt * 1e3, 4), "torch_row_structures_per_s": round(B * Sb / tt),
                   "kernel_over_torch": round(tt / tk, 3), "largest_relative_difference": rel}
            res["loglik"].append(row)
            print("loglik", row, flush=True)
        # ---- cross-validation at cv_rows: one call against the per-fold composition
        Sc = args.cv_rows
        xc = x[:Sc].contiguous()
        ev = GaussianEvaluator.from_device(f"syn{n}", "bic-g", xc)
        for B in (1, 64):
            parents = network(n, B).parents

            def composition():
                parts = [torch.from_numpy(p).cuda() for p in cv_folds(Sc, 10, 0)]
                total = None
                for f, part in enumerate(parts):
                    rest = torch.cat([p for g, p in enumerate(parts) if g != f])
                    fit = gaussian_fit(GaussianEvaluator.from_device("rest", "bic-g", xc[rest]), parents)
                    ll = gaussian_log_likelihood(fit, xc[part])
                    total = ll if total is None else total + ll
                return -total / Sc
            same = gaussian_cross_validate(ev, parents).cpu().numpy().tobytes() == composition().cpu().numpy().tobytes()
            tc, tp = alternating_s(lambda: gaussian_cross_validate(ev, parents), composition, args.repeats)
            row = {"n": n, "batch": B, "rows": Sc, "folds": 10, "ms": round(tc * 1e3, 3), "composition_ms": round(tp * 1e3, 3),
                   "composition_over_call": round(tp / tc, 3), "equal_bytes": bool(same)}
            res["cross_validate"].append(row)
            print("cross_validate", row, flush=True)
    res["not_measured"] = ["kernel times by rocprofv3 (only end-to-end call times are taken)", "n = 48", "dvs_gbn_predict and dvs_gbn_joint",
                           "row counts other than --rows and --cv-rows"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
