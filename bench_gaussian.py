"""Gaussian networks (include/dvs_gaussian.h) at 5000 rows: moment rows per second of ``dvs_gbn_moments`` at
n = 8 / 11 / 37 for one set and for 200 row sets; families per second of ``dvs_gbn_scores`` through ``local_score_table``;
structures per second of the toggle pass, beside the discrete ``dvs_bn_toggle_scores`` at the same n and S (the same rows cut
into three levels at their terciles); ``hill_climb`` and ``boot_strength(replicates=200)`` end to end — each beside the numpy
restatement of the header's definitions on the CPU (tests/gaussian_corpus.py), timed on a share of the work and scaled.
Seeded linear-Gaussian data (``gauss_data``).  Writes profiles/gaussian_bench.json.

    python bench_gaussian.py [--rows 5000] [--repeats 5] [--replicates 200]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, GaussianEvaluator, boot_strength, bootstrap_rows, hill_climb, local_score_table
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd.gaussian import _moments
from tests import gaussian_corpus as gc

HERE = os.path.dirname(os.path.abspath(__file__))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_s(fn, repeats, window=0.05):
    """seconds per call: after a warm-up call, the median over ``repeats`` windows of back-to-back calls, each window sized
    from one probe call to last about ``window`` seconds (a window of microseconds would time the clock and the scheduler)"""
    fn()                                                     # warm-up: code objects, allocations
    inner = max(1, min(2000, int(window / max(wall(fn)[0], 1e-6))))

    def many():
        for _ in range(inner):
            fn()
    return float(np.median([wall(many)[0] for _ in range(repeats)])) / inner


def cpu_s(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def discretised(x):
    """the rows cut at each column's terciles -> level codes 0..2 (the discrete scorer's input at the same n and S)"""
    q = np.quantile(x, [1 / 3, 2 / 3], axis=0)
    return ((x > q[0]).astype(np.uint8) + (x > q[1]).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 11, 37])
    ap.add_argument("--table-sizes", type=int, nargs="+", default=[8, 11, 20])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gaussian_bench.json"))
    args = ap.parse_args()
    S, R = args.rows, args.replicates
    res = {"device": torch.cuda.get_device_name(0), "rows": S, "repeats": args.repeats, "replicates": R,
           "timing": "host clock around windows of back-to-back calls (about 50 ms each, sized from a probe call) that end in a "
                     "device synchronise; the median window of the repeats divided by its calls, after one warm-up call; the "
                     "numpy restatement is timed once on the stated share of the work",
           "moments": [], "local_score_table": [], "toggle": [], "hill_climb": [], "boot_strength": []}
    lib = dl.load()
    for n in args.sizes:
        x = np.array(gc.gauss_data(n, S))
        ev = GaussianEvaluator(f"syn{n}", "bic-g", data=x)
        # ---- moments: one set, and R bootstrap sets in one call
        rows = bootstrap_rows(R, S, S, seed=1)
        t1 = median_s(lambda: _moments(lib, ev.x, None), args.repeats)
        tR = median_s(lambda: _moments(lib, ev.x, rows), args.repeats)
        t_np = cpu_s(lambda: gc.restated_moments(x[:640]))
        row = {"n": n, "one_set_ms": round(t1 * 1e3, 4), "one_set_rows_per_s": round(S / t1),
               f"sets_{R}_ms": round(tR * 1e3, 4), f"sets_{R}_rows_per_s": round(R * S / tR),
               "numpy_restatement_rows_per_s": round(640 / t_np), "numpy_rows_timed": 640}
        res["moments"].append(row)
        print("moments", row, flush=True)
        # ---- the toggle pass: B structures, all n^2 cells each; the discrete pass on the same rows in three levels
        B = 256
        P = torch.from_numpy(gc.random_dags(n, B, 3, seed=n).view(np.int64)).cuda()
        disc = BNLearnWrapper(f"syn{n}-3", "bic", data=discretised(x))
        for name, e in (("bic-g", ev), ("bge", GaussianEvaluator(f"syn{n}", "bge", data=x)), ("discrete bic", disc)):
            out = e.toggle_scores(P)
            t = median_s(lambda: e.toggle_scores(P, out=out), args.repeats)
            row = {"n": n, "score": name, "batch": B, "ms": round(t * 1e3, 4), "structures_per_s": round(B / t),
                   "cells_per_s": round(B * n * n / t)}
            res["toggle"].append(row)
            print("toggle", row, flush=True)
        # ---- hill_climb and boot_strength end to end, Gaussian beside discrete
        steps = 6 * n
        for name, e in (("bic-g", ev), ("discrete bic", disc)):
            t = median_s(lambda: hill_climb(e, batch=64, max_steps=steps), args.repeats)
            r = hill_climb(e, batch=64, max_steps=steps)
            row = {"n": n, "score": name, "batch": 64, "max_steps": steps, "steps": int(r.steps[0]), "converged": int(r.converged.sum()),
                   "ms": round(t * 1e3, 3)}
            res["hill_climb"].append(row)
            print("hill_climb", row, flush=True)
            t = median_s(lambda: boot_strength(e, replicates=R, algorithm_args=dict(max_steps=steps), seed=1), max(2, args.repeats // 2))
            s = boot_strength(e, replicates=R, algorithm_args=dict(max_steps=steps), seed=1)
            row = {"n": n, "score": name, "replicates": R, "max_steps": steps, "exhausted": s.exhausted, "ms": round(t * 1e3, 3),
                   "replicates_per_s": round(R / t, 1)}
            res["boot_strength"].append(row)
            print("boot_strength", row, flush=True)
    # ---- families per second of dvs_gbn_scores through local_score_table; beyond the cap a family is refused at once
    for n in args.table_sizes:
        x = np.array(gc.gauss_data(n, S))
        for metric in ("bic-g", "bge"):
            e = GaussianEvaluator(f"syn{n}", metric, data=x)
            t = median_s(lambda: local_score_table(e), args.repeats)
            fams = (1 << n) * n
            mom = e.moments[0].cpu().numpy()
            share = 2000
            t_np = cpu_s(lambda: [gc.restated_local(mom, n, k % n, (k * 2654435761) % (1 << n), metric) for k in range(share)])
            row = {"n": n, "metric": metric, "families": fams, "ms": round(t * 1e3, 3), "families_per_s": round(fams / t),
                   "refused_share": round(float(torch.isnan(local_score_table(e)).double().mean()), 4),
                   "numpy_restatement_families_per_s": round(share / t_np), "numpy_families_timed": share}
            res["local_score_table"].append(row)
            print("local_score_table", row, flush=True)
    res["not_measured"] = ["kernel times by rocprofv3 (only end-to-end call times are taken)", "shares of peak",
                           "row counts other than --rows", "n = 48", "tabu_search, exact_search, order_mcmc on Gaussian data"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
