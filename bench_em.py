"""Learning from incomplete data (dvs_bn_expected_counts, dvs_bn_fit_counts, dvs_bn_impute): one E-step on asia
(n = 8, bayes tables) and on the 48-variable banded network of tests/eliminate_corpus.py, rows drawn by ``sample`` with 10 % and
30 % of the values missing completely at random, against the composition a user could write before it — ``run_plans`` over ALL
rows for every family, a torch division and a sum over the rows — measured in the same call, alternating, median of the wall
times with a device synchronise; the kernel times come from the library's HIP events in a run of their own.  The level masks
the composition needs are built outside its timed region (which flatters it).  Also: seconds per EM iteration (E-step, M-step
and the one read-back), the rows per second of ``impute``, and the rows-per-group sweep of the fused pass.  Nothing is asserted
about speed.  Writes profiles/em_bench.json.

    python bench_em.py [--repeats 5] [--rows 65536]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_params import kernels_ms
from dags_vae_search_amd import FittedBN, em_fit, expected_counts, family_plans, impute, sample, target_plans
from dags_vae_search_amd import eliminate as el
from tests import eliminate_corpus as ec

HERE = os.path.dirname(os.path.abspath(__file__))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternating(fns, repeats):
    """the median wall time in ms of every function, one run of each in turn per round, after one warm-up round"""
    for fn in fns:
        fn()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            times[i].append(wall_ms(fn))
    return [float(np.median(t)) for t in times]


def composition(fitted, plans, masks):
    """the expected counts of every family in the plan's layout, as the functions of eliminate.py compose them: every (family,
    row) pair is eliminated, [rows, cells] fp64 per family goes through global memory, the sum's order is torch's"""
    out = []
    for plan in plans:
        cells, z = el.run_plans(fitted, [plan], masks)
        out.append((cells[0] / z[0][:, None]).sum(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "em_bench.json"))
    args = ap.parse_args()
    R = args.rows
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": R, "e_step": [], "sweep": [], "em": [], "impute": []}
    for name in ("asia", "band48"):
        net = ec.network(name)
        n = len(net.card)
        fitted = FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables)
        rows = sample(fitted, R, seed=2)
        plans, targets = family_plans(fitted), target_plans(fitted)
        rule = max(1, min(64, 1024 // max(p.max_step_cells for p in plans)))
        base = {"name": name, "n": n, "arena_cells": max(p.arena_cells for p in plans), "out_cells": max(p.out_cells for p in plans),
                "max_step_cells": max(p.max_step_cells for p in plans), "plan_words": max(len(p.words) for p in plans), "rule_G": rule}
        for rate in (0.1, 0.3):
            seen = np.random.default_rng(200 + n).random((R, n)) >= rate
            observed = torch.from_numpy((seen.astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)).cuda()
            data = (rows, observed)
            fam = np.array([[u == v or (int(net.masks[v]) >> u) & 1 for u in range(n)] for v in range(n)])
            share = float(np.mean([(~seen[:, fam[v]]).any(1).mean() for v in range(n)]))
            masks = el.level_masks(fitted, rows, observed)
            fused = lambda: expected_counts(fitted, data, plans=plans)
            comp = lambda: composition(fitted, plans[:n], masks)
            ms_fused, ms_comp = alternating([fused, comp], args.repeats)
            kern_fused, kern_comp = kernels_ms(fused), kernels_ms(comp)
            got, ref = fused(), comp()
            worst = max(float(((got.table(v).sum() - ref[v].sum()).abs() / R).item()) for v in range(n))
            row = dict(base, missing=rate, pairs_with_a_missing_member=share, fused_ms=ms_fused, composition_ms=ms_comp,
                       ratio=ms_comp / ms_fused, fused_kernels=kern_fused, composition_kernels=kern_comp,
                       fused_kernel_ms=sum(k["ms"] for k in kern_fused.values()), composition_kernel_ms=sum(k["ms"] for k in kern_comp.values()),
                       skipped=int(got.skipped.item()), largest_difference_of_a_family_total_per_row=worst)
            res["e_step"].append(row)
            print(row, flush=True)

            iters = 5
            run = lambda: em_fit([int(m) for m in net.masks], net.card, data, max_iter=iters, tol=0.0)
            (ms,) = alternating([run], args.repeats)
            row = dict(name=name, missing=rate, rows=R, iterations=iters, ms=ms, seconds_per_iteration=ms * 1e-3 / iters)
            res["em"].append(row)
            print(row, flush=True)

            run = lambda: impute(fitted, data, plans=targets)
            (ms,), kern = alternating([run], args.repeats), kernels_ms(run)
            row = dict(name=name, missing=rate, rows=R, ms=ms, rows_per_s=R / (ms * 1e-3),
                       kernel_rows_per_s=R / (sum(k["ms"] for k in kern.values()) * 1e-3), kernels=kern)
            res["impute"].append(row)
            print(row, flush=True)

            if rate == 0.3:                                      # the rows per group of the fused pass, kernel time
                for G in sorted({1, 2, 4, 8, 16, 32, 64, rule}):
                    run = lambda: expected_counts(fitted, data, plans=plans, rows_per_group=G)
                    (ms,), kern = alternating([run], 3), kernels_ms(run)
                    row = dict(name=name, missing=rate, rows=R, rows_per_group=G, is_rule=G == rule, ms=ms,
                               counts_kernel_ms=kern.get("k_bn_inc_counts", {}).get("ms"),
                               evidence_kernel_ms=kern.get("k_bn_inc_evidence", {}).get("ms"))
                    res["sweep"].append(row)
                    print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
