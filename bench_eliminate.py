"""Exact inference by variable elimination (dvs_bn_eliminate): queries per second of exact_posterior over all
targets on asia (n = 8, bayes tables) and on the 48-variable banded network of tests/eliminate_corpus.py, Q rows drawn by
``sample`` with half the variables observed, each by wall time and by the library's HIP-event kernel time; the same queries
through ``posterior`` (likelihood weighting, 10 000 particles per query, on fewer rows: it is several orders slower); the numpy
restatement of tests/eliminate_corpus.py on the CPU (a reference, not a tuned CPU implementation); and the rows-per-workgroup
sweep of one target's plan: the library's rule G, G halved and G doubled through the rows_per_group argument.  Nothing is
asserted about speed.  Writes profiles/eliminate_bench.json.

    python bench_eliminate.py [--repeats 5] [--rows 65536] [--lw-rows 256] [--cpu-rows 512]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_params import kernels_ms, timed
from dags_vae_search_amd import FittedBN, exact_posterior, posterior, sample
from dags_vae_search_amd import eliminate as el
from tests import eliminate_corpus as ec

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_total(kern):
    return sum(k["ms"] for k in kern.values()) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--lw-rows", type=int, default=256)
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--cpu-rows", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "eliminate_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": args.rows, "posterior": [], "sweep": []}

    for name in ("asia", "band48"):
        net = ec.network(name)
        n = len(net.card)
        fitted = FittedBN.from_tables([int(m) for m in net.masks], net.card, net.tables)
        rows = sample(fitted, args.rows, seed=2)
        rng = np.random.default_rng(100 + n)
        observed = torch.tensor([sum(1 << int(v) for v in rng.choice(n, size=n // 2, replace=False)) for _ in range(args.rows)],
                                dtype=torch.int64, device="cuda")
        targets = list(range(n))
        plans = [el.elimination_plan(fitted, (v,)) for v in targets]
        base = {"name": name, "n": n, "targets": n, "width": max(p.width for p in plans),
                "arena_cells": max(p.arena_cells for p in plans), "max_step_cells": max(p.max_step_cells for p in plans),
                "plan_words": max(len(p.words) for p in plans)}

        run = lambda: exact_posterior(fitted, targets, (rows, observed), plan=plans)
        ms, kern = timed(run, args.repeats), kernels_ms(run)
        row = dict(base, method="exact_posterior", rows=args.rows, ms=ms, queries_per_s=args.rows / (ms * 1e-3),
                   kernel_queries_per_s=args.rows / kernel_total(kern), kernels=kern)
        res["posterior"].append(row)
        print(row, flush=True)

        few = (rows[:args.lw_rows].contiguous(), observed[:args.lw_rows].contiguous())
        run = lambda: posterior(fitted, targets, few, n=args.particles, seed=3)
        ms, kern = timed(run, args.repeats), kernels_ms(run)
        row = dict(base, method="posterior (likelihood weighting)", rows=args.lw_rows, particles=args.particles, ms=ms,
                   queries_per_s=args.lw_rows / (ms * 1e-3), kernel_queries_per_s=args.lw_rows / kernel_total(kern), kernels=kern)
        res["posterior"].append(row)
        print(row, flush=True)

        masks = el.level_masks(fitted, rows[:args.cpu_rows], observed[:args.cpu_rows]).cpu().numpy().view(np.uint16)
        t0 = time.perf_counter()
        for p in plans:
            ec.execute_plan(p.words, net.card, net.tables, masks)
        row = dict(base, method="numpy restatement (CPU)", rows=args.cpu_rows, queries_per_s=args.cpu_rows / (time.perf_counter() - t0))
        res["posterior"].append(row)
        print(row, flush=True)

        # the rows per workgroup: the library's rule and its neighbours, on the plan of the middle target over every row
        plan = plans[n // 2]
        masks_dev = el.level_masks(fitted, rows, observed)
        rule = max(1, min(64, 1024 // plan.max_step_cells, el.MAX_CELLS // plan.arena_cells))
        for G in sorted({max(1, rule // 2), rule, min(64, rule * 2), 1, 64}):
            run = lambda: el.run_plans(fitted, [plan], masks_dev, rows_per_group=G)
            ms, kern = timed(run, args.repeats), kernels_ms(run)
            row = dict(name=name, target=n // 2, rows=args.rows, rows_per_group=G, is_rule=G == rule, ms=ms,
                       kernel_ms=kern.get("k_bn_eliminate", {}).get("ms"), kernel_rows_per_s=args.rows / kernel_total(kern))
            res["sweep"].append(row)
            print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
