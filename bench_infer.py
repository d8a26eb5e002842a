"""Inference on a fitted network (dvs_bn_lw, dvs_bn_blanket_posterior): weighted particles per second of one
likelihood-weighting query at 10^6 and 10^7 particles (without evidence, next to dvs_bn_sample's rows per second on the same
tables, and with evidence and a target), rows per second of predict(method="bayes-lw") at 10^5 rows x 500 particles and of the
exact path, on asia (n = 8), sachs (n = 11) and a seeded 37-variable / 4-level data set, each by wall time and by the
library's HIP-event kernel time, next to the numpy restatement of tests/infer_corpus.py on the CPU (a reference, not a tuned
CPU implementation).  Writes profiles/infer_bench.json.

    python bench_infer.py [--repeats 5] [--particles 1000000 10000000] [--rows 100000]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_params import datasets, kernels_ms, random_dag, timed
from dags_vae_search_amd import BNLearnWrapper, bn_fit, predict, sample
from dags_vae_search_amd import infer
from tests import infer_corpus as ic
from tests import params_corpus as pm
from tests import scoring_corpus as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_total(kern):
    return sum(k["ms"] for k in kern.values()) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--particles", type=int, nargs="+", default=[1000000, 10000000])
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--predict-particles", type=int, default=500)
    ap.add_argument("--cpu-particles", type=int, default=20000)
    ap.add_argument("--cpu-rows", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "infer_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "lw": [], "predict": []}

    for name, data, known in datasets():
        ev = BNLearnWrapper(name, "bic", data=data)
        card = (data.max(0) + 1).astype(np.uint8)
        n = ev.n_vars
        rng = np.random.default_rng(1000 + n)
        masks = sc.masks_of(n, known if known is not None else random_dag(rng, n))
        fitted = bn_fit(ev, torch.from_numpy(masks.view(np.int64)).cuda(), method="bayes", iss=10.0)
        net = pm.Network(name, card, masks[0], [fitted.table(v).cpu().numpy() for v in range(n)])
        base = {"name": name, "n": n, "cells": int(fitted.cpt.numel())}
        target = n - 1
        one = ev.packed[:1].contiguous()
        none = torch.zeros(1, dtype=torch.int64, device="cuda")
        some = torch.tensor([1 | (1 << (n // 2))], dtype=torch.int64, device="cuda")      # two observed variables

        for M in args.particles:
            run = lambda: sample(fitted, M, seed=1)
            ms, kern = timed(run, args.repeats), kernels_ms(run)
            sample_rate, sample_kernel_rate = M / (ms * 1e-3), M / kernel_total(kern)
            for what, observed, targets in (("no evidence", none, 0), ("evidence, one target", some, 1 << target)):
                run = lambda: infer._lw(fitted, one, observed, n_particles=M, seed=1, targets=targets)
                ms, kern = timed(run, args.repeats), kernels_ms(run)
                row = dict(base, case=what, particles=M, ms=ms, particles_per_s=M / (ms * 1e-3),
                           kernel_particles_per_s=M / kernel_total(kern), kernels=kern)
                if targets == 0:
                    row.update(sample_rows_per_s=sample_rate, sample_kernel_rows_per_s=sample_kernel_rate,
                               lw_over_sample_kernel_time=sample_kernel_rate / row["kernel_particles_per_s"])
                if M == args.particles[0]:
                    levels = pm.unpack(one.cpu().numpy().view(np.uint64), n)
                    t0 = time.perf_counter()
                    ic.lw_ref(net, levels, [int(observed[0])], args.cpu_particles, 1, 0, None, targets)
                    row["cpu_particles"], row["cpu_particles_per_s"] = args.cpu_particles, args.cpu_particles / (time.perf_counter() - t0)
                res["lw"].append(row)
                print(row, flush=True)

        rows = sample(fitted, args.rows, seed=2)
        levels = pm.unpack(rows[:args.cpu_rows].cpu().numpy().view(np.uint64), n)
        for method in ("bayes-lw", "exact", "parents"):
            run = lambda: predict(fitted, target, rows, method=method, n=args.predict_particles, seed=3, prob=True)
            ms, kern = timed(run, args.repeats), kernels_ms(run)
            t0 = time.perf_counter()
            if method == "bayes-lw":
                ic.predict_lw_ref(net, levels, target, args.predict_particles, 3)
            else:
                ic.blanket_ref(levels, card, masks[0], net.tables, target, method == "exact")
            cpu_s = time.perf_counter() - t0
            row = dict(base, method=method, rows=args.rows, particles=args.predict_particles if method == "bayes-lw" else None,
                       target=target, ms=ms, rows_per_s=args.rows / (ms * 1e-3), kernel_rows_per_s=args.rows / kernel_total(kern),
                       cpu_rows=args.cpu_rows, cpu_rows_per_s=args.cpu_rows / cpu_s, kernels=kern)
            res["predict"].append(row)
            print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
