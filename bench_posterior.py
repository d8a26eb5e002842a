"""Exact arc posterior (dvs_arc_posterior): the time to build the local-score table and the time of the dynamic
programme alone on asia (n = 8), sachs (n = 11, at most 3 parents) and the synthetic n = 12 set; the programme alone on random
tables at n = 8, 9, 10 (both sides of the one-workgroup chain), 12, 16 and 20 with its per-kernel times, next to
dvs_exact_search on the same tables for scale; and on asia with bde, the largest distance between the exact posterior's arc
strength and boot_strength(replicates=200).  Writes profiles/posterior_bench.json.

    python bench_posterior.py [--repeats 5]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, _lib as dl
from dags_vae_search_amd import arc_posterior, arc_posterior_from_tables, boot_strength, exact_from_tables, local_score_table
from tests import hillclimb_corpus as hc

HERE = os.path.dirname(os.path.abspath(__file__))


def timed(fn, repeats):
    """median wall time in ms of fn(), the device drained before and after"""
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def kernels_ms(fn):
    lib = dl.load()
    lib.dvs_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    prof = dl.profile_collect(lib)
    lib.dvs_profile_enable(0)
    return {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in prof.items() if k.startswith("k_post")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "posterior_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "data": [], "random": [], "asia_bde_vs_bootstrap": None}

    for name, case, cap in (("asia", "asia", None), ("sachs", "sachs", 3), ("syn12", None, None)):
        if case is None:
            from tests import scoring_corpus as sc
            data, _ = sc.synthetic_dataset(12, 2000, np.random.default_rng(12).integers(2, 4, 12), seed=912)
        else:
            data = hc.hc_case(case).data
        ev = BNLearnWrapper(name, "bde", data=data, iss=10.0)
        table = local_score_table(ev, max_parents=cap)
        post = arc_posterior_from_tables(table[None], max_parents=cap)
        row = {"name": name, "n": ev.n_vars, "samples": ev.n_samples, "max_parents": cap, "score": "bde iss 10",
               "table_ms": timed(lambda: local_score_table(ev, max_parents=cap), args.repeats),
               "dp_ms": timed(lambda: arc_posterior_from_tables(table[None], max_parents=cap), args.repeats),
               "dp_kernels": kernels_ms(lambda: arc_posterior_from_tables(table[None], max_parents=cap)),
               "log_z": float(post.log_z[0]), "log_z_back": float(post.log_z_back[0]),
               "arcs_above_half": int((post.prob[0] > 0.5).sum())}
        res["data"].append(row)
        print(row, flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    for n, batch in ((8, 1), (8, 1024), (9, 1), (10, 1), (12, 1), (16, 1), (20, 1)):
        tables = torch.randn(batch, 1 << n, n, dtype=torch.float64, device="cuda", generator=gen)
        row = {"n": n, "batch": batch, "cells": batch * (1 << n) * n,
               "dp_ms": timed(lambda: arc_posterior_from_tables(tables), args.repeats),
               "dp_kernels": kernels_ms(lambda: arc_posterior_from_tables(tables)),
               "exact_search_ms": timed(lambda: exact_from_tables(tables), args.repeats),
               "workspace_mb": dl.load().dvs_arc_posterior_workspace_bytes(batch, n) / 2 ** 20}
        res["random"].append(row)
        print(row, flush=True)
        del tables

    case = hc.hc_case("asia")
    ev = BNLearnWrapper("asia", "bde", data=case.data, iss=10.0)
    post = arc_posterior(ev)
    boot = boot_strength(ev, replicates=200, algorithm_args={"max_steps": 60, "min_delta": case.min_delta}, seed=1)
    gap = (post.strength[0] - boot.strength).abs()
    u, v = divmod(int(gap.argmax()), ev.n_vars)
    res["asia_bde_vs_bootstrap"] = {"replicates": 200, "largest_strength_gap": float(gap.max()), "at": [u, v],
                                    "exact": float(post.strength[0, u, v]), "bootstrap": float(boot.strength[u, v]),
                                    "mean_strength_gap": float(gap.mean())}
    print(res["asia_bde_vs_bootstrap"], flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
