"""Exact structure search (dvs_exact_search): the time to build the local-score table and the time of the dynamic
programme alone on asia (n = 8), sachs (n = 11, at most 3 parents) and the synthetic n = 12 set; the programme alone on random
tables at n = 8, 9, 10 (both sides of the one-workgroup sink walk), 12, 16 and 20; and on asia, for every score type, the gap
between the exact optimum and the bests of hill_climb and tabu_search from the empty graph with the SHD between their CPDAGs.
Writes profiles/exact_bench.json.

    python bench_exact.py [--repeats 5]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, _lib as dl
from dags_vae_search_amd import compare_structures, exact_from_tables, exact_search, hill_climb, local_score_table, tabu_search
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
    return {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in prof.items() if k.startswith("k_exact")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "exact_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "data": [], "random": [], "asia_gaps": []}

    for name, case, cap in (("asia", "asia", None), ("sachs", "sachs", 3), ("syn12", None, None)):
        if case is None:
            from tests import scoring_corpus as sc
            data, _ = sc.synthetic_dataset(12, 2000, np.random.default_rng(12).integers(2, 4, 12), seed=912)
        else:
            data = hc.hc_case(case).data
        ev = BNLearnWrapper(name, "bic", data=data)
        table = local_score_table(ev, max_parents=cap)
        row = {"name": name, "n": ev.n_vars, "samples": ev.n_samples, "max_parents": cap,
               "table_ms": timed(lambda: local_score_table(ev, max_parents=cap), args.repeats),
               "dp_ms": timed(lambda: exact_from_tables(table[None], max_parents=cap), args.repeats),
               "dp_kernels": kernels_ms(lambda: exact_from_tables(table[None], max_parents=cap)),
               "score": float(exact_search(ev, max_parents=cap).scores[0])}
        res["data"].append(row)
        print(row, flush=True)

    gen = torch.Generator(device="cuda").manual_seed(1)
    for n, batch in ((8, 1), (8, 1024), (9, 1), (10, 1), (12, 1), (16, 1), (20, 1)):
        tables = torch.randn(batch, 1 << n, n, dtype=torch.float64, device="cuda", generator=gen)
        ms = timed(lambda: exact_from_tables(tables), args.repeats)
        cells = batch * (1 << n) * n
        row = {"n": n, "batch": batch, "cells": cells, "dp_ms": ms, "dp_kernels": kernels_ms(lambda: exact_from_tables(tables)),
               "workspace_mb": dl.load().dvs_exact_workspace_bytes(batch, n) / 2 ** 20}
        res["random"].append(row)
        print(row, flush=True)
        del tables

    case = hc.hc_case("asia")
    for typ in dl.SCORE_TYPES:
        ev = BNLearnWrapper("asia", typ, data=case.data, **({"iss": 10.0} if typ in ("bde", "bds") else {}))
        opt = exact_search(ev)
        row = {"type": typ, "exact": float(opt.scores[0]), "rescored": float(opt.rescored[0])}
        for what, r in (("hill_climb", hill_climb(ev, batch=1, max_steps=60, min_delta=case.min_delta)),
                        ("tabu_search", tabu_search(ev, batch=1, max_steps=100, tabu=10, min_delta=case.min_delta))):
            row[what] = {"score": float(r.scores[0]), "gap": float(opt.scores[0] - r.scores[0]), "steps": int(r.steps[0]),
                         "cpdag_shd": int(compare_structures(r.parents, opt.parents[0]).shd[0])}
        res["asia_gaps"].append(row)
        print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
