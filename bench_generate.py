#!/usr/bin/env python3
"""Throughput of the device graph generator (generate.generate_dags, csrc/dvs_generate.h): graphs/s per launch next to
synthetic.synthetic_dags (the host loop it replaces) in the same process, the lanes-per-DAG comparison, and the time of one
curriculum data set.
    python bench_generate.py [--reps 20] [--out profiles/generate_bench.json]
Prints one JSON line and writes it to --out.  (The driver's metric is bench.py; this is the measurement of the generator row.)"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
STEP_MS = (1.19, 1.23)         # the n = 12, B = 4096 train step


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):                       # best of 3 blocks of `reps` back-to-back launches
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "generate_bench.json"))
    args = ap.parse_args()
    from dags_vae_search_amd import _lib as dl
    from dags_vae_search_amd import create_encoder_dataset, encoder_dag_train_schema, generate_dags
    from dags_vae_search_amd._lib import nbytes, ptr, stream
    from dags_vae_search_amd.generate import draw_edge_counts
    from dags_vae_search_amd.synthetic import synthetic_dags
    dev = "cuda:0"
    lib = dl.load()
    rows = []

    def case(n, card, B, m, what):
        if m == "mixture":
            edges = draw_edge_counts(encoder_dag_train_schema(n, 0.4, 20), B, seed=1, device=dev)
        else:
            edges = torch.full((B,), m, dtype=torch.int32, device=dev)
        dt = timed(lambda: generate_dags(n, card, edges, seed=1), args.reps)
        _, attempts = generate_dags(n, card, edges, seed=1)
        row = {"n": n, "card": card, "batch": B, "edges": m, "ms": dt * 1e3, "graphs_per_s": B / dt,
               "mean_attempts": float(attempts[attempts > 0].float().mean()), "failed": int((attempts == 0).sum())}
        # lanes per DAG: the library's choice (above) against every fixed group size, raw ABI calls on preallocated buffers
        wide = n > 13
        labels = torch.empty((B, n), dtype=torch.uint8, device=dev)
        preds = torch.empty((B, n), dtype=torch.int64 if wide else torch.int16, device=dev)
        groups = {}
        for k in range(0, 8):
            def call():
                dl.check(lib, lib.dvs_generate_dags(B, n, card, 1 if wide else 0, ptr(edges), 1, 0, 100, k << dl.GEN_GROUP_SHIFT,
                                                    ptr(labels), ptr(preds), nbytes(preds), ptr(attempts), stream()), what)
            groups["auto" if k == 0 else str(1 << (k - 1))] = timed(call, args.reps) * 1e3
        row["kernel_ms_by_lanes_per_dag"] = groups
        rows.append(row)
        return row

    for B in (4096, 65536):
        for m in (11, 26, "mixture"):
            case(12, 12, B, m, "n12")
    case(37, 37, 2048, 133, "n37")
    stream_row = next(r for r in rows if r["batch"] == 4096 and r["edges"] == "mixture")

    t0 = time.perf_counter()
    synthetic_dags(12, 12, 2000, seed=1)
    host = 2000 / (time.perf_counter() - t0)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ds = create_encoder_dataset(12, 12, 200, 20, 0.4, seed=1, device=dev)
    torch.cuda.synchronize()
    t_ds = time.perf_counter() - t0
    out = {"metric": "graphs/sec generate_dags, n=12 batch 4096, curriculum mixture", "value": stream_row["graphs_per_s"],
           "unit": "graphs/s", "cases": rows,
           "fraction_of_train_step": [stream_row["ms"] / s for s in STEP_MS],
           "synthetic_dags_same_process": {"value": host, "unit": "graphs/s", "sample": "2000 graphs, n = 12"},
           "create_encoder_dataset_12_12_200_20_0.4": {"seconds": t_ds, "graphs": len(ds), "dropped": ds.dropped},
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
