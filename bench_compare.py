#!/usr/bin/env python3
"""Measurements of structure comparison (dags_vae_search_amd/compare.py, csrc/dvs_cpdag.h): dvs_cpdag and
dvs_pdag_compare on random DAGs of n = 8 (asia-sized) and n = 37, B = 4 096 and 65 536, density 0.2 and 0.5.  Structures per
second and microseconds per launch come from the library's per-kernel HIP-event timing: per shape one warm-up launch, then
--reps profiled runs of --launches launches each, the median over the runs.  dvs_hc_step on the same B and n in the same
process goes beside them as the yardstick — the same kind of kernel, a closure plus an n-loop, one wave per structure — on
an all-zero toggle table: every structure has all its moves priced, none gains, and it converges without moving.
Prints one JSON line and writes it to --out.
    python bench_compare.py [--reps 5] [--launches 20] [--out profiles/compare_bench.json]
(The driver's metric is bench.py; this measures the structure-comparison kernels.)"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
SHAPES = [(n, B, d) for n in (8, 37) for B in (4096, 65536) for d in (0.2, 0.5)]


def random_dags(n, B, density, seed):
    """int64 [B, n] on the device: each edge of a random topological order with probability `density`, the order a random
    permutation of the variable indices"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    order = torch.rand(B, n, device="cuda", generator=g).argsort(1)                       # position -> variable
    rank = torch.empty_like(order).scatter_(1, order, torch.arange(n, device="cuda").expand(B, n))
    edge = (torch.rand(B, n, n, device="cuda", generator=g) < density) & (rank[:, None, :] < rank[:, :, None])   # [b, v, u]
    return (edge.to(torch.int64) << torch.arange(n, device="cuda")).sum(2)


def profiled_us(lib, dl, fn, kernel, launches, reps):
    fn()                                                                                   # warm-up
    torch.cuda.synchronize()
    per = []
    for _ in range(reps):
        lib.dvs_profile_enable(1)
        for _ in range(launches):
            fn()
        torch.cuda.synchronize()
        count, ms = dl.profile_collect(lib)[kernel]
        lib.dvs_profile_enable(0)
        assert count == launches, (kernel, count)
        per.append(1e3 * ms / count)
    return float(np.median(per))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "compare_bench.json"))
    args = ap.parse_args()
    from dags_vae_search_amd import _lib as dl
    lib = dl.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"bench": "compare", "device": torch.cuda.get_device_name(0), "reps": args.reps, "launches": args.launches, "shapes": []}
    for n, B, density in SHAPES:
        parents = random_dags(n, B, density, seed=1000 * n + int(10 * density))
        other = random_dags(n, B, density, seed=7)
        pdag, flags = torch.empty_like(parents), torch.empty(B, dtype=torch.int32, device="cuda")
        counts = torch.empty(B, 5, dtype=torch.int32, device="cuda")
        i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device="cuda")
        L, T = torch.zeros(B, n, dtype=torch.float64, device="cuda"), torch.zeros(B, n, n, dtype=torch.float64, device="cuda")
        work, wl, steps, conv, hflags, active = parents.clone(), i32(2 * B), i32(B), i32(B), i32(B), i32(1)

        def run_cpdag():
            dl.check(lib, lib.dvs_cpdag(B, n, p(parents), p(pdag), pdag.numel() * 8, p(flags), stream), "dvs_cpdag")

        def run_compare():
            dl.check(lib, lib.dvs_pdag_compare(B, n, p(pdag), p(other), B, p(counts), counts.numel() * 4, stream), "dvs_pdag_compare")

        def run_hc_step():
            conv.zero_()                                                                   # every structure is priced again
            dl.check(lib, lib.dvs_hc_step(B, n, p(work), p(L), p(T), T.numel() * 8, 0, 0.0, None, 1, p(wl), p(steps), p(conv),
                                          p(hflags), None, 0, p(active), stream), "dvs_hc_step")

        us = {k: profiled_us(lib, dl, fn, k, args.launches, args.reps)
              for k, fn in (("k_cpdag", run_cpdag), ("k_pdag_compare", run_compare), ("k_hc_step", run_hc_step))}
        assert not bool(flags.any()) and not bool(hflags.any()) and bool(conv.all()) and not bool(steps.any())
        undirected = (pdag & torch.stack([((pdag >> v) & 1) << torch.arange(n, device="cuda") for v in range(n)], 1).sum(2)) != 0
        res["shapes"].append({
            "n": n, "batch": B, "density": density, "edges_mean": float(sum(((parents >> u) & 1).sum() for u in range(n))) / B,
            "share_of_structures_with_an_undirected_edge": float(undirected.any(1).double().mean()),
            "per_launch_us": us,
            "structures_per_s": {k: B / (v * 1e-6) for k, v in us.items()},
            "cpdag_over_hc_step": us["k_cpdag"] / us["k_hc_step"],
            "pdag_compare_over_hc_step": us["k_pdag_compare"] / us["k_hc_step"]})
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
