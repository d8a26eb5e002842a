#!/usr/bin/env python3
"""Measurements of tabu search (dags_vae_search_amd/tabu.py, csrc/dvs_tabu.h): asia and sachs, bic, B = 4 096
starts from generate_dags (row 0 the empty graph).
  1. structure-steps/s of tabu_search(tabu=10) and, on the same starts in the same process and alternating with it, of
     hill_climb — the comparison base; wall time per step launch of both;
  2. the per-launch split into toggle pass and step kernel from the library's per-kernel HIP-event timing (runs of their own);
  3. what tabu buys: the share of starts whose tabu best exceeds their greedy final score by more than tau and the mean gain
     over all starts (tau = (n / 2) * 4e-12 * |greedy score|: the score's magnitude bounds the T_abs of the test corpus' rule
     from below by far less than the gains counted here, which are of the order of 1).
Prints one JSON line and writes it to --out.
    python bench_tabu.py [--batch 4096] [--reps 3] [--out profiles/tabu_bench.json]
(The driver's metric is bench.py; this measures the structure-space baselines.)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
MIN_DELTA = 2.0 ** -26
MAX_STEPS = 200
TABU = 10


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def profiled(lib, dl, fn):
    lib.dvs_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    prof = dl.profile_collect(lib)
    lib.dvs_profile_enable(0)
    return prof


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tabu_bench.json"))
    args = ap.parse_args()
    from dags_vae_search_amd import BNLearnWrapper, generate_dags, hill_climb, tabu_search
    from dags_vae_search_amd import _lib as dl
    from tests.helpers import load_npz
    lib = dl.load()
    res = {"bench": "tabu", "device": torch.cuda.get_device_name(0), "batch": args.batch, "score": "bic", "tabu": TABU,
           "min_delta": MIN_DELTA, "max_steps": MAX_STEPS, "reps": args.reps, "workloads": {}}
    for name, n, edges in (("asia", 8, 9), ("sachs", 11, 14)):
        ev = BNLearnWrapper(name, "bic", data=load_npz(f"bn_{name}_data.npz")["data"])
        batch, attempts = generate_dags(n, n, edges, args.batch, seed=7)
        starts = ev.compact_parent_masks(batch)
        starts[0] = 0
        starts[attempts <= 0] = 0
        tabu = lambda: tabu_search(ev, starts, max_steps=MAX_STEPS, tabu=TABU, min_delta=MIN_DELTA)
        greedy = lambda: hill_climb(ev, starts, max_steps=MAX_STEPS, min_delta=MIN_DELTA)
        rt, rg = tabu(), greedy()                                       # warm-up of both
        assert bool(rt.converged.all()) and bool(rg.converged.all()), name
        tt, tg = [], []
        for _ in range(args.reps):                                      # alternating
            tt.append(wall_ms(tabu)[0])
            tg.append(wall_ms(greedy)[0])
        pt, pg = profiled(lib, dl, tabu), profiled(lib, dl, greedy)
        st, sg = int(rt.steps.sum()), int(rg.steps.sum())
        tms, gms = float(np.median(tt)), float(np.median(tg))
        lt, lg = pt["k_tabu_step"][0], pg["k_hc_step"][0]
        gain = (rt.scores - rg.scores)
        tau = 0.5 * n * 4e-12 * rg.scores.abs()
        us = lambda prof, k: 1e3 * prof[k][1] / prof[k][0]
        res["workloads"][name] = {
            "n": n,
            "tabu": {"ms": tms, "steps_total": st, "steps_max": int(rt.steps.max()), "step_launches": lt,
                     "structure_steps_per_s": st / (tms * 1e-3), "wall_us_per_launch": 1e3 * tms / lt,
                     "per_launch_us": {"toggle_pass": us(pt, "k_bn_toggle"), "step_kernel": us(pt, "k_tabu_step")}},
            "hill_climb": {"ms": gms, "steps_total": sg, "steps_max": int(rg.steps.max()), "step_launches": lg,
                           "structure_steps_per_s": sg / (gms * 1e-3), "wall_us_per_launch": 1e3 * gms / lg,
                           "per_launch_us": {"toggle_pass": us(pg, "k_bn_toggle"), "step_kernel": us(pg, "k_hc_step")}},
            "wall_per_launch_tabu_over_hill_climb": (tms / lt) / (gms / lg),
            "step_kernel_tabu_over_hill_climb": us(pt, "k_tabu_step") / us(pg, "k_hc_step"),
            "ring_bytes_per_structure": TABU * n * 8,
            "share_of_starts_tabu_beats_greedy": float((gain > tau).double().mean()),
            "share_of_starts_tabu_below_greedy": float((gain < -tau).double().mean()),
            "mean_gain": float(gain.mean()), "max_gain": float(gain.max())}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
