#!/usr/bin/env python3
"""Measurements of the greedy hill climb (dags_vae_search_amd/hillclimb.py, csrc/dvs_hillclimb.h): asia and
sachs, bic, B = 4 096 starts (one empty graph, the rest from generate_dags), run to convergence.
  1. the fused path (hill_climb: dvs_hc_step + the incremental dvs_bn_toggle_scores pass, 2 n families per structure and
     step): wall time, structure-steps/s, steps to convergence, and the per-step split into toggle pass and step kernel from
     the library's per-kernel HIP-event timing (a run of its own);
  2. in the same process, alternating with it, what the scorer alone can do: every step re-scores all n^2 toggled families
     of every structure in one score_masks(local=True) call and picks the move in torch with the same rules.
Both must end on the same masks (asserted).  Prints one JSON line and writes it to --out.
    python bench_hillclimb.py [--batch 4096] [--reps 3] [--out profiles/hillclimb_bench.json]
(The driver's metric is bench.py; this measures the structure-space baseline.)"""
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


def closure(P, n):
    reach = P.clone()
    for k in range(n):
        reach = torch.where(((reach >> k) & 1).bool(), reach | reach[:, k:k + 1], reach)
    return reach


def composed_step(ev, P, n):
    """One greedy step from score_masks alone: (new P, moved [B] bool).  Structure (b, u) of the scored batch is P[b] with
    bit u flipped in every row but u, so its local score of v is T[b][v][u]."""
    B = P.shape[0]
    dev = P.device
    idx = torch.arange(n, device=dev)
    bit = (torch.ones(n, dtype=torch.int64, device=dev) << idx)
    flip = torch.where(idx[:, None] == idx[None, :], torch.zeros_like(bit)[None, :].expand(n, n), bit[:, None].expand(n, n))
    Q = (P[:, None, :] ^ flip[None, :, :]).reshape(B * n, n)            # [(b, u), v]
    L = ev.score_masks(P, local=True)[1]
    T = ev.score_masks(Q, local=True)[1].reshape(B, n, n).transpose(1, 2)   # [b, v, u]
    reach = closure(P, n)
    has = ((P[:, :, None] >> idx[None, None, :]) & 1).bool()            # [b, v, u]: u in P[v]
    anc_vu = ((reach[:, None, :] >> idx[None, :, None]) & 1).bool()     # [b, v, u]: v in reach[u]
    offdiag = (idx[:, None] != idx[None, :])[None]
    d1 = T - L[:, :, None]
    d_add = torch.where(~has & ~anc_vu & offdiag, d1, torch.full_like(d1, -np.inf))
    d_del = torch.where(has & offdiag, d1, torch.full_like(d1, -np.inf))
    child = torch.zeros(B, n, dtype=torch.int64, device=dev)           # child[b, u]: bit w <=> u in P[w]
    for w in range(n):
        child |= ((P[:, w:w + 1] >> idx[None, :]) & 1) << w
    blocked = ((child[:, None, :] & ~bit[None, :, None]) & (reach[:, :, None] | bit[None, :, None])) != 0
    d_rev = torch.where(has & ~blocked & offdiag, d1 + (T.transpose(1, 2) - L[:, None, :]), torch.full_like(d1, -np.inf))
    d = torch.stack([d_add, d_del, d_rev], 1).reshape(B, 3 * n * n)
    d = torch.where(torch.isnan(d), torch.full_like(d, -np.inf), d)
    best = d.max(1).values
    codes = torch.arange(3 * n * n, device=dev)[None, :].expand(B, -1)
    code = torch.where(d == best[:, None], codes, torch.full_like(codes, 1 << 30)).min(1).values
    moved = best > MIN_DELTA
    op, v, u = code // (n * n), (code % (n * n)) // n, code % n
    rows = torch.arange(B, device=dev)
    newP = P.clone()
    m = moved
    newP[rows[m], v[m]] = P[rows[m], v[m]] ^ (1 << u[m])
    r = m & (op == 2)
    newP[rows[r], u[r]] = P[rows[r], u[r]] | (1 << v[r])
    return newP, moved


def composed_climb(ev, starts, n):
    P = starts.clone()
    steps = torch.zeros(P.shape[0], dtype=torch.int64, device=P.device)
    for t in range(MAX_STEPS):
        P, moved = composed_step(ev, P, n)
        steps += moved
        if (t + 1) % 8 == 0 and not bool(moved.any()):
            break
    return P, steps


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "hillclimb_bench.json"))
    args = ap.parse_args()
    from dags_vae_search_amd import BNLearnWrapper, generate_dags, hill_climb
    from dags_vae_search_amd import _lib as dl
    from tests.helpers import load_npz
    res = {"bench": "hillclimb", "device": torch.cuda.get_device_name(0), "batch": args.batch, "score": "bic",
           "min_delta": MIN_DELTA, "reps": args.reps, "workloads": {}}
    for name, n, edges in (("asia", 8, 9), ("sachs", 11, 14)):
        ev = BNLearnWrapper(name, "bic", data=load_npz(f"bn_{name}_data.npz")["data"])
        batch, attempts = generate_dags(n, n, edges, args.batch, seed=7)
        starts = ev.compact_parent_masks(batch)
        starts[0] = 0
        starts[attempts <= 0] = 0
        fused = lambda: hill_climb(ev, starts, max_steps=MAX_STEPS, min_delta=MIN_DELTA)
        comp = lambda: composed_climb(ev, starts, n)
        r = fused()
        Pc, steps_c = comp()                                            # warm-up of both, and the equality check
        assert torch.equal(r.parents, Pc) and torch.equal(r.steps.long(), steps_c), name
        assert bool(r.converged.all())
        tf, tc = [], []
        for _ in range(args.reps):                                      # alternating
            tf.append(wall_ms(fused)[0])
            tc.append(wall_ms(comp)[0])
        lib = dl.load()
        lib.dvs_profile_enable(1)
        fused()
        torch.cuda.synchronize()
        prof = dl.profile_collect(lib)
        lib.dvs_profile_enable(0)
        total_steps = int(r.steps.sum())
        launches = prof["k_hc_step"][0]
        fms, cms = float(np.median(tf)), float(np.median(tc))
        res["workloads"][name] = {
            "n": n, "steps_total": total_steps, "steps_max": int(r.steps.max()), "steps_mean": total_steps / args.batch,
            "step_launches": launches, "fused_ms": fms, "composed_ms": cms, "composed_over_fused": cms / fms,
            "fused_structure_steps_per_s": total_steps / (fms * 1e-3),
            "families_per_structure_step": {"fused": 2 * n, "composed": n * n + n},
            "per_launch_us": {"toggle_pass": 1e3 * prof["k_bn_toggle"][1] / prof["k_bn_toggle"][0],
                              "step_kernel": 1e3 * prof["k_hc_step"][1] / launches},
            "faster_than_composition": fms < cms}
        assert fms < cms, (name, fms, cms)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
