#!/usr/bin/env python3
"""Reconstruction-judging measurements (dags_vae_search_amd/recon.py, csrc/dvs_match.h):
  1. dvs_match_decoded alone (HIP events, median of reps after warm-up), pairs/s, next to dvs_decode of the same rows, at
     n = 12 card = 1 (the shipped synthetic checkpoint 78, synthetic_dags targets, R = 100) and n = 37 card = 37 (random
     weights);
  2. evaluate_reconstruction per batch of 32 graphs x 100 decodes (n = 12 card = 1) against the host-judged model_test of the
     same shape (a 32 x 10 sample, scaled x 10: the CPU denominator).
    python bench_recon.py [--reps 20]
Prints one JSON line.  (The driver's metric is bench.py; this is the measurement of the evaluation path.)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
DEV = "cuda:0"


def _model(n, card, ckpt=None):
    from dags_vae_search_amd import PaceVaeV3
    torch.manual_seed(0)
    m = PaceVaeV3(n, card, 32, 8, 3, 64, 32, 32, 0.15)
    if ckpt:
        from tests.helpers import load_npz
        ck = load_npz(ckpt)
        m.load_state_dict({k: torch.from_numpy(ck[k]).float() for k in ck.files})
    return m.to(DEV).eval()


def _event_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def kernel_leg(n, card, ckpt, R, reps, B=32):
    from dags_vae_search_amd.recon import match_decoded, topological_targets
    from dags_vae_search_amd.synthetic import synthetic_dags
    model = _model(n, card, ckpt)
    graphs = synthetic_dags(n, card, B, seed=5)
    mu, _ = model.encode(graphs)
    z = mu.repeat_interleave(R, dim=0)
    model.seed(1)
    states = model.decode_states(z)
    targets = topological_targets(graphs, n)
    flags = match_decoded(targets, states, R, card)
    decode_ms = _event_ms(lambda: model.decode_states(z), max(3, reps // 4))
    match_ms = _event_ms(lambda: match_decoded(targets, states, R, card), reps)
    f = flags.to(torch.int64)
    rows = B * R
    return {"rows": rows, "match_ms": round(match_ms, 4), "match_pairs_per_s": round(rows / (match_ms * 1e-3)),
            "decode_ms": round(decode_ms, 3), "match_over_decode": round(match_ms / decode_ms, 4),
            "valid": int((f & 1).sum()), "structure": int(((f >> 1) & 1).sum()), "labelled": int(((f >> 2) & 1).sum()),
            "undecided": int(((f >> 3) & 1).sum())}


def eval_leg(reps):
    from dags_vae_search_amd import LabeledDag, evaluate_reconstruction, model_test
    from dags_vae_search_amd.synthetic import synthetic_dags
    model = _model(12, 1, "n12c1_ckpt78.npz")
    graphs = synthetic_dags(12, 1, 32, seed=9)
    tk = LabeledDag(12, 1)
    try:
        import networkx  # noqa: F401     the host judge of model_test (graph_equals with repeated labels)
        judge = "networkx"
    except ImportError:
        from tests import iso_ref
        tk.graph_equals = iso_ref.graph_equals
        judge = "tests/iso_ref.py"
    out = None
    times = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = evaluate_reconstruction(model, graphs, tk, batch_size=32, encode_times=10, decode_times=10, shuffle=False, seed=2)
        torch.cuda.synchronize()
        if i:
            times.append((time.perf_counter() - t0) * 1e3)
    dev_ms = float(np.median(times))
    t0 = time.perf_counter()
    host = model_test(model, graphs, tk, batch_size=32, encode_times=1, decode_times=10, shuffle=False, seed=2)
    host_ms = (time.perf_counter() - t0) * 1e3 * 10
    return {"evaluate_reconstruction_ms_per_batch": round(dev_ms, 2), "cpu_model_test_ms_per_batch": round(host_ms, 1),
            "cpu_model_test_sample": "32 graphs x 10 decodes, scaled x 10", "cpu_judge": judge,
            "speedup": round(host_ms / dev_ms, 1), "device_rates": {k: out[k] for k in ("valid_ratio", "recon_accuracy",
                                                                                         "structure_accuracy", "undecided")},
            "host_rates": {k: host[k] for k in ("valid_ratio", "recon_accuracy")}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    res = {"bench": "recon", "device": torch.cuda.get_device_name(0),
           "match_n12_c1_R100": kernel_leg(12, 1, "n12c1_ckpt78.npz", 100, args.reps),
           "match_n37_c37_R100": kernel_leg(37, 37, None, 100, args.reps),
           "evaluate_n12_c1": eval_leg(max(1, args.reps // 10))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
