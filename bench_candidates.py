#!/usr/bin/env python3
"""Measurements of the search's candidate stage (dags_vae_search_amd/search.py, csrc/dvs_structs.h):
  1. wall time of "decoded states -> gathered new rows" — everything between decode_states returning and keys[new] /
     compact[new] being ready — on the host path (states.cpu() -> graphs_from_states -> new_structures -> encode_graphs ->
     .to(device)) and on the device path (decoded_structures -> StructureSet filter -> gather), in the same process on the
     same states, alternating, median of --reps repetitions after warm-up; for 4 096 / 16 384 / 65 536 draws of the asia
     checkpoint and 4 096 draws at n = 37 (random weights), against an empty set and a set of 100 000 structures;
  2. where the device time goes (HIP events per step; the two kernels alone from the library's per-kernel timing) next to
     dvs_decode of the same rows;
  3. one search iteration at 4 096 candidates x 4 tries with candidates="device" (timings_ms), beside 64 x 4 on both paths.
    python bench_candidates.py [--reps 20] [--out profiles/search_candidates_bench.json]
Prints one JSON line and writes it to --out.  (The driver's metric is bench.py; this measures the search's host stage.)"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)
DEV = "cuda:0"
SET_SIZE = 100_000


def _model(n, ckpt=None):
    from dags_vae_search_amd import PaceVaeV3
    torch.manual_seed(0)
    m = PaceVaeV3(n, n, 32, 8, 3, 64, 32, 32, 0.15)
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


def random_structures(n, count, seed):
    """`count` distinct random DAGs on n vertices with permutation labels (sparse: about 1.5 parents per vertex)."""
    from dags_vae_search_amd import LabeledGraph
    from dags_vae_search_amd.search import structure_key
    rng = np.random.default_rng(seed)
    p = min(0.5, 3.0 / max(n - 1, 1))
    out, keys = [], set()
    while len(out) < count:
        labels = [int(x) for x in rng.permutation(n)]
        vs, us = np.nonzero(np.tril(rng.random((n, n)) < p, -1))
        g = LabeledGraph(labels, list(zip(us.tolist(), vs.tolist())))
        k = structure_key(g)
        if k not in keys:
            keys.add(k)
            out.append(g)
    return out, keys


def _host_stage(states, n, dag, seen):
    from dags_vae_search_amd.pace import graphs_from_states
    from dags_vae_search_amd.records import encode_graphs
    from dags_vae_search_amd.search import new_structures
    draws = graphs_from_states(states.cpu().numpy(), n + 3)
    new, n_valid = new_structures(draws, dag, seen)
    batch = encode_graphs(new, n).to(DEV) if new else None
    torch.cuda.synchronize()
    return len(new), n_valid, batch


def _device_stage(model, states, sset):
    from dags_vae_search_amd.search import STRUCT_VALID, decoded_structures
    flags, compact, keys, hashes = decoded_structures(model, states)
    _, idx, (n_valid,) = sset._filter_rows(keys, hashes, flags, False, also=(flags & STRUCT_VALID).sum())
    rows, new_keys = compact[idx], keys[idx]
    torch.cuda.synchronize()
    return int(idx.numel()), n_valid, rows, new_keys


def stage_leg(model, n, z, sets, reps, states=None):
    """``states``: hand-made rows instead of decode_states(z) (then there is no decode time to put beside)."""
    from dags_vae_search_amd import LabeledDag, StructureSet
    from dags_vae_search_amd import _lib as dl
    from dags_vae_search_amd.search import decoded_structures
    dag = LabeledDag(n, n)
    if states is None:
        model.seed(1)
        states = model.decode_states(z)
        out = {"rows": states.shape[0], "decode_ms": round(_event_ms(lambda: model.decode_states(z), max(3, reps // 4)), 3)}
    else:
        out = {"rows": states.shape[0], "decode_ms": None}
    rows = states.shape[0]
    for label, (graphs, seen) in sets.items():
        sset = StructureSet(n, DEV)
        sset.add_graphs(graphs)
        assert len(sset) == len(seen)
        host_t, dev_t = [], []
        for i in range(reps + 2):                    # two warm-up rounds; host and device alternate
            mine = set(seen)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            h_new, h_valid, h_batch = _host_stage(states, n, dag, mine)
            t1 = time.perf_counter()
            d_new, d_valid, d_rows, _ = _device_stage(model, states, sset)
            t2 = time.perf_counter()
            assert (h_new, h_valid) == (d_new, d_valid), ((h_new, h_valid), (d_new, d_valid))
            if h_new:
                assert torch.equal(h_batch.labels, d_rows.labels) and torch.equal(h_batch.preds, d_rows.preds)
            if i >= 2:
                host_t.append((t1 - t0) * 1e3)
                dev_t.append((t2 - t1) * 1e3)
        host_ms, dev_ms = float(np.median(host_t)), float(np.median(dev_t))
        # the device stage on its own: without the host stage's garbage (graph objects, key tuples) between the calls
        gc.collect()
        alone_t = []
        for i in range(reps + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _device_stage(model, states, sset)
            if i >= 2:
                alone_t.append((time.perf_counter() - t0) * 1e3)
        # where the device time goes: HIP events per step, then the two kernels alone
        flags, compact, keys, hashes = decoded_structures(model, states)
        mask = sset._verdicts(keys, hashes, flags) == 1
        n_new = int(mask.sum())
        steps = {
            "structures": _event_ms(lambda: decoded_structures(model, states), reps),
            "sort_hashes": _event_ms(lambda: torch.sort(hashes, stable=True), reps),
            "sort_and_filter": _event_ms(lambda: sset._verdicts(keys, hashes, flags), reps),
            "index_of_new": _event_ms(lambda: torch.sort(mask.to(torch.uint8), descending=True, stable=True).indices[:n_new], reps),
        }
        idx = torch.sort(mask.to(torch.uint8), descending=True, stable=True).indices[:n_new]
        steps["gather"] = _event_ms(lambda: (compact[idx], keys[idx]), reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            mask.sum().reshape(1).tolist()
        steps["count_readback_wall"] = (time.perf_counter() - t0) * 1e3 / reps
        lib = dl.load()
        lib.dvs_profile_enable(1)
        for _ in range(reps):
            decoded_structures(model, states)
            sset._verdicts(keys, hashes, flags)
        torch.cuda.synchronize()
        prof = dl.profile_collect(lib)
        lib.dvs_profile_enable(0)
        kernels = {k: round(ms / max(c, 1), 4) for k, (c, ms) in prof.items() if k in ("k_decoded_structures", "k_structset_filter")}
        out[label] = {"set_size": len(seen), "valid": d_valid, "new": d_new, "host_ms": round(host_ms, 3),
                      "device_ms": round(dev_ms, 3), "host_over_device": round(host_ms / dev_ms, 1),
                      "device_alone_ms": round(float(np.median(alone_t)), 3),
                      "host_spread_ms": [round(min(host_t), 3), round(max(host_t), 3)],
                      "device_spread_ms": [round(min(dev_t), 3), round(max(dev_t), 3)],
                      "host_rows_per_s": round(rows / (host_ms * 1e-3)), "device_rows_per_s": round(rows / (dev_ms * 1e-3)),
                      "device_steps_ms": {k: round(v, 4) for k, v in steps.items()}, "kernel_ms": kernels}
    return out


def search_leg(metric="bic"):
    from dags_vae_search_amd import BNLearnWrapper, LabeledGraph, latent_bo_search
    from dags_vae_search_amd.predictor import GPRegressionModel
    from tests.helpers import graphs_from, load_npz
    fix = load_npz("asia_predictor.npz")
    graphs = [LabeledGraph(list(l), list(e)) for l, e in graphs_from(load_npz("asia_predictor_graphs.npz"), 8)][:256]
    ev = BNLearnWrapper("asia", metric, data=load_npz("bn_asia_data.npz")["data"])
    out = {}
    for name, batch, cand in (("64x4_host", 64, "host"), ("64x4_device", 64, "device"), ("4096x4_device", 4096, "device")):
        vae = _model(8, "asia_ckpt110.npz")
        gp = GPRegressionModel(torch.from_numpy(fix["x"][:256]), torch.from_numpy(fix["y"][:256]))
        gp.load_state_dict({"likelihood.noise_covar.raw_noise": torch.from_numpy(fix["raw_noise"]),
                            "mean_module.raw_constant": torch.from_numpy(fix["raw_constant"]),
                            "base_covar_module.raw_outputscale": torch.from_numpy(fix["raw_outputscale"]),
                            "base_covar_module.base_kernel.raw_lengthscale": torch.from_numpy(fix["raw_lengthscale"]),
                            "covar_module.inducing_points": torch.from_numpy(fix["inducing_points"])})
        res = latent_bo_search(vae, gp, ev, graphs, iterations=3, batch_size=batch, n_starts=max(256, batch), steps=30, lr=0.02,
                               decode_tries=4, xi=0.0, variance="sor", seed=1234, candidates=cand)
        h = res.history[-1]                           # the last iteration: every shape is warm
        out[name] = {"iteration": h.iteration, "draws": h.n_candidates, "valid": h.n_valid, "new": h.n_new,
                     "ms": round(h.seconds * 1e3, 2), "timings_ms": {k: round(v, 3) for k, v in h.timings_ms.items()},
                     "new_all_iterations": sum(s.n_new for s in res.history)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_candidates_bench.json"))
    ap.add_argument("--set-size", type=int, default=SET_SIZE)
    ap.add_argument("--metric", default="bic", help="the search leg's score type (BNLearnWrapper metric_name)")
    args = ap.parse_args()
    from tests.helpers import load_npz
    res = {"bench": "search_candidates", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "timing": "wall clock around work that ends in a device synchronise; median; host and device alternate"}
    x = torch.from_numpy(load_npz("asia_predictor.npz")["x"]).float()
    asia = _model(8, "asia_ckpt110.npz")
    big8 = random_structures(8, args.set_size, 1)
    sets8 = {"empty_set": ([], set()), "set_100k": big8}
    g = torch.Generator().manual_seed(2)
    for rows in (4096, 16384, 65536):
        # draws as a search makes them: 4 tries per latent; a quarter of the latents are posterior means of known graphs
        # (mostly valid draws, many repeats), the rest are those means with N(0, 0.3^2) noise (mostly invalid draws)
        noise = 0.3 * (torch.arange(rows // 4) % 4 != 0).float()[:, None]
        z = x[torch.randint(0, len(x), (rows // 4,), generator=g)] + noise * torch.randn(rows // 4, 32, generator=g)
        res[f"asia_{rows}"] = stage_leg(asia, 8, z.repeat_interleave(4, 0).to(DEV), sets8, args.reps)
    sets37 = {"empty_set": ([], set()), "set_100k": random_structures(37, args.set_size, 3)}
    z = torch.randn(4096, 32, generator=g).to(DEV)
    m37 = _model(37)
    res["n37_4096"] = stage_leg(m37, 37, z, sets37, args.reps)
    # random weights give next to no valid rows at n = 37, so the filter idles there; the same shape with hand-made valid
    # rows: 1 024 structures of the set and 1 024 others, 4 096 draws with repeats
    from tests.recon_corpus import states_of
    pool = sets37["set_100k"][0][:1024] + random_structures(37, 1024, 4)[0]
    pick = np.random.default_rng(5).integers(0, len(pool), 4096)
    made = torch.from_numpy(states_of([pool[i] for i in pick], 37)).to(DEV)
    res["n37_4096_handmade_valid"] = stage_leg(m37, 37, None, sets37, args.reps, states=made)
    res["search_iteration_asia"] = search_leg(args.metric)
    res["metric"] = args.metric
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
