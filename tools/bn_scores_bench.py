#!/usr/bin/env python3
"""Throughput of the batched BN scorer per score type, and a same-call A/B of dvs_bic_scores between builds.
    python tools/bn_scores_bench.py --out profiles/bn_scores_throughput.json [--ab parent]
Method: that of tests/test_gpu_bic.py (which wrote profiles/r03_bic_throughput.log) — BNLearnWrapper.score_masks on 4 096
synthetic DAGs of asia / sachs, a host clock around calls that end in a device synchronise — with a warm-up of 20 calls and
`rounds` timed windows of `calls` calls each instead of one window of 5.  `--ab NAME` also measures dvs_bic_scores of
dags_vae_search_amd/libdvs_NAME.so (tools/build_variant.sh NAME <rev>): one child process per build and repeat, the two
builds alternating, so that the spread of either is seen next to the difference between them."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("loglik", "aic", "bic", "bde", "bds", "k2", "bdj")
BATCH = 4096


def child(lib_name, types, calls, rounds):
    import time
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from dags_vae_search_amd import _lib as dl
    dl.LIB_NAME = f"libdvs_{lib_name}.so"
    if lib_name != "hip":                         # an older build may lack newer exports: bind the one entry point timed
        import ctypes
        raw = ctypes.CDLL(dl.lib_path())
        raw.dvs_bic_scores.restype = ctypes.c_int
        raw.dvs_bic_scores.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_void_p] * 7
        raw.dvs_last_error.restype = ctypes.c_char_p
        dl._lib = raw
    from dags_vae_search_amd import BNLearnWrapper
    from dags_vae_search_amd.synthetic import synthetic_dags
    out = {}
    for name, n in (("asia", 8), ("sachs", 11)):
        data = np.load(os.path.join(REPO, "tests", "golden", f"bn_{name}_data.npz"))["data"]
        graphs = synthetic_dags(n, n, BATCH, seed=9)
        masks = None
        for typ in types:
            ev = BNLearnWrapper(name, typ, data=data)
            if masks is None:
                masks = torch.from_numpy(ev._parent_masks(graphs, "type").view(np.int64)).cuda()
            for _ in range(20):
                ev.score_masks(masks)
            torch.cuda.synchronize()
            ms = []
            for _ in range(rounds):
                t0 = time.perf_counter()
                for _ in range(calls):
                    ev.score_masks(masks)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) / calls * 1e3)
            out[f"{name}_{typ}"] = ms
            if typ == "bic":
                import hashlib
                out[f"{name}_bic_sha256"] = hashlib.sha256(ev.score_masks(masks).cpu().numpy().tobytes()).hexdigest()
    print("RESULT " + json.dumps(out), flush=True)


def run_child(lib_name, types, calls, rounds):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", lib_name, "--types", ",".join(types), "--calls", str(calls),
           "--rounds", str(rounds)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    if p.returncode != 0 or not lines:
        raise SystemExit(f"child {lib_name} failed ({p.returncode}): {p.stderr[-2000:]}")
    return json.loads(lines[-1][7:])


def stats(ms):
    mean = sum(ms) / len(ms)
    return {"mean_ms": round(mean, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "structures_per_s": round(BATCH / (mean * 1e-3))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bn_scores_throughput.json"))
    ap.add_argument("--ab", default=None, help="name of a second build (libdvs_<name>.so) to compare dvs_bic_scores against")
    ap.add_argument("--repeats", type=int, default=3, help="child processes per build in the A/B")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--child", default=None)
    ap.add_argument("--types", default=",".join(TYPES))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.types.split(","), args.calls, args.rounds)
    res = {"bench": "bn_scores", "batch": BATCH, "calls_per_window": args.calls, "windows": args.rounds, "warmup_calls": 20,
           "timing": "host clock around BNLearnWrapper.score_masks calls that end in a device synchronise; ms per call"}
    first = run_child("hip", TYPES, args.calls, args.rounds)
    res["throughput"] = {k: stats(v) for k, v in first.items() if isinstance(v, list)}
    if args.ab:
        runs = {"hip": [], args.ab: []}
        for _ in range(args.repeats):
            for name in ("hip", args.ab):
                runs[name].append(run_child(name, ["bic"], args.calls, args.rounds))
        ab = {}
        for key in ("asia_bic", "sachs_bic"):
            ab[key] = {}
            for name, label in (("hip", "this_build"), (args.ab, "parent_build")):
                per_process = [sum(r[key]) / len(r[key]) for r in runs[name]]
                windows = [x for r in runs[name] for x in r[key]]
                ab[key][label] = dict(stats(windows), process_means_ms=[round(x, 4) for x in per_process],
                                      spread_of_process_means_ms=round(max(per_process) - min(per_process), 4))
            new, old = ab[key]["this_build"], ab[key]["parent_build"]
            ab[key]["this_minus_parent_ms"] = round(new["mean_ms"] - old["mean_ms"], 4)
            ab[key]["within_parent_spread"] = new["mean_ms"] - old["mean_ms"] <= old["max_ms"] - old["min_ms"]
            digests = {r[key + "_sha256"] for name in runs for r in runs[name]}
            ab[key]["equal_bytes_across_builds_and_runs"] = len(digests) == 1
        res["dvs_bic_scores_ab"] = ab
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
