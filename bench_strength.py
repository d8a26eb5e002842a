"""Model averaging (dvs_bn_scores_rows / dvs_bn_toggle_scores_rows, dvs_bootstrap_rows, dvs_arc_strength, dvs_averaged_network,
DESIGN.md §21): bootstrap replicates per second of ``boot_strength`` — all replicates of a call climbing in lock-step on
their own row sets — next to the composition the package allowed before row sets existed (per replicate: gather the rows,
``BNLearnWrapper.from_packed``, one ``hill_climb``), the two alternating in one process; structures per second of
``dvs_arc_strength`` at 10^5 structures; the time of a 64-threshold ``dvs_averaged_network`` sweep; and, reported only, the
SHD between CPDAGs of the averaged network and of one ``hill_climb`` on the full data to the generating network.  On asia
(n = 8) and sachs (n = 11) from tests/golden, and a seeded 37-variable network (``generate_dags``, random tables through
``FittedBN.from_tables``, ``sample``), with bic and bde.  Writes profiles/strength_bench.json.

    python bench_strength.py [--replicates 200] [--repeats 3] [--rows 5000]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import (BNLearnWrapper, FittedBN, arc_strength, averaged_network, boot_strength, bootstrap_rows,
                                 compare_structures, generate_dags, hill_climb, sample)
from dags_vae_search_amd import _lib as dl
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def synthetic_network(n=37, edges=45, card=3, seed=37):
    """(parent masks u64 [n], card [n], tables): one generated DAG in data-set variable indices with Dirichlet(1/2) rows"""
    batch, attempts = generate_dags(n, n, edges, 1, seed=seed)
    assert int(attempts[0]) > 0
    labels, preds = batch.labels.cpu().numpy()[0], batch.preds.cpu().numpy()[0].astype(np.int64).view(np.uint64)
    parents = np.zeros(n, np.uint64)
    for v in range(n):
        for u in sc.mask_bits(preds[v]):
            parents[labels[v]] |= np.uint64(1) << np.uint64(labels[u])
    rng = np.random.default_rng(seed)
    cards = [card] * n
    tables = [rng.dirichlet([0.5] * card, size=card ** len(sc.mask_bits(parents[v]))) for v in range(n)]
    return parents, cards, tables


def configurations(rows):
    for name, steps in (("asia", 40), ("sachs", 80)):
        data = np.load(os.path.join(HERE, "tests", "golden", f"bn_{name}_data.npz"))["data"].astype(np.uint8)
        known = sc.masks_of(8, hc.ASIA_KNOWN)[0] if name == "asia" else None
        yield name, steps, known, lambda metric, data=data, name=name: BNLearnWrapper(name, metric, data=data,
                                                                                       **({"iss": 10.0} if metric == "bde" else {}))
    parents, cards, tables = synthetic_network()
    packed = sample(FittedBN.from_tables(parents, cards, tables), rows, seed=371)
    yield "syn37", 150, parents, lambda metric: BNLearnWrapper.from_packed("syn37", metric, packed, cards,
                                                                           iss=10.0 if metric == "bde" else None)


def per_replicate(ev, name, metric, replicates, seed, **args):
    """the composition without row sets: one gather, one evaluator and one hill_climb call per replicate"""
    rows = bootstrap_rows(replicates, ev.n_samples, ev.n_samples, seed=seed)
    nets = []
    for r in range(replicates):
        one = BNLearnWrapper.from_packed(name, metric, ev.packed[rows[r].long()], ev.card_host, iss=ev.iss)
        nets.append(hill_climb(one, batch=1, **args).parents)
    return arc_strength(torch.cat(nets))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replicates", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--arc-batch", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "strength_bench.json"))
    args = ap.parse_args()
    R = args.replicates
    res = {"device": torch.cuda.get_device_name(0), "replicates": R, "repeats": args.repeats,
           "timing": "host clock around calls that end in a device synchronise; the two compositions alternate in one process",
           "boot_strength": [], "arc_strength": [], "averaged_network": []}
    last = None
    for name, steps, known, make in configurations(args.rows):
        for metric in ("bic", "bde"):
            ev = make(metric)
            hc_args = dict(max_steps=steps)
            batched = lambda: boot_strength(ev, replicates=R, algorithm="hc", algorithm_args=hc_args, seed=1)
            plain = lambda: per_replicate(ev, name, metric, R, 1, **hc_args)
            batched(), per_replicate(ev, name, metric, 4, 1, **hc_args)                  # warm-up
            tb, tp = [], []
            for _ in range(args.repeats):
                t, s = wall(batched)
                tb.append(t)
                t, s_plain = wall(plain)
                tp.append(t)
            row = {"name": name, "n": ev.n_vars, "samples": ev.n_samples, "metric": metric, "max_steps": steps,
                   "exhausted": s.exhausted, "equal_counts": bool(torch.equal(s.any, s_plain.any) and torch.equal(s.dir2, s_plain.dir2)),
                   "boot_strength_s": [round(x, 4) for x in tb], "per_replicate_s": [round(x, 4) for x in tp],
                   "boot_strength_replicates_per_s": round(R / float(np.median(tb)), 1),
                   "per_replicate_replicates_per_s": round(R / float(np.median(tp)), 1)}
            net = averaged_network(s)
            row.update(threshold=net.threshold, placed=net.placed, dropped=net.dropped, ties=net.ties)
            if known is not None:
                target = torch.from_numpy(np.ascontiguousarray(known, np.uint64).view(np.int64).copy()).cuda()
                full = hill_climb(ev, batch=1, **hc_args).parents
                row["shd_averaged_network"] = int(compare_structures(net.parents[None], target).shd[0])
                row["shd_one_hill_climb"] = int(compare_structures(full, target).shd[0])
            res["boot_strength"].append(row)
            print(row, flush=True)
            last = s

    lib = dl.load()
    for n in (8, 37, 48):
        B = args.arc_batch
        bits = (torch.rand(B, n, n, device="cuda") < 2.5 / n) & torch.ones(n, n, dtype=torch.bool, device="cuda").tril(-1)
        P = (bits.to(torch.int64) << torch.arange(n, device="cuda")).sum(-1).contiguous()
        counts = torch.zeros(n, n, 2, dtype=torch.int32, device="cuda")
        run = lambda: dl.check(lib, lib.dvs_arc_strength(B, n, P.data_ptr(), counts.data_ptr(), counts.numel() * 4, None), "dvs_arc_strength")
        run()
        ts = [wall(run)[0] for _ in range(max(args.repeats, 5))]
        row = {"n": n, "batch": B, "ms": round(float(np.median(ts)) * 1e3, 4), "structures_per_s": round(B / float(np.median(ts)))}
        res["arc_strength"].append(row)
        print(row, flush=True)

    sweep = [k / 64.0 for k in range(64)]
    run = lambda: averaged_network(last, sweep)
    run()
    ts = [wall(run)[0] for _ in range(max(args.repeats, 5))]
    row = {"n": int(last.any.shape[0]), "thresholds": 64, "ms": round(float(np.median(ts)) * 1e3, 4)}
    res["averaged_network"].append(row)
    print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
