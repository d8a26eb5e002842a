"""BN parameters (dvs_bn_fit, dvs_bn_sample, dvs_bn_loglik): the time of fitting a batch of structures, sampled
rows per second and held-out rows per second at 10^6 rows, on asia (n = 8), sachs (n = 11) and a seeded 37-variable / 4-level
data set, each by wall time and by the library's HIP-event kernel time, next to the numpy restatement of
tests/params_corpus.py on the CPU (exact rationals and math.fsum: a reference, not a tuned CPU implementation).  Writes
profiles/params_bench.json.

    python bench_params.py [--repeats 5] [--rows 1000000] [--batch 256]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, _lib as dl
from dags_vae_search_amd import bn_fit, log_likelihood, sample
from tests import hillclimb_corpus as hc
from tests import params_corpus as pm
from tests import pc_corpus as pc
from tests import scoring_corpus as sc

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
    return {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in prof.items() if k.startswith("k_bn_")}


def random_dag(rng, n, max_parents=3):
    order = rng.permutation(n)
    return {int(order[k]): sorted(int(x) for x in rng.choice(order[:k], size=min(int(rng.integers(0, max_parents + 1)), k), replace=False))
            for k in range(1, n)}


def datasets():
    yield "asia", pc.e2e_data("asia", 5000)[0], hc.ASIA_KNOWN
    yield "sachs", pc.e2e_data("sachs", 5000)[0], None
    yield "syn37", sc.synthetic_dataset(37, 5000, [4] * 37, seed=937)[0], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--cpu-rows", type=int, default=20000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "params_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": args.rows, "fit": [], "sample": [], "loglik": []}

    for name, data, known in datasets():
        ev = BNLearnWrapper(name, "bic", data=data)
        card = (data.max(0) + 1).astype(np.uint8)
        n = ev.n_vars
        rng = np.random.default_rng(1000 + n)
        dags = [known if known is not None else random_dag(rng, n)] + [random_dag(rng, n) for _ in range(args.batch - 1)]
        masks = sc.masks_of(n, *dags)
        dev_masks = torch.from_numpy(masks.view(np.int64)).cuda()
        base = {"name": name, "n": n, "samples": ev.n_samples}

        for method in ("mle", "bayes"):
            run = lambda: bn_fit(ev, dev_masks, method=method)
            t0 = time.perf_counter()
            for v in range(n):
                pm.fit_reference(pm.family_counts(data, card, masks[0, v], v), 0 if method == "mle" else 1, 1.0, 0)
            cpu_s = time.perf_counter() - t0
            ms = timed(run, args.repeats)
            row = dict(base, method=method, batch=args.batch, cells=int(pm.offsets_of(card, masks)[-1]), ms=ms,
                       structures_per_s=args.batch / (ms * 1e-3), cpu_structures_per_s=1.0 / cpu_s, kernels=kernels_ms(run))
            res["fit"].append(row)
            print(row, flush=True)

        fitted = bn_fit(ev, dev_masks[:1], method="bayes")
        net = pm.Network(name, card, masks[0], [fitted.table(v).cpu().numpy() for v in range(n)])
        run = lambda: sample(fitted, args.rows, seed=1)
        t0 = time.perf_counter()
        pm.sample_ref(net, args.cpu_rows, 1)
        cpu_s = time.perf_counter() - t0
        ms = timed(run, args.repeats)
        kern = kernels_ms(run)
        row = dict(base, rows=args.rows, cells=int(fitted.cpt.numel()), ms=ms, rows_per_s=args.rows / (ms * 1e-3),
                   kernel_rows_per_s=args.rows / (sum(k["ms"] for k in kern.values()) * 1e-3), cpu_rows=args.cpu_rows,
                   cpu_rows_per_s=args.cpu_rows / cpu_s, kernels=kern)
        res["sample"].append(row)
        print(row, flush=True)

        held_out = sample(fitted, args.rows, seed=2)
        for batch in (1, 8):
            many = bn_fit(ev, dev_masks[:batch], method="bayes")
            run = lambda: log_likelihood(many, held_out)
            ms = timed(run, args.repeats)
            kern = kernels_ms(run)
            row = dict(base, rows=args.rows, batch=batch, ms=ms, rows_per_s=args.rows * batch / (ms * 1e-3),
                       kernel_rows_per_s=args.rows * batch / (sum(k["ms"] for k in kern.values()) * 1e-3), kernels=kern)
            if batch == 1:
                cpu_rows = min(args.cpu_rows, 2000)
                levels = pm.unpack(held_out[:cpu_rows].cpu().numpy().view(np.uint64), n)
                t0 = time.perf_counter()
                pm.loglik_reference(levels, card, masks[:1], [net.tables])
                row["cpu_rows"], row["cpu_rows_per_s"] = cpu_rows, cpu_rows / (time.perf_counter() - t0)
            res["loglik"].append(row)
            print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
