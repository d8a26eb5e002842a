"""Order MCMC (dvs_order_mcmc) on asia (n = 8), sachs (n = 11, at most 3 parents) and a synthetic n = 37 data
set (5 000 rows, at most 3 parents: 289 k families): the time to build the family list, and for window in {1, 4, n - 1} the
kernel time of 256 chains from the library's HIP-event profile, steps per second per chain and in total, and the acceptance
rate.  On asia and sachs also the largest |prob - arc_posterior's prob| next to the largest std_error, the top chain's
best_score minus exact_search's optimum and how many chains reached it.  Writes profiles/order_mcmc_bench.json.

    python bench_ordermc.py [--chains 256] [--steps 2000] [--steps-wide 500]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, FamilyScores, _lib as dl
from dags_vae_search_amd import arc_posterior, exact_search, family_scores, local_score_table, order_mcmc
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def kernel_ms(fn):
    lib = dl.load()
    lib.dvs_profile_enable(1)
    out = fn()
    torch.cuda.synchronize()
    prof = dl.profile_collect(lib)
    lib.dvs_profile_enable(0)
    return out, {k: round(ms, 4) for k, (c, ms) in prof.items() if k.startswith("k_omc")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--steps-wide", type=int, default=500, help="steps at n = 37")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "order_mcmc_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "chains": args.chains, "workloads": []}
    for name, cap in (("asia", None), ("sachs", 3), ("syn37", 3)):
        if name == "syn37":
            data, _ = sc.synthetic_dataset(37, 5000, np.random.default_rng(37).integers(2, 5, 37), seed=937)
        else:
            data = hc.hc_case(name).data
        ev = BNLearnWrapper(name, "bde", data=data, iss=10.0)
        n = ev.n_vars
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if name == "syn37":
            fam = family_scores(ev, max_parents=cap)
            exact = best = None
        else:
            # the list on the exact posterior's own cells, so that the comparison below is with the same distribution
            fam = FamilyScores.from_table(local_score_table(ev, max_parents=cap), max_parents=cap)
            exact = arc_posterior(ev, max_parents=cap).prob[0]
            best = float(exact_search(ev, max_parents=cap).scores[0])
        torch.cuda.synchronize()
        steps = args.steps_wide if name == "syn37" else args.steps
        row = {"name": name, "n": n, "samples": ev.n_samples, "max_parents": cap, "score": "bde iss 10",
               "families": fam.n_families, "list_mb": fam.n_families * 16 / 2 ** 20,
               "list_and_yardsticks_ms": (time.perf_counter() - t0) * 1e3, "steps": steps, "windows": []}
        for window in sorted({1, min(4, n - 1), n - 1}):
            order_mcmc(fam, chains=args.chains, steps=10, window=window, seed=1)                # first launch
            r, prof = kernel_ms(lambda: order_mcmc(fam, chains=args.chains, steps=steps, window=window, seed=1))
            ms = prof.get("k_omc_chain", float("nan"))
            w = {"window": window, "kernels_ms": prof, "steps_per_s_per_chain": steps / ms * 1e3,
                 "steps_per_s_total": steps * args.chains / ms * 1e3, "accept_rate": float(r.accept_rate.mean()),
                 "kept_per_chain": int(r.kept[0]), "largest_std_error": float(r.std_error.max())}
            if exact is not None:
                w["largest_prob_error"] = float((r.prob - exact).abs().max())
                w["best_minus_optimum"] = r.best()[1] - best
                w["chains_at_optimum"] = int(((r.best_score - best).abs() <= 1e-9 * abs(best)).sum())
            row["windows"].append(w)
            print(name, w, flush=True)
        res["workloads"].append(row)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
