"""Constraint-based structure learning (dvs_ci_tests, dvs_pc_*): conditional-independence tests per second at
conditioning-set sizes 0 .. 3 on asia (n = 8), sachs (n = 11) and a seeded 37-variable / 4-level / 5000-sample data set, and
the wall time of pc_stable, each next to the numpy restatement of tests/pc_corpus.py on the CPU (its p-values are mpmath's, so
it is a reference, not a tuned CPU implementation).  Writes profiles/pc_bench.json.

    python bench_pc.py [--repeats 5] [--tests 20000] [--cpu-tests 200]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import BNLearnWrapper, _lib as dl
from dags_vae_search_amd import ci_tests, pc_stable
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
    return {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in prof.items() if k.startswith(("k_ci", "k_pc"))}


def random_tests(n, level, count, seed):
    """(x, y, conditioning variables) with x != y and `level` other variables, seeded"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        pick = rng.choice(n, size=level + 2, replace=False)
        out.append((int(pick[0]), int(pick[1]), tuple(int(z) for z in pick[2:])))
    return out


def datasets():
    yield "asia", pc.e2e_data("asia", 5000)[0], None
    yield "sachs", pc.e2e_data("sachs", 5000)[0], None
    yield "syn37", sc.synthetic_dataset(37, 5000, [4] * 37, seed=937)[0], 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tests", type=int, default=20000)
    ap.add_argument("--cpu-tests", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "pc_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "ci_tests": [], "pc_stable": []}

    for name, data, cap in datasets():
        ev = BNLearnWrapper(name, "bic", data=data)
        card = (data.max(0) + 1).astype(np.uint8)
        n = ev.n_vars
        for level in range(4):
            tests = random_tests(n, level, args.tests, seed=100 * n + level)
            pairs = torch.tensor([[x, y] for x, y, _ in tests], dtype=torch.int32, device="cuda")
            cond = torch.tensor([pc.mask_of(z) for _, _, z in tests], dtype=torch.int64, device="cuda")
            ms = timed(lambda: ci_tests(ev, pairs, cond, "mi"), args.repeats)
            t0 = time.perf_counter()
            for x, y, zs in tests[:args.cpu_tests]:
                pc.data_test(data, card, x, y, pc.mask_of(zs), "mi")
            cpu_s = time.perf_counter() - t0
            row = {"name": name, "n": n, "samples": ev.n_samples, "level": level, "tests": len(tests), "ms": ms,
                   "tests_per_s": len(tests) / (ms * 1e-3), "cpu_tests": min(args.cpu_tests, len(tests)),
                   "cpu_tests_per_s": min(args.cpu_tests, len(tests)) / cpu_s,
                   "kernels": kernels_ms(lambda: ci_tests(ev, pairs, cond, "mi"))}
            res["ci_tests"].append(row)
            print(row, flush=True)

        r = pc_stable(ev, test="mi", max_cond=cap)
        row = {"name": name, "n": n, "samples": ev.n_samples, "max_cond": cap, "tests_per_level": r.tests_per_level,
               "edges": int(sum(bin(int(a) & ((1 << n) - 1)).count("1") for a in r.skeleton.cpu()) // 2), "conflicts": r.conflicts,
               "refused": r.refused, "flags": r.flags, "ms": timed(lambda: pc_stable(ev, test="mi", max_cond=cap), args.repeats),
               "kernels": kernels_ms(lambda: pc_stable(ev, test="mi", max_cond=cap))}
        cpu_cap = cap if cap is None else 1                  # the CPU restatement of the 37-variable set stops after level 1
        t0 = time.perf_counter()
        ref = pc.pc_ref(n, lambda x, y, m: pc.data_test(data, card, x, y, m, "mi")[2] > pc.ALPHA, max_cond=cpu_cap)
        row["cpu_max_cond"], row["cpu_ms"], row["cpu_tests_per_level"] = cpu_cap, (time.perf_counter() - t0) * 1e3, ref.tests_per_level
        if cpu_cap != cap:
            row["ms_at_cpu_max_cond"] = timed(lambda: pc_stable(ev, test="mi", max_cond=cpu_cap), args.repeats)
        res["pc_stable"].append(row)
        print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
