"""Conditional Gaussian networks on mixed data (include/dvs_mixed.h).

1. ``dvs_cg_partition`` + ``dvs_cg_moments`` per request at S in {5000, 100000} rows and n_c in {8, 24} real columns, for sets D of
   1, 12 and 96 configurations, beside ``dvs_gbn_moments`` on all rows of the same columns: both sum the same products, and the
   Gaussian kernel is the yardstick.  The outputs are compared as bytes at the sizes timed (the D = {} table against
   ``dvs_gbn_moments``, every other table against a second run).
2. The share of ``score_masks`` and of a full toggle pass spent on building tables, at a cold and at a warm cache.
3. ``hill_climb`` wall time and moves on mixed data with 8 + 8 and 24 + 24 variables, with the cache's hit rate and the
   read-back cost per pass.

Host clock around launches that end in a device synchronise, the median of ``--repeats`` runs after one warm-up.  Writes
profiles/mixed_bench.json.

    python bench_mixed.py [--repeats 5] [--quick]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from dags_vae_search_amd import MixedEvaluator, hill_climb
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd.gaussian import _moments

HERE = os.path.dirname(os.path.abspath(__file__))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def median_s(fn, repeats):
    fn()
    return float(np.median([wall(fn)[0] for _ in range(repeats)]))


def mixed_rows(nd, nc, S, seed=0):
    """nd factors of 2 / 3 / 4 levels (a chain of noisy copies) then nc real columns, each a regression on the one before whose
    intercept follows a factor"""
    rng = np.random.default_rng(3900 + seed)
    card = [(2, 3, 4)[i % 3] for i in range(nd)] + [0] * nc
    a = np.zeros((S, nd + nc))
    for i in range(nd):
        src = a[:, i - 1] if i else np.zeros(S)
        a[:, i] = np.where(rng.random(S) < 0.6, src % card[i], rng.integers(0, card[i], S))
    for j in range(nc):
        prev = a[:, nd + j - 1] if j else np.zeros(S)
        a[:, nd + j] = 0.6 * prev + 0.8 * a[:, j % nd] + rng.normal(0, 1.0, S)
    return a, card


def bytes_of(t):
    return t.cpu().numpy().tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="S = 5000 only, the 8 + 8 climb only")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mixed_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "host clock around calls that end in a device synchronise; the median of the repeats after one warm-up call",
           "tables": [], "cache": [], "hill_climb": []}
    lib = dl.load()
    # ---- 1. partition + ragged moments per request, beside dvs_gbn_moments on all rows
    for S in ((5000,) if args.quick else (5000, 100000)):
        for nc in (8, 24):
            a, card = mixed_rows(6, nc, S)
            ev = MixedEvaluator("bench", "bic-cg", data=a, discrete=card)
            t_g = median_s(lambda: _moments(lib, ev.x, None), args.repeats)
            gauss = _moments(lib, ev.x, None)
            for D in (0, 0b000110, 0b111100):                # q = 1, 12, 96
                q = ev.configurations(D)
                t_b = median_s(lambda: ev.build_tables([D] * 8), args.repeats) / 8
                t_1 = median_s(lambda: ev.build_tables([D]), args.repeats)
                one, two = ev.build_tables([D])[0], ev.build_tables([D, D])[1]
                assert bytes_of(one) == bytes_of(two), "two builds give equal bytes"
                if D == 0:
                    assert bytes_of(one[0]) == bytes_of(gauss[0]), "D = {} is dvs_gbn_moments on all rows"
                res["tables"].append({"rows": S, "n_cont": nc, "configurations": q, "gbn_moments_ms": 1e3 * t_g,
                                      "one_request_ms": 1e3 * t_1, "per_request_of_8_ms": 1e3 * t_b,
                                      "ratio_one_request": t_1 / t_g, "ratio_per_request_of_8": t_b / t_g})
                print(res["tables"][-1], flush=True)
    # ---- 2. the share of table building in the scorer and in the toggle pass: a cold against a warm cache
    for nd, nc, B in ((8, 8, 64), (24, 24, 8)):
        a, card = mixed_rows(nd, nc, 5000, seed=1)
        ev = MixedEvaluator("bench", "bic-cg", data=a, discrete=card)
        n = nd + nc
        rng = np.random.default_rng(7)
        P = np.zeros((B, n), np.uint64)
        for b in range(B):
            for v in range(nd, n):                           # every real column: up to two factors and two earlier real columns
                pa = list(rng.choice(nd, size=int(rng.integers(0, 3)), replace=False)) + \
                    list(rng.choice(np.arange(nd, v), size=min(v - nd, int(rng.integers(0, 3))), replace=False))
                P[b, v] = np.uint64(sum(1 << int(u) for u in pa))
        P = torch.from_numpy(P.view(np.int64)).cuda()
        for name, fn in (("score_masks", lambda: ev.score_masks(P)), ("toggle_scores", lambda: ev.toggle_scores(P))):
            def cold():
                ev.clear_cache()
                return fn()
            t_cold, t_warm = median_s(cold, args.repeats), median_s(fn, args.repeats)
            out_c, out_w = cold(), fn()
            same = bytes_of(out_c) == bytes_of(out_w) if torch.is_tensor(out_c) else all(bytes_of(x) == bytes_of(y) for x, y in zip(out_c, out_w))
            assert same, "a cold and a warm cache give equal bytes"
            ev.clear_cache()
            before = dict(ev.cache_stats)
            fn()
            built = ev.cache_stats["built"] - before["built"]
            res["cache"].append({"call": name, "factors": nd, "real": nc, "batch": B, "tables_built_cold": built, "cold_ms": 1e3 * t_cold,
                                 "warm_ms": 1e3 * t_warm, "table_building_share_cold": 1 - t_warm / t_cold})
            print(res["cache"][-1], flush=True)
    # ---- 3. hill_climb end to end
    for nd, nc in (((8, 8),) if args.quick else ((8, 8), (24, 24))):
        a, card = mixed_rows(nd, nc, 5000, seed=2)
        ev = MixedEvaluator("bench", "bic-cg", data=a, discrete=card)
        B = 16

        def climb():
            ev.clear_cache()
            return hill_climb(ev, batch=B, max_steps=200, max_parents=4)
        t, out = median_s(climb, max(1, args.repeats // 2 + 1)), climb()
        again = climb()
        assert bytes_of(out.parents) == bytes_of(again.parents) and bytes_of(out.scores) == bytes_of(again.scores)
        ev.clear_cache()
        for k in ev.cache_stats:
            ev.cache_stats[k] = 0
        climb()
        st = ev.cache_stats
        # the read-back alone: the unique masks of one incremental pass brought to the host
        masks = torch.randint(0, 1 << nd, (2 * B, nd + nc), device="cuda")
        t_rb = median_s(lambda: torch.unique(masks).cpu(), args.repeats)
        res["hill_climb"].append({"factors": nd, "real": nc, "rows": 5000, "batch": B, "wall_s": t, "moves": int(out.steps.sum()),
                                  "passes": st["passes"], "tables_built": st["built"], "cache_hit_rate": st["hits"] / max(1, st["hits"] + st["misses"]),
                                  "ms_per_pass": 1e3 * t / max(1, st["passes"]), "readback_ms_per_pass": 1e3 * t_rb})
        print(res["hill_climb"][-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
