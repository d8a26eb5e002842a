"""Local and hybrid structure learning (dvs_ci_tests_group, dvs_mmpc_update) on asia (n = 8), sachs (n = 11) and
a seeded 37-variable network sampled on the device (``generate_dags``, ``FittedBN.from_tables``, ``sample``).

(a) The grouped kernel: the group list of every MMPC round, through dvs_ci_tests_group and — the same (x, y | Z) tests, one
    workgroup each — through dvs_ci_tests, alternating in one process: tests per second of both and their ratio, by the host
    clock around ``--inner`` launches that end in a device synchronise, and the kernels' own time from the library's profile.
(b) End to end: the wall time of ``mmpc`` and of ``pc_stable`` with their group and test counts.
(c) Hybrid: ``mmhc`` next to a plain ``hill_climb`` from the empty graph: time, score, SHD to the generating network.
Writes profiles/mmpc_bench.json.

    python bench_mmpc.py [--repeats 5] [--inner 20] [--rows 5000]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_strength import synthetic_network
from dags_vae_search_amd import (BNLearnWrapper, FittedBN, _lib as dl, compare_structures, hill_climb, mmhc, mmpc, pc_stable,
                                 sample)
from dags_vae_search_amd import local
from tests import hillclimb_corpus as hc
from tests import scoring_corpus as sc

HERE = os.path.dirname(os.path.abspath(__file__))


def wall_ms(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, out


def kernels_ms(fn, prefixes):
    lib = dl.load()
    lib.dvs_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    prof = dl.profile_collect(lib)
    lib.dvs_profile_enable(0)
    return {k: {"launches": c, "ms": round(ms, 4)} for k, (c, ms) in prof.items() if k.startswith(prefixes)}


def bits(m):
    return [i for i in range(m.bit_length()) if (m >> i) & 1]


def dev_u64(values):
    return torch.from_numpy(np.array(values, np.uint64).view(np.int64)).cuda()


def configurations(rows):
    for name in ("asia", "sachs"):
        data = np.load(os.path.join(HERE, "tests", "golden", f"bn_{name}_data.npz"))["data"].astype(np.uint8)
        known = sc.masks_of(8, hc.ASIA_KNOWN)[0] if name == "asia" else None
        yield name, known, BNLearnWrapper(name, "bic", data=data)
    parents, cards, tables = synthetic_network()
    packed = sample(FittedBN.from_tables(parents, cards, tables), rows, seed=371)
    yield "syn37", parents, BNLearnWrapper.from_packed("syn37", "bic", packed, cards)


def round_rows(name, ev, repeats, inner):
    """(a): every round of mmpc on this data set, both ways"""
    lib, p, n = ev.lib, dl.ptr, ev.n_vars
    card = [int(c) for c in ev.card_host]
    rounds = []
    local._mmpc(ev, 0.05, "mi", 3, None, rounds)             # the group list of every round, with the LDS size mmpc gave it
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    out_rows = []
    top = sorted(card, reverse=True)
    for r, (phase, target, cond, cands, lds) in enumerate(rounds):
        G = len(target)
        tests = [(x, t, z) for t, z, c in zip(target, cond, cands) for x in bits(c)]
        T = len(tests)
        if T == 0:
            continue
        d_t, d_z, d_c = torch.tensor(target, dtype=torch.int32, device="cuda"), dev_u64(cond), dev_u64(cands)
        pairs = torch.tensor([[x, t] for x, t, _ in tests], dtype=torch.int32, device="cuda")
        zs = dev_u64([z for _, _, z in tests])
        level = max(bin(z).count("1") for z in cond)
        max_cells = max(1, min(int(np.prod(top[:level + 2])), dl.CI_MAX_CELLS))   # what pc.py gives dvs_ci_tests at this level
        out_g = torch.empty(G, n, 3, dtype=torch.float64, device="cuda")
        out_t = torch.empty(T, 3, dtype=torch.float64, device="cuda")

        def grouped():
            dl.check(lib, lib.dvs_ci_tests_group(G, n, ev.n_samples, p(ev.packed), p(ev.card), p(d_t), p(d_z), p(d_c), 0, lds, p(out_g),
                                                 dl.nbytes(out_g), p(status), dl.stream()), "dvs_ci_tests_group")

        def per_test():
            dl.check(lib, lib.dvs_ci_tests(T, n, ev.n_samples, p(ev.packed), p(ev.card), p(pairs), p(zs), 0, max_cells, p(out_t), T * 24,
                                           p(status), dl.stream()), "dvs_ci_tests")
        wall_ms(grouped, 3), wall_ms(per_test, 3)            # warm-up
        tg, tp = [], []
        for _ in range(repeats):                             # alternating
            tg.append(wall_ms(grouped, inner)[0])
            tp.append(wall_ms(per_test, inner)[0])
        # the same bytes, at the sizes timed
        flat = out_g[torch.tensor([g for g, c in enumerate(cands) for _ in bits(c)], device="cuda"),
                     torch.tensor([x for x, _, _ in tests], device="cuda")]
        equal = flat.cpu().numpy().tobytes() == out_t.cpu().numpy().tobytes()
        kg, kp = kernels_ms(grouped, ("k_ci",)), kernels_ms(per_test, ("k_ci",))
        mg, mp = float(np.median(tg)), float(np.median(tp))
        row = {"name": name, "n": n, "samples": ev.n_samples, "round": r, "phase": phase, "groups": G, "tests": T,
               "largest_cond": level, "lds_cells": lds, "per_test_max_cells": max_cells, "equal_bytes": equal,
               "grouped_ms": [round(x, 4) for x in tg], "per_test_ms": [round(x, 4) for x in tp],
               "grouped_tests_per_s": round(T / (mg * 1e-3)), "per_test_tests_per_s": round(T / (mp * 1e-3)),
               "ratio_wall": round(mp / mg, 3), "grouped_kernel_ms": kg["k_ci_group"]["ms"], "per_test_kernel_ms": kp["k_ci_tests"]["ms"],
               "ratio_kernel": round(kp["k_ci_tests"]["ms"] / kg["k_ci_group"]["ms"], 3)}
        out_rows.append(row)
        print(row, flush=True)
    return out_rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mmpc_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "inner": args.inner,
           "timing": "host clock around `inner` launches that end in a device synchronise, medians over `repeats`, the two kernels "
                     "alternating in one process; kernel ms from the library's profile (device events), one launch",
           "grouped_kernel": [], "end_to_end": [], "hybrid": []}
    edges = lambda rows, n: int(sum(bin(int(a) & ((1 << n) - 1)).count("1") for a in rows.cpu()) // 2)
    for name, known, ev in configurations(args.rows):
        n = ev.n_vars
        res["grouped_kernel"] += round_rows(name, ev, args.repeats, args.inner)

        cap = 3 if name == "syn37" else None                 # as bench_pc.py caps PC-stable on the 37-variable set
        mmpc(ev), pc_stable(ev, max_cond=cap)                # warm-up
        tm, tc = [], []
        for _ in range(args.repeats):
            t, m = wall_ms(lambda: mmpc(ev))
            tm.append(t)
            t, c = wall_ms(lambda: pc_stable(ev, max_cond=cap))
            tc.append(t)
        row = {"name": name, "n": n, "samples": ev.n_samples, "mmpc_ms": [round(x, 3) for x in tm], "mmpc_groups_per_round": m.groups_per_round,
               "mmpc_edges": edges(m.skeleton, n), "mmpc_refused": m.refused, "mmpc_asymmetric": m.asymmetric,
               "mmpc_kernels": kernels_ms(lambda: mmpc(ev), ("k_ci", "k_mmpc")),
               "pc_stable_ms": [round(x, 3) for x in tc], "pc_stable_max_cond": cap, "pc_stable_tests_per_level": c.tests_per_level,
               "pc_stable_edges": edges(c.skeleton, n), "same_skeleton": bool(torch.equal(m.skeleton, c.skeleton))}
        res["end_to_end"].append(row)
        print(row, flush=True)

        kw = dict(max_steps=max(16, n * n))
        mmhc(ev, maximize_args=kw), hill_climb(ev, batch=1, **kw)
        th, tf = [], []
        for _ in range(args.repeats):
            t, h = wall_ms(lambda: mmhc(ev, maximize_args=kw))
            th.append(t)
            t, f = wall_ms(lambda: hill_climb(ev, batch=1, **kw))
            tf.append(t)
        row = {"name": name, "n": n, "samples": ev.n_samples, "max_steps": kw["max_steps"], "mmhc_ms": [round(x, 3) for x in th],
               "mmhc_score": float(h.search.scores[0]), "mmhc_steps": int(h.search.steps[0]),
               "hill_climb_ms": [round(x, 3) for x in tf], "hill_climb_score": float(f.scores[0]), "hill_climb_steps": int(f.steps[0])}
        if known is not None:
            target = torch.from_numpy(np.ascontiguousarray(known, np.uint64).view(np.int64).copy()).cuda()
            row["mmhc_shd"] = int(compare_structures(h.search.parents, target).shd[0])
            row["hill_climb_shd"] = int(compare_structures(f.parents, target).shd[0])
        res["hybrid"].append(row)
        print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
