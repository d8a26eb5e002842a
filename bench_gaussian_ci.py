"""Gaussian CI tests (include/dvs_gaussian_ci.h) at 5000 rows and n = 8 / 11 / 37: the time of one PC level's tests
(levels 0 to 3 of the complete graph, through ``dvs_pc_expand`` and ``dvs_gbn_ci_tests``); every (target, conditioning set)
group of a level through the grouped call and the same tests through the per-test call; ``pc_stable`` and ``mmpc`` under ``zf``
end to end, beside the discrete ``mi`` on the same rows cut into three levels at their terciles; and the numpy restatement of the
header's definitions on the CPU (tests/gaussian_ci_corpus.py), timed on a share of the tests.  Seeded linear-Gaussian data
(``gauss_data``).  No threshold rides on any of these numbers.  Writes profiles/gaussian_ci_bench.json.

    python bench_gaussian_ci.py [--rows 5000] [--repeats 5]
"""
import argparse
import json
import os
from itertools import combinations

import numpy as np
import torch

from bench_gaussian import cpu_s, discretised, median_s
from dags_vae_search_amd import BNLearnWrapper, GaussianEvaluator, mmpc, pc_stable
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd.local import _launch_group
from dags_vae_search_amd.pc import _run_gaussian_tests, level_tests
from tests import gaussian_ci_corpus as gi
from tests import gaussian_corpus as gc

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64


def pc_level(ev, level):
    """the tests of a PC-stable level on the complete graph, expanded on the device -> (pairs int32 [T, 2], cond int64 [T])"""
    n, lib, p = ev.n_vars, ev.lib, dl.ptr
    adj = [((1 << n) - 1) & ~(1 << v) for v in range(n)]
    pair_xy, offsets = level_tests(adj, level)
    T, P = offsets[-1], len(pair_xy)
    d_adj = torch.from_numpy(np.array(adj, U64).view(np.int64)).cuda()
    d_xy = torch.tensor(pair_xy, dtype=torch.int32, device="cuda")
    d_off = torch.tensor(offsets, dtype=torch.int64, device="cuda")
    pairs = torch.empty(T, 2, dtype=torch.int32, device="cuda")
    cond = torch.empty(T, dtype=torch.int64, device="cuda")
    dl.check(lib, lib.dvs_pc_expand(P, n, level, p(d_adj), p(d_xy), p(d_off), T, p(pairs), p(cond), T * 8, dl.stream()), "dvs_pc_expand")
    return pairs, cond


def level_groups(n, level):
    """every (target, Z) with |Z| = level and all other variables as candidates -> (target, cond, candidates) numpy arrays, and
    the same tests one by one (pairs [T, 2] = (target, candidate), cond [T])"""
    full = (1 << n) - 1
    target, cond = [], []
    for t in range(n):
        for Z in combinations([v for v in range(n) if v != t], level):
            target.append(t)
            cond.append(sum(1 << z for z in Z))
    target, cond = np.asarray(target, np.int32), np.asarray(cond, np.int64)
    cand = full & ~cond & ~(np.int64(1) << target.astype(np.int64))
    px, py, pz = [], [], []
    for c in range(n):
        sel = ((cand >> c) & 1).astype(bool)
        px.append(target[sel])
        py.append(np.full(int(sel.sum()), c, np.int32))
        pz.append(cond[sel])
    pairs = np.stack([np.concatenate(px), np.concatenate(py)], 1).astype(np.int32)
    return target, cond, cand, pairs, np.concatenate(pz)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 11, 37])
    ap.add_argument("--levels", type=int, nargs="+", default=[0, 1, 2, 3])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "gaussian_ci_bench.json"))
    args = ap.parse_args()
    S = args.rows
    res = {"device": torch.cuda.get_device_name(0), "rows": S, "repeats": args.repeats,
           "timing": "host clock around windows of back-to-back calls (about 50 ms each, sized from a probe call) that end in a "
                     "device synchronise; the median window of the repeats divided by its calls, after one warm-up call; the "
                     "numpy restatement is timed once on the stated share of the tests",
           "pc_level": [], "grouped_vs_per_test": [], "pc_stable": [], "mmpc": []}
    zf = dl.GCI_TYPES["zf"]
    for n in args.sizes:
        x = np.array(gc.gauss_data(n, S))
        ev = GaussianEvaluator(f"syn{n}", "bic-g", data=x)
        disc = BNLearnWrapper(f"syn{n}-3", "bic", data=discretised(x))
        mom = ev.moments[0].cpu().numpy()
        for level in args.levels:
            # ---- one PC level's tests of the complete graph through dvs_gbn_ci_tests
            pairs, cond = pc_level(ev, level)
            T = cond.numel()
            out = torch.empty(T, 3, dtype=torch.float64, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            for name in gi.TYPES:
                typ = dl.GCI_TYPES[name]
                t = median_s(lambda: _run_gaussian_tests(ev, pairs, cond, typ, out, status, T), args.repeats)
                row = {"n": n, "level": level, "test": name, "tests": T, "ms": round(t * 1e3, 4), "tests_per_s": round(T / t)}
                if name == "zf":
                    share = min(T, 400)
                    hp, hc = pairs[:share].cpu().numpy(), cond[:share].cpu().numpy().view(U64)
                    t_np = cpu_s(lambda: [gi.restated_test(mom, n, hp[i, 0], hp[i, 1], hc[i], "zf") for i in range(share)])
                    row.update(numpy_restatement_tests_per_s=round(share / t_np), numpy_tests_timed=share)
                res["pc_level"].append(row)
                print("pc_level", row, flush=True)
            assert int(status.item()) == 0
            # ---- every (target, Z) group of the level through the grouped call, and its tests one by one
            target, gcond, cand, tp, tz = level_groups(n, level)
            d_t, d_z, d_c = (torch.from_numpy(a).cuda() for a in (target, gcond, cand))
            d_p, d_pz = torch.from_numpy(tp).cuda(), torch.from_numpy(tz).cuda()
            G, T = len(target), len(tz)
            gout = torch.empty(G, n, 3, dtype=torch.float64, device="cuda")
            tout = torch.empty(T, 3, dtype=torch.float64, device="cuda")
            tg = median_s(lambda: _launch_group(ev, d_t, d_z, d_c, zf, 0, gout, status), args.repeats)
            tt = median_s(lambda: _run_gaussian_tests(ev, d_p, d_pz, zf, tout, status, T), args.repeats)
            row = {"n": n, "level": level, "test": "zf", "groups": G, "tests": T, "grouped_ms": round(tg * 1e3, 4),
                   "per_test_ms": round(tt * 1e3, 4), "grouped_tests_per_s": round(T / tg), "per_test_tests_per_s": round(T / tt),
                   "per_test_over_grouped": round(tt / tg, 3)}
            res["grouped_vs_per_test"].append(row)
            print("grouped_vs_per_test", row, flush=True)
        # ---- pc_stable and mmpc end to end: zf on the real rows, mi on the same rows in three levels
        for name, e, test in (("zf", ev, "zf"), ("discrete mi", disc, "mi")):
            t = median_s(lambda: pc_stable(e, test=test), args.repeats)
            r = pc_stable(e, test=test)
            row = {"n": n, "test": name, "tests_per_level": r.tests_per_level, "edges": sum(bin(int(a)).count("1") for a in
                   r.skeleton.cpu().numpy().view(U64)) // 2, "refused": r.refused, "ms": round(t * 1e3, 3)}
            res["pc_stable"].append(row)
            print("pc_stable", row, flush=True)
            t = median_s(lambda: mmpc(e, test=test), args.repeats)
            r = mmpc(e, test=test)
            row = {"n": n, "test": name, "groups_per_round": r.groups_per_round, "edges": sum(bin(int(a)).count("1") for a in
                   r.skeleton.cpu().numpy().view(U64)) // 2, "refused": r.refused, "ms": round(t * 1e3, 3)}
            res["mmpc"].append(row)
            print("mmpc", row, flush=True)
    res["not_measured"] = ["kernel times by rocprofv3 (only end-to-end call times are taken)", "shares of peak",
                           "row counts other than --rows (the tests read the moments, not the rows: only the moments call does)",
                           "n = 48", "levels above 3", "rsmax2 / mmhc end to end"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
