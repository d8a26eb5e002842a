"""Monte Carlo permutation CI tests (dvs_ci_perm_tests) on asia (n = 8), sachs (n = 11) and a seeded 37-variable
network sampled on the device, at ``--rows`` samples and ``--perms`` permutations.

(a) Per test type: every pair unconditionally and given one other variable, in one ``ci_tests`` call: kernel time from the
    library's profile (device events), wall time as the median of ``--repeats`` drained calls, draws per second (the draws
    counted on the host from the tables: sum over configurations of n_z less the last occupied row, times the permutations
    each test used), and the numpy restatement of tests/permtest_corpus.py on the first test as a reference column.
(b) The effect of ``slices`` on the raw call at 28, 1 000 and 20 000 mc-mi tests (asia's 28 pairs, repeated).
(c) ``pc_stable`` under mc-mi and smc-mi against mi, and what smc saves.
Writes profiles/permtest_bench.json.

    python bench_permtest.py [--repeats 5] [--rows 5000] [--perms 5000] [--skip-large]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_mmpc import configurations, dev_u64, kernels_ms, wall_ms
from dags_vae_search_amd import _lib as dl, ci_tests, pc_stable
from dags_vae_search_amd.pc import PERM_FILL
from tests import pc_corpus as pc
from tests import permtest_corpus as pt

HERE = os.path.dirname(os.path.abspath(__file__))


def unpack(ev):
    """uint8 [S, n] level codes of the evaluator's packed rows"""
    words = ev.packed.cpu().numpy().view(np.uint64)
    return np.stack([((words[:, v >> 4] >> np.uint64(4 * (v & 15))) & np.uint64(15)).astype(np.uint8) for v in range(ev.n_vars)], 1)


def draws_of(tab):
    """draws one permutation makes on the observed table [q, rx, ry]"""
    rows = tab.sum(2)
    last = np.where(rows > 0, np.arange(rows.shape[1])[None], -1).max(1)
    return int(sum(rows[z].sum() - rows[z, last[z]] for z in range(len(rows)) if last[z] >= 0))


def type_rows(name, ev, data, B, repeats):
    n = ev.n_vars
    card = ev.card_host
    tests = [(x, y, ()) for x in range(n) for y in range(x + 1, n)]
    tests += [(x, y, (min(set(range(n)) - {x, y}),)) for x, y, _ in tests]
    pairs = torch.tensor([[x, y] for x, y, _ in tests], dtype=torch.int32, device="cuda")
    cond = dev_u64([pc.mask_of(z) for _, _, z in tests])
    per_test = np.array([draws_of(pc.ci_table(data, card, x, y, z)) for x, y, z in tests], np.int64)
    t0 = time.perf_counter()
    x, y, z = tests[0]
    pt.perm_reference(pc.ci_table(data, card, x, y, z), True, B, 0, 0)
    numpy_s = time.perf_counter() - t0
    rows = []
    for typ in ("mi",) + pt.TYPES:
        kw = dict(B=B, seed=1, return_used=True) if typ in pt.TYPES else {}
        fn = lambda: ci_tests(ev, pairs, cond, typ, **kw)
        wall_ms(fn)                                          # warm-up
        walls = [wall_ms(fn)[0] for _ in range(repeats)]
        got = fn()
        kern = kernels_ms(fn, ("k_ci",))
        row = {"name": name, "n": n, "samples": ev.n_samples, "tests": len(tests), "type": typ, "wall_ms": [round(w, 3) for w in walls],
               "kernels": kern}
        if typ in pt.TYPES:
            used = got[1].cpu().numpy().astype(np.int64)
            draws = int((per_test * used).sum())
            k_ms = kern["k_ci_perm"]["ms"]
            row.update(permutations=B, mean_used=round(float(used.mean()), 1), draws=draws, draws_per_s_kernel=round(draws / (k_ms * 1e-3)),
                       draws_per_s_wall=round(draws / (float(np.median(walls)) * 1e-3)),
                       numpy_first_test_s=round(numpy_s, 3), numpy_draws_per_s=round(int(per_test[0]) * B / numpy_s))
        rows.append(row)
        print(row, flush=True)
    return rows


def slices_rows(ev, B, repeats, sizes):
    """(b): asia's 28 unconditional pairs repeated to T tests, mc-mi through the raw call, slices from 1 to all blocks"""
    lib, p, n = ev.lib, dl.ptr, ev.n_vars
    base = [(x, y) for x in range(n) for y in range(x + 1, n)]
    blocks = (B + 255) // 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = []
    for T in sizes:
        pairs = torch.tensor([base[t % len(base)] for t in range(T)], dtype=torch.int32, device="cuda")
        cond = torch.zeros(T, dtype=torch.int64, device="cuda")
        out = torch.empty(T, 3, dtype=torch.float64, device="cuda")
        used = torch.empty(T, dtype=torch.int32, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        work = torch.empty(dl.workspace_bytes(lib, "dvs_ci_perm_workspace_bytes", T, B), dtype=torch.uint8, device="cuda")
        chosen = max(1, min(blocks, -(-PERM_FILL * cus // T)))
        first = None
        for slices in sorted({1, 2, 5, 10, blocks, chosen}):
            def fn():
                dl.check(lib, lib.dvs_ci_perm_tests(T, n, ev.n_samples, p(ev.packed), p(ev.card), p(pairs), p(cond), 0, B, 0.05, 1, 0, slices,
                                                    16, p(work), dl.nbytes(work), p(out), T * 24, p(used), p(status), dl.stream()),
                         "dvs_ci_perm_tests")
            wall_ms(fn)
            walls = [wall_ms(fn)[0] for _ in range(repeats if T < 10000 else 3)]
            bytes_ = out.cpu().numpy().tobytes()
            first = first or bytes_
            row = {"tests": T, "permutations": B, "slices": slices, "workgroups": T * slices, "chosen_by_ci_tests": slices == chosen,
                   "wall_ms": [round(w, 3) for w in walls], "kernel_ms": kernels_ms(fn, ("k_ci",))["k_ci_perm"]["ms"],
                   "equal_bytes": bytes_ == first}
            rows.append(row)
            print(row, flush=True)
    return rows


def pc_rows(name, ev, B, repeats, cap):
    rows = []
    for typ in ("mi", "mc-mi", "smc-mi"):
        kw = dict(B=B, seed=1) if typ != "mi" else {}
        fn = lambda: pc_stable(ev, test=typ, max_cond=cap, **kw)
        wall_ms(fn)
        walls, r = [], None
        for _ in range(repeats):
            t, r = wall_ms(fn)
            walls.append(t)
        row = {"name": name, "type": typ, "max_cond": cap, "wall_ms": [round(w, 3) for w in walls], "tests_per_level": r.tests_per_level,
               "edges": int(sum(bin(int(a) & ((1 << ev.n_vars) - 1)).count("1") for a in r.skeleton.cpu()) // 2), "refused": r.refused,
               "kernels": kernels_ms(fn, ("k_ci", "k_pc"))}
        rows.append(row)
        print(row, flush=True)
    rows[2]["smc_over_mc_wall"] = round(float(np.median(rows[2]["wall_ms"]) / np.median(rows[1]["wall_ms"])), 3)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--perms", type=int, default=5000)
    ap.add_argument("--skip-large", action="store_true", help="leave out the 20 000-test row of (b)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "permtest_bench.json"))
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count,
           "repeats": args.repeats, "rows": args.rows, "permutations": args.perms,
           "timing": "wall: host clock around one call that ends in a device synchronise, `repeats` calls after a warm-up (the list "
                     "holds them all); kernel ms from the library's profile (device events), one call",
           "types": [], "slices": [], "pc_stable": []}
    for name, _, ev in configurations(args.rows):
        if ev.n_samples > args.rows:
            ev = type(ev).from_packed(name, "bic", ev.packed[:args.rows].contiguous(), [int(c) for c in ev.card_host])
        res["types"] += type_rows(name, ev, unpack(ev), args.perms, args.repeats)
        if name == "asia":
            res["slices"] = slices_rows(ev, args.perms, args.repeats, (28, 1000) if args.skip_large else (28, 1000, 20000))
        res["pc_stable"] += pc_rows(name, ev, args.perms, args.repeats, 2 if name == "syn37" else None)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
