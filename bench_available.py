"""Structure search on incomplete data (dvs_bn_scores_avail, dvs_bn_toggle_scores_avail, structural_em).

(a) The cost of the mask: structures per second of the available-case scorer with every value observed against the plain
    scorer (loglik) on the same rows and structures — the counts are identical — measured in the same call, alternating,
    median of the wall times with a device synchronise.
(b) The same with 10 % and 30 % of the values missing completely at random.
(c) One ``structural_em`` iteration, and the structural Hamming distance to the generating CPDAG (``compare_structures``) of
    three learners: ``hill_climb`` (bic) on the complete rows only, ``hill_climb`` on the ``pnal`` view, ``structural_em``; and,
    because the default penalty of pnal turned out to admit almost no arc at these sizes, ``hill_climb`` on the ``pnal`` view
    with k = log(S) / (2 S), which is bic's penalty on the per-row scale.
Data: rows drawn by ``sample`` from asia (n = 8) and from a seeded 37-variable banded network.  Nothing is asserted about speed
or distance.  Writes profiles/available_bench.json.

The scorer is timed on a batch large enough that a call takes milliseconds (2048 distinct structures, repeated); next to the
wall times the kernels' own times from the library's HIP events, in a run of their own.  The learners run once each.

    python bench_available.py [--repeats 5] [--rows 5000] [--structures 32768]
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from bench_em import alternating, wall_ms
from dags_vae_search_amd import _lib as dl
from dags_vae_search_amd import (BNLearnWrapper, FittedBN, available_case_evaluator, compare_structures, hill_climb, sample,
                                 structural_em)
from tests import eliminate_corpus as ec

HERE = os.path.dirname(os.path.abspath(__file__))


def band37():
    """37 variables, 2..4 levels, 1..2 parents within the 4 preceding indices, seeded tables with one favoured level per row"""
    rng = np.random.default_rng(3701)
    n = 37
    card = rng.integers(2, 5, n)
    masks, tables = [0] * n, []
    for v in range(n):
        ps = [] if v == 0 else sorted(set(int(u) for u in rng.integers(max(0, v - 4), v, int(rng.integers(1, 3)))))
        masks[v] = sum(1 << u for u in ps)
        q = int(np.prod([card[u] for u in ps])) if ps else 1
        t = rng.dirichlet(np.full(card[v], 0.5), q)
        tables.append(t)
    return [int(c) for c in card], masks, tables


def local_kernel_ms(fn):
    """{kernel: ms} of the two counting kernels over one call of fn, from the library's HIP events"""
    lib = dl.load()
    lib.dvs_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    prof = dl.profile_collect(lib)
    lib.dvs_profile_enable(0)
    return {k: round(ms, 4) for k, (c, ms) in prof.items() if k in ("k_bic_local", "k_bn_local_avail")}


def random_structures(n, B, max_parents, seed, distinct=2048):
    """int64 [B, n]: parent sets of up to max_parents variables of lower index under a random order; `distinct` of them, repeated"""
    rng = np.random.default_rng(seed)
    out = np.zeros((min(B, distinct), n), np.uint64)
    for b in range(len(out)):
        order = rng.permutation(n)
        for i in range(1, n):
            k = int(rng.integers(0, min(i, max_parents) + 1))
            for u in rng.choice(order[:i], k, replace=False):
                out[b, order[i]] |= np.uint64(1) << np.uint64(int(u))
    out = np.tile(out, ((B + len(out) - 1) // len(out), 1))[:B]
    return torch.from_numpy(np.ascontiguousarray(out).view(np.int64)).cuda()


def observed_words(R, n, rate, seed):
    seen = np.random.default_rng(seed).random((R, n)) >= rate
    return seen, torch.from_numpy((seen.astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(1, dtype=np.uint64).view(np.int64)).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, default=5000)
    ap.add_argument("--structures", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "available_bench.json"))
    args = ap.parse_args()
    R, B = args.rows, args.structures
    res = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "rows": R, "structures": B, "scorer": [], "learners": []}
    asia = ec.network("asia")
    nets = (("asia", [int(c) for c in asia.card], [int(m) for m in asia.masks], asia.tables), ("band37", *band37()))
    for name, card, masks, tables in nets:
        n = len(card)
        fitted = FittedBN.from_tables(masks, card, tables)
        rows = sample(fitted, R, seed=3)
        target = torch.tensor(masks, dtype=torch.int64, device="cuda")
        plain = BNLearnWrapper.from_packed(name, "loglik", rows, card)
        structures = random_structures(n, B, 3, seed=40 + n)
        for rate in (0.0, 0.1, 0.3):
            seen, observed = observed_words(R, n, rate, seed=300 + n)
            view = plain.available_case(observed, "nal")
            ms_plain, ms_view = alternating([lambda: plain.score_masks(structures), lambda: view.score_masks(structures)], args.repeats)
            used = view.used(structures).double().mean().item()
            kern = {**local_kernel_ms(lambda: plain.score_masks(structures)), **local_kernel_ms(lambda: view.score_masks(structures))}
            row = dict(name=name, n=n, missing=rate, plain_ms=ms_plain, avail_ms=ms_view, kernel_ms=kern,
                       avail_over_plain_kernel=kern["k_bn_local_avail"] / kern["k_bic_local"], plain_structures_per_s=B / (ms_plain * 1e-3),
                       avail_structures_per_s=B / (ms_view * 1e-3), avail_over_plain=ms_view / ms_plain, mean_rows_used=used)
            res["scorer"].append(row)
            print(row, flush=True)
            if rate == 0.0:
                continue
            data = (rows, observed)
            shd = lambda parents: int(compare_structures(parents.reshape(1, n), target).shd[0].item())
            complete = torch.from_numpy(seen.all(1)).cuda()
            n_complete = int(complete.sum())
            t0 = time.perf_counter()
            if n_complete:
                ev = BNLearnWrapper.from_packed(name, "bic", rows[complete].contiguous(), card)
                shd_complete = shd(hill_climb(ev, batch=1, max_steps=n * n, max_parents=3).parents[0])
            else:
                shd_complete = None
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            pnal = available_case_evaluator(data, card, "pnal")
            shd_pnal = shd(hill_climb(pnal, batch=1, max_steps=n * n, max_parents=3).parents[0])
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            k_bic = float(np.log(R) / (2 * R))               # bic on the per-row scale of nal: LL / S - (log S / 2 S) params
            pnal_bic = available_case_evaluator(data, card, "pnal", k=k_bic)
            found = hill_climb(pnal_bic, batch=1, max_steps=n * n, max_parents=3)
            shd_pnal_bic, steps_pnal_bic = shd(found.parents[0]), int(found.steps[0])
            found = hill_climb(pnal, batch=1, max_steps=n * n, max_parents=3)
            steps_pnal = int(found.steps[0])
            torch.cuda.synchronize()
            t2b = time.perf_counter()
            em = structural_em(data, card)
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            one_iteration_ms = wall_ms(lambda: structural_em(data, card, max_iter=1))
            row = dict(name=name, n=n, missing=rate, rows=R, complete_rows=n_complete, shd_complete_rows_hc=shd_complete,
                       shd_pnal_hc=shd_pnal, shd_structural_em=shd(em.parents), complete_rows_hc_s=t1 - t0, pnal_hc_s=t2 - t1,
                       structural_em_s=t3 - t2b, pnal_default_k=pnal.penalty, pnal_hc_steps=steps_pnal,
                       pnal_bic_scale_k=k_bic, shd_pnal_bic_scale_hc=shd_pnal_bic, pnal_bic_scale_hc_steps=steps_pnal_bic, structural_em_iterations=em.iterations, structural_em_converged=em.converged,
                       structural_em_left_out=[e["left_out"] for e in em.trace],
                       structural_em_log_likelihood=[e["log_likelihood"] for e in em.trace],
                       structural_em_one_iteration_ms=one_iteration_ms)
            res["learners"].append(row)
            print(row, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
