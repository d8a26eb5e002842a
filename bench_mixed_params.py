"""A fitted conditional Gaussian network (include/dvs_mixed_params.h) on 8 + 8 and 24 + 24 variables (factors +
real columns): ``cg_sample``, ``cg_log_likelihood`` and ``cg_predict`` on a class (mode 2) at 10^6 rows, and
``cg_cross_validate(folds=10)`` at 5000 rows, each beside the same computation written in torch ops on the device (gathers of the
per-configuration parameters, one pass per variable), timed alternately in the same process.  Seeded networks.  The two must
agree before either number counts, or the run stops: the log-likelihoods to 1e-12 relative, the posteriors to 1e-9 absolute and
the predictions on every row whose two best posteriors are 1e-9 apart, the cross-validation as bytes with its per-fold
composition; the sampler draws other normals than torch.randn, so there the implied deviates (x - mu) / sd of the kernel's rows
must have mean 0 and variance 1 within 5 standard errors.  Nothing is gated on speed.
Writes profiles/mixed_params_bench.json.

    python bench_mixed_params.py [--rows 1000000] [--cv-rows 5000] [--repeats 5]
"""
import argparse
import json
import os

import numpy as np
import torch

from bench_gaussian_params import alternating_s
from dags_vae_search_amd import (FittedCGBN, MixedEvaluator, cg_cross_validate, cg_fit, cg_log_likelihood, cg_predict, cg_sample, cv_folds,
                                 infer)
from dags_vae_search_amd.mixed import _spread_rows, _sub_rows
from dags_vae_search_amd.params import log_likelihood, sample

HERE = os.path.dirname(os.path.abspath(__file__))
LOGLIK_AGREEMENT = 1e-12     # two fp64 sums of S n terms of like sign in different orders: a thousand times (log2(S n) + n + 8) u
POSTERIOR_AGREEMENT = 1e-9   # a softmax of sums of at most 24 terms of magnitude ~10: a million times 24 * 10 * u


def network(nd, nc, seed=0):
    """nd factors (2 .. 4 levels, up to two factors as parents) then nc reals in a random order (up to two factors and three
    reals as parents), the class 0 a parent of every second real; seeded parameters and tables"""
    rng = np.random.default_rng(9000 + nd + nc + seed)
    n = nd + nc
    kinds = rng.permutation([1] * nd + [0] * nc)
    kinds[0] = 1 if kinds[0] else kinds[0]
    card = [int(rng.integers(2, 5)) if k else 0 for k in kinds]
    if not card[0]:                                          # variable 0 is the class
        j = next(v for v in range(n) if card[v])
        card[0], card[j] = card[j], 0
    order = [0] + [int(v) for v in rng.permutation(np.arange(1, n))]
    parents = [0] * n
    for k, v in enumerate(order):
        ds, cs = [u for u in order[:k] if card[u]], [u for u in order[:k] if not card[u]]
        for u in rng.choice(ds, size=min(len(ds), int(rng.integers(0, 3))), replace=False):
            parents[v] |= 1 << int(u)
        if not card[v]:
            for u in rng.choice(cs, size=min(len(cs), int(rng.integers(0, 4))), replace=False) if cs else []:
                parents[v] |= 1 << int(u)
            if k % 2:
                parents[v] |= 1
    coef, icpt, sd, tables = [None] * n, [None] * n, [None] * n, [None] * n
    for v in range(n):
        q = int(np.prod([card[u] for u in range(n) if (parents[v] >> u) & 1 and card[u]], dtype=np.int64))
        if card[v]:
            t = rng.uniform(0.2, 1.0, (q, card[v]))
            tables[v] = t / t.sum(1, keepdims=True)
        else:
            coef[v] = np.zeros((q, n))
            for u in range(n):
                if (parents[v] >> u) & 1 and not card[u]:
                    coef[v][:, u] = rng.uniform(0.3, 0.9, q) * rng.choice([-1.0, 1.0], q)
            icpt[v], sd[v] = rng.uniform(-2.0, 2.0, q), rng.uniform(0.5, 2.0, q)
    return FittedCGBN.from_parameters(parents, card, coef, icpt, sd, tables)


class TorchNet:
    """what the torch compositions read: per real variable its factor parents with their radix multipliers, its real parents and
    its first cell; per factor its table's offset and its parents' multipliers"""

    def __init__(self, f):
        self.f, self.n = f, f.n_vars
        self.card, self.offset, self.coef, self.icpt, self.sd = f.flat()
        host = [int(m) for m in f.parents.cpu().tolist()]
        off = [int(o) for o in self.offset.cpu().tolist()]
        self.col = {v: j for j, v in enumerate(f.continuous_vars)}
        self.real, self.order = {}, []
        for v in f.continuous_vars:
            mul, ds = 1, []
            for u in range(self.n):
                if (host[v] >> u) & 1 and f.card[u]:
                    ds.append((u, mul))
                    mul *= f.card[u]
            self.real[v] = (off[v], ds, [u for u in range(self.n) if (host[v] >> u) & 1 and not f.card[u]])
        placed = 0
        while len(self.order) < self.n:
            v = next(v for v in range(self.n) if not (placed >> v) & 1 and not host[v] & ~(1 << v) & ~placed)
            self.order.append(v)
            placed |= 1 << v
        d = f.discrete
        self.factor = {}
        for j, v in enumerate(f.discrete_vars):
            mul, ds = 1, []
            for i, u in enumerate(f.discrete_vars):
                if (int(d.parents_host[0, j]) >> i) & 1:
                    ds.append((u, mul))
                    mul *= f.card[u]
            self.factor[v] = (d.offsets_host[j], ds)
        self.log_cpt = torch.log(d.cpt)

    def levels(self, packed):
        return [((packed[:, v // 16] >> (4 * (v % 16))) & 15) for v in range(self.n)]

    def cell(self, v, lev, override=None):
        base, ds, _ = self.real[v]
        z = torch.full_like(lev[0], base)
        for u, mul in ds:
            z = z + (lev[u] if override is None or u != override[0] else override[1]) * mul
        return z

    def mu(self, v, cell, x):
        mu = self.icpt[cell]
        for u in self.real[v][2]:
            mu = mu + self.coef[cell, u] * x[:, self.col[u]]
        return mu

    def sample(self, packed, seed):
        lev = self.levels(packed)
        x = torch.empty(packed.shape[0], len(self.col), dtype=torch.float64, device=packed.device)
        gen = torch.Generator(device=packed.device).manual_seed(seed)
        for v in self.order:
            if v in self.real:
                cell = self.cell(v, lev)
                x[:, self.col[v]] = self.mu(v, cell, x) + self.sd[cell] * torch.randn(packed.shape[0], dtype=torch.float64, device=packed.device,
                                                                                      generator=gen)
        return x

    def real_term(self, v, cell, x):
        e = (x[:, self.col[v]] - self.mu(v, cell, x)) / self.sd[cell]
        return torch.log(self.sd[cell]) + 0.9189385332046727 + 0.5 * (e * e)

    def loglik(self, packed, x):
        lev = self.levels(packed)
        total = torch.zeros(packed.shape[0], dtype=torch.float64, device=packed.device)
        for v, (base, ds) in self.factor.items():
            cfg = torch.zeros_like(lev[0])
            for u, mul in ds:
                cfg = cfg + lev[u] * mul
            total = total + self.log_cpt[base + cfg * self.f.card[v] + lev[v]]
        for v in self.real:
            total = total - self.real_term(v, self.cell(v, lev), x)
        return total.sum()

    def classify(self, t, packed, x, prior):
        lev = self.levels(packed)
        a = torch.log(prior)
        for v, (_, ds, _) in self.real.items():
            if any(u == t for u, _ in ds):
                a = a - torch.stack([self.real_term(v, self.cell(v, lev, (t, k)), x) for k in range(self.f.card[t])], dim=1)
        post = torch.softmax(a, dim=1)
        return post.argmax(1).to(torch.uint8), post


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--cv-rows", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 24])
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "mixed_params_bench.json"))
    args = ap.parse_args()
    S, Sc = args.rows, args.cv_rows
    res = {"device": torch.cuda.get_device_name(0), "rows": S, "cv_rows": Sc, "repeats": args.repeats,
           "timing": "host clock around windows of back-to-back calls (about 50 ms each, sized from a probe call) that end in a "
                     "device synchronise; the median window of the repeats divided by its calls, after one warm-up call of every "
                     "shape; a call and its torch baseline take their windows alternately",
           "sample": [], "loglik": [], "predict_class": [], "cross_validate": []}
    for half in args.sizes:
        f = network(half, half)
        tn, n = TorchNet(f), 2 * half
        # ---- sampling: both sides draw the levels with sample() on the discrete sub-network, then fill the real columns
        packed, x = cg_sample(f, S, seed=1)
        lev = tn.levels(packed)
        for v in f.continuous_vars:
            cell = tn.cell(v, lev)
            z = (x[:, tn.col[v]] - tn.mu(v, cell, x)) / tn.sd[cell]
            if not (abs(float(z.mean())) < 5 / S ** 0.5 and abs(float((z * z).mean()) - 1) < 5 * (2 / S) ** 0.5):
                raise SystemExit(f"cg_sample: the implied deviates of variable {v} at {half} + {half} are not standard normal")

        def torch_sample():
            sub = sample(f.discrete, S, seed=1)
            return tn.sample(_spread_rows(sub, f.discrete_vars, n), 1)
        tk, tt = alternating_s(lambda: cg_sample(f, S, seed=1), torch_sample, args.repeats)
        row = {"factors": half, "reals": half, "rows": S, "ms": round(tk * 1e3, 4), "torch_ms": round(tt * 1e3, 4), "rows_per_s": round(S / tk),
               "torch_over_call": round(tt / tk, 3)}
        res["sample"].append(row)
        print("sample", row, flush=True)
        # ---- the log-likelihood of those rows
        a, b = cg_log_likelihood(f, (packed, x)), tn.loglik(packed, x)
        rel = abs(float(a) - float(b)) / abs(float(b))
        if not rel < LOGLIK_AGREEMENT:
            raise SystemExit(f"cg_log_likelihood and the torch composition disagree at {half} + {half}: relative difference {rel}")
        tk, tt = alternating_s(lambda: cg_log_likelihood(f, (packed, x)), lambda: tn.loglik(packed, x), args.repeats)
        row = {"factors": half, "reals": half, "rows": S, "ms": round(tk * 1e3, 4), "torch_ms": round(tt * 1e3, 4), "rows_per_s": round(S / tk),
               "torch_over_call": round(tt / tk, 3), "relative_difference": rel}
        res["loglik"].append(row)
        print("loglik", row, flush=True)
        # ---- the class (variable 0) given everything else: both sides take the discrete blanket's posterior from infer.predict
        sub = _sub_rows(packed, f.discrete_vars)

        def torch_classify():
            _, prior = infer.predict(f.discrete, 0, sub, method="exact", prob=True)
            return tn.classify(0, packed, x, prior)
        (pa, qa), (pb, qb) = cg_predict(f, 0, (packed, x), method="exact", prob=True), torch_classify()
        diff = float((qa - qb).abs().max())
        top = torch.topk(qb, 2, dim=1).values
        clear = (top[:, 0] - top[:, 1]) > POSTERIOR_AGREEMENT
        if not (diff < POSTERIOR_AGREEMENT and bool((pa[clear] == pb[clear]).all())):
            raise SystemExit(f"cg_predict and the torch composition disagree at {half} + {half}: largest posterior difference {diff}")
        tk, tt = alternating_s(lambda: cg_predict(f, 0, (packed, x), method="exact", prob=True), torch_classify, args.repeats)
        row = {"factors": half, "reals": half, "rows": S, "levels": f.card[0], "real_children": sum(1 for v in tn.real if any(u == 0 for u, _ in tn.real[v][1])),
               "ms": round(tk * 1e3, 4), "torch_ms": round(tt * 1e3, 4), "rows_per_s": round(S / tk), "torch_over_call": round(tt / tk, 3),
               "largest_posterior_difference": diff}
        res["predict_class"].append(row)
        print("predict_class", row, flush=True)
        # ---- cross-validation at cv_rows: one call against its per-fold composition
        pc, xc = packed[:Sc].contiguous(), x[:Sc].contiguous()
        ev = MixedEvaluator.from_device(f"syn{half}", "bic-cg", pc, xc, f.card)

        def composition():
            parts = [torch.from_numpy(p).cuda() for p in cv_folds(Sc, 10, 0)]
            total = None
            for i, part in enumerate(parts):
                rest = torch.cat([p for g, p in enumerate(parts) if g != i])
                fit = cg_fit(MixedEvaluator.from_device("rest", "bic-cg", pc[rest], xc[rest], f.card), f.parents)
                ll = cg_log_likelihood(fit, (pc[part].contiguous(), xc[part].contiguous()))
                total = ll if total is None else total + ll
            return -total / torch.full_like(total, float(Sc))
        try:
            same = cg_cross_validate(ev, f.parents).cpu().numpy().tobytes() == composition().cpu().numpy().tobytes()
            tc, tp = alternating_s(lambda: cg_cross_validate(ev, f.parents), composition, args.repeats)
            row = {"factors": half, "reals": half, "rows": Sc, "folds": 10, "ms": round(tc * 1e3, 3), "composition_ms": round(tp * 1e3, 3),
                   "composition_over_call": round(tp / tc, 3), "equal_bytes": bool(same), "loss": float(cg_cross_validate(ev, f.parents))}
        except ValueError as err:                            # cg_fit refuses a fold with a configuration of 1 .. p + 1 rows
            row = {"factors": half, "reals": half, "rows": Sc, "folds": 10, "refused": str(err)[:200]}
        res["cross_validate"].append(row)
        print("cross_validate", row, flush=True)
    res["not_measured"] = ["kernel times by rocprofv3 (only end-to-end call times are taken; each call includes its discrete half and its "
                           "allocations)", "cg_predict on a real target (modes 0 and 1)", "q = 4096 and variables with 20 real parents",
                           "row counts other than --rows and --cv-rows", "a torch baseline of cross-validation other than its own per-fold composition"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
