#!/usr/bin/env python3
"""bench.py — DAGs/sec of the PACE-VAE train step (BASELINE.json metric) on N MI355X of one node.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" = one full train step on one batch of synthetic DAGs whose reference-layout dense features are already
resident in HBM: dvs_pack_features -> forward -> backward -> (RCCL SUM all-reduce of the flat gradient when N > 1)
-> fused clip_grad_norm_(1.0) + Adam(lr 1e-4), in train mode with dropout 0.15 — i.e. train_batch() of
experiments/03_synthetic_12/main.py:95-118 including its loss.item() host read.  Workload: BASELINE configs[1]/metric
shape: synthetic n=12, card=12, batch 4096 per GPU (weak scaling: global batch = 4096 * N, one gradient all-reduce).
With N > 1 and --full the same run also times the strong-scaling reading of the metric (GLOBAL batch 4096,
4096 / N DAGs per GPU) and reports it as the "strong" object of the same line; `--scaling strong` makes that the headline.

Prints ONE JSON line (rank 0).  A plain run sets up, warms up, times the K steps and prints the headline (`value`,
`ms_per_step`, ...); `--dump-outputs DIR` first writes what the last timed step returned (see dump_outputs).  `--full`
adds what the headline does not need, measured after the timed region: "kernels" and "roofline" for the dominant
kernel (per-kernel durations measured with HIP events on the launch stream inside libdvs_hip.so, in separate untimed
steps; `frac` on SURVEY §8d's algorithmic FLOPs, i.e. WITHOUT the backward's recompute, `hfu` with it), "hbm_roofline",
the other scaling reading at N > 1, and "cpu_baseline" (the oracle = CPU port of the reference step, timed on the host's
cores on a bounded sample; rank 0 at N=1 only, `--no-cpu-baseline` drops it).
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

N_VERT, CARD = 12, 12            # --workload changes these (the driver's default run is the BASELINE metric shape)
WORKLOADS = {   # name: (n, card, default per-GPU batch, edge-density limit, description)
    "n12": (12, 12, 4096, 0.4, "synthetic_v12 DAGs (n=12, card=12, N=15 tokens)"),
    "asia": (8, 8, 4096, 0.4, "asia-shaped synthetic DAGs (n=8, card=8, N=11 tokens)"),
    "sachs": (11, 11, 8192, 0.4, "sachs-shaped synthetic DAGs (n=11, card=11, N=14 tokens)"),
    "alarm": (37, 37, 2048, 0.2, "alarm-size synthetic DAGs (n=37, card=37, N=40 tokens, tiled wide path)"),
}
DENSITY = 0.4
PEAK_F32_MFMA_TFLOPS = 157.3      # MI355X_MICROARCH.md: dense fp32 matrix/vector peak
PEAK_HBM_GBS = 8000.0


def algo_flops_per_dag(N: int, C: int):
    """FLOPs per DAG of each kernel (multiply-add = 2), counted on the TRUE token count N (not the 16-token tile) and on
    the reference's formulation (the edge head in its factored U_i+V_j form).  Returns
    (algorithmic, executed): `executed` adds the backward's recompute of forward quantities to the algorithmic count.
    proj = one N x 64 x 64 projection; core = QK^T + PV of all 8 heads."""
    proj = 2.0 * N * 64 * 64
    core = 2.0 * 2 * N * N * 64
    pairs = (N - 1) * (N - 2) / 2
    node = 2.0 * N * (64 * 32 + 32 * C)
    edge = 2 * proj + pairs * 64 * 3
    emb = 2.0 * N * 64 * 32 + N * 64 * 3
    latent_f = 2.0 * N * 64 * 64 + 2.0 * 32 * N * 64
    f = {
        "k_embed_fwd": emb, "k_attn_fwd": 4 * proj + core, "k_ffn_fwd": 2 * proj, "k_latent_fwd": latent_f,
        "k_loss_fwd": node + edge,
        # backward kernels: recompute (1x forward) + gradients (2x forward) of the ops they own
        "k_loss_bwd": 3 * (node + edge), "k_ffn_bwd": 3 * 2 * proj,
        "k_attn_bwd": (3 * proj + core) + 2 * (proj + core) + proj,     # recompute q,k,v,P ; dWo,dO + core bwd ; O
        "k_proj_bwd<3>": 2 * 3 * proj, "k_proj_bwd<2>": 2 * 2 * proj, "k_proj_bwd<1>": 2 * proj,
        "k_latent_bwd": 2.0 * 32 * N * 64 + 2.0 * N * 64 * 64, "k_fc_dw": latent_f, "k_embed_bwd": 2 * emb,
    }
    # SURVEY.md §8d's algorithmic count (whole step = 3 x forward, so a backward kernel = 2 x the forward ops it owns):
    # what the hardware additionally re-computes (q, k, v, probabilities, hidden activations) is NOT algorithmic work
    a = dict(f)
    a.update({"k_loss_bwd": 2 * (node + edge), "k_ffn_bwd": 2 * 2 * proj, "k_attn_bwd": 2 * (proj + core)})

    # the wide attention backward reads q, k, v back from the forward (round 3): it recomputes the probabilities only
    f["k_attn_bwd_w"] = core + 2 * (proj + core)
    a["k_attn_bwd_w"] = a["k_attn_bwd"]
    # chained launches (one-tile path): the sum over the sublayers one launch walks.  The decoder's 18 backward phases
    # go out as two launches of 9, so its per-launch figure is half the decoder total.
    for t in (f, a):
        t["k_fwd_stack<0>"] = 3 * (t["k_attn_fwd"] + t["k_ffn_fwd"])
        t["k_fwd_stack<1>"] = 3 * (2 * t["k_attn_fwd"] + t["k_ffn_fwd"])
        t["k_bwd_stack<0>"] = 3 * (t["k_ffn_bwd"] + 2 * t["k_attn_bwd"] + t["k_proj_bwd<1>"] + t["k_proj_bwd<2>"]
                                   + t["k_proj_bwd<3>"]) / 2
        t["k_bwd_stack<1>"] = 3 * (t["k_ffn_bwd"] + t["k_attn_bwd"] + t["k_proj_bwd<3>"])
    return a, f


STACK_PHASES = {   # what one launch of a chained kernel walks (csrc/k_forward.hip, k_backward.hip)
    "k_fwd_stack<0>": "encoder forward: 3 x (attention, FFN)",
    "k_fwd_stack<1>": "decoder forward: 3 x (self-attention, cross-attention, FFN)",
    "k_bwd_stack<0>": "decoder backward, its 15 phases in two launches (9 + 6; the figure is the per-launch average): 3 x (FFN, "
                      "cross-attention core, q | k,v projections as one split phase, self-attention core, q/k/v projections)",
    "k_bwd_stack<1>": "encoder backward: 3 x (FFN, attention core, q/k/v projections)",
}


def bytes_per_dag(N: int, C: int, P: int, B_local: int) -> float:
    """SURVEY.md §8d algorithmic bytes per DAG: consumed reference-layout features + amortised parameter traffic."""
    return N * C * 4 + 2 * N * N * 4 + 8 * N * N + 9.0 * P * 4 / B_local


PROFILE_TAG = "r03"


def pmc_profile(workload: str, batch: int, kind: str):
    """Path (relative to the repo) of the committed rocprofv3 --pmc summary for this workload, or None.  Counters cannot
    be collected from inside the timed process: these files are BUILDER-SIDE data (tools/collect_profiles.sh, run on an
    MI355X of the same pool), replayed into the line and labelled with their source."""
    for tag in (PROFILE_TAG, "r02", "r01"):
        for name in (f"{tag}_pmc_{kind}_{workload}_b{batch}.csv", f"{tag}_pmc_{kind}.csv" if workload == "n12" and batch == 4096 else None):
            if name and os.path.exists(os.path.join(REPO, "profiles", name)):
                return os.path.join("profiles", name)
    return None


def pmc_traffic(kernel: str, workload: str, batch: int):
    """(HBM bytes per launch of `kernel`, HBM bytes per step, source file) from the committed FETCH_SIZE / WRITE_SIZE
    passes (FETCH_SIZE doubled per MI355X_MICROARCH.md §HBM); (None, None, None) without a profile for this config.
    File: kernel,launches_per_step,fetch_KB_corrected,write_KB,bytes_per_DAG (+ a TOTAL_PER_STEP row); round-1 files have
    no launches column and give no per-step total."""
    path = pmc_profile(workload, batch, "hbm")
    if path is None:
        return None, None, None
    per_launch, per_step = None, None
    for line in open(os.path.join(REPO, path)):
        parts = line.strip().split(",")
        try:
            per_dag = float(parts[-1])
        except (ValueError, IndexError):
            continue
        if parts[0] == "TOTAL_PER_STEP":
            per_step = per_dag * batch
        elif parts[0].replace("void ", "") == kernel:
            per_launch = per_dag * batch          # bytes per DAG and launch x DAGs per launch
    return per_launch, per_step, path


def pmc_mfma_busy(kernel: str, workload: str, batch: int):
    """(matrix-pipe busy share, waves-parked share, source) of `kernel` from the committed SQ counter pass's derived table
    (tools/rocprof_summary.py sq-derived), or (None, None, None)."""
    path = pmc_profile(workload, batch, "sqd")
    if path is None:
        return None, None, None
    try:
        import csv
        for r in csv.DictReader(open(os.path.join(REPO, path))):
            if r["kernel"].replace("void ", "") == kernel:
                return float(r["mfma_pipe_busy"]), float(r["wait_any_frac"]), path
    except (OSError, ValueError, KeyError):
        pass
    return None, None, path


def make_batch(batch: int, seed: int, device):
    from dags_vae_search_amd import prepare_features
    from dags_vae_search_amd.synthetic import synthetic_dags
    graphs = synthetic_dags(N_VERT, CARD, batch, seed=seed, density_limit=DENSITY)
    feats = prepare_features(graphs, N_VERT + 3, CARD + 3)
    dev_feats = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in feats.items()}
    return graphs, feats, dev_feats


def host_cores() -> int:
    """CPU cores this process may really use: affinity mask capped by the cgroup CPU quota (the GPU box gives a
    16-core share of a much larger host; os.cpu_count() there reports the whole host)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return max(1, n)


def log(msg):
    print(f"[bench +{time.perf_counter() - T0:7.1f}s] {msg}", file=sys.stderr, flush=True)


T0 = time.perf_counter()


def cpu_baseline(graphs, feats, steps: int = 5, warmup: int = 3):
    """Reference CPU path = oracle port of train_batch (train mode, dropout 0.15, Adam), all usable host cores;
    BASELINE.md §3: 3 warm-up + 5 timed steps on the same batch."""
    from oracle import pace_oracle as po
    cores = min(host_cores(), 32)
    torch.set_num_threads(cores)
    log(f"cpu_baseline: {cores} threads (os.cpu_count()={os.cpu_count()})")
    cfg = po.PaceConfig(n=N_VERT, card=CARD)
    torch.manual_seed(42)
    tr = po.OracleTrainer(cfg, po.init_params(cfg, seed=42))
    f = {k: v for k, v in feats.items()}
    for _ in range(warmup):
        tr.step(f)
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(f)
    dt = (time.perf_counter() - t0) / steps
    B = len(graphs)
    return {"value": B / dt, "unit": "DAGs/s", "cores": cores, "kind": "port",
            "sample": f"{steps} timed train steps (+{warmup} warm-up) of the oracle on the same n={N_VERT} card={CARD} "
                      f"B={B} batch, torch CPU fp32, {cores} threads", "ms_per_step": dt * 1e3}


def dump_outputs(out_dir: str, last, model):
    """What a caller of the timed path holds after its last step: train_batch's (loss, recon, kld) and the model it
    updated, i.e. every parameter and its .grad, flattened and concatenated in model.parameters() order (independent of
    the padding of the device's flat buffer).  Inputs, initial weights and dropout streams are seeded, so the same
    arguments give the same inputs on every run."""
    import numpy as np
    loss_value, recon, kld = last
    params = list(model.parameters())
    arrays = {"loss": np.array([loss_value, float(recon), float(kld)], dtype=np.float64),     # [total, recon, kld]
              "params": torch.cat([p.detach().reshape(-1) for p in params]).float().cpu().numpy(),
              "grads": torch.cat([p.grad.detach().reshape(-1) for p in params]).float().cpu().numpy()}
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return sorted(arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=None,
                    help="DAGs per GPU under weak scaling, GLOBAL batch under strong scaling (default: the workload's)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="n12",
                    help="n12 = the BASELINE metric shape (default); the others are the remaining BASELINE configs")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak",
                    help="weak: --batch DAGs per GPU (global = batch * N); strong: --batch DAGs in total (SURVEY §8d's "
                         "reading of the metric: global 4096, 4096 / N per GPU).  With --full and N > 1 the other one is "
                         "timed too and reported as a secondary object of the same line")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave out the CPU baseline")
    ap.add_argument("--force-dist", action="store_true",
                    help="take the RCCL code path even with one rank (checks init / all-reduce plumbing on a 1-GPU box)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also measure per-kernel durations and the roofline, the other scaling "
                         "reading (N > 1) and the CPU baseline (N = 1); a plain run measures the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (loss scalars, parameters, gradient) as DIR/<name>.npy")
    args = ap.parse_args()
    global N_VERT, CARD, DENSITY
    N_VERT, CARD, default_batch, DENSITY, workload_desc = WORKLOADS[args.workload]
    if args.batch is None:
        args.batch = default_batch

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        # no re-exec and no GPU call before this point: the launcher hop must come before anything touches the GPU
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE is {world}: for N > 1 launch one rank per GPU with\n"
              f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node {args.gpus} --master-addr 127.0.0.1 "
              f"--master-port 29533 bench.py --gpus {args.gpus} ...", file=sys.stderr)
        sys.exit(2)
    if args.batch % world:
        print(f"bench.py: --batch {args.batch} is not divisible by {world} ranks", file=sys.stderr)
        sys.exit(2)

    # libraries (RCCL's version banner, ...) write to fd 1: keep stdout clean for the ONE JSON line
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)

    distributed = world > 1 or args.force_dist
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    from dags_vae_search_amd import PaceVaeV3, optim as dopt
    from dags_vae_search_amd import _lib as dl
    from dags_vae_search_amd.train import train_batch

    torch.set_num_threads(min(host_cores(), 16))
    group = True if distributed else None

    def sync():
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()

    def timed_run(local_batch: int, steps: int, warmup: int):
        """One model + one resident batch of `local_batch` DAGs per rank; W untimed + K timed train steps bracketed by
        barrier + synchronize, MAX over ranks.  Returns (seconds, what the last step returned, model, step fn, graphs,
        host features)."""
        torch.manual_seed(42)      # experiments/03_synthetic_12/main.py:122-124: same initial weights on every rank
        model = PaceVaeV3(max_num_vertices=N_VERT, vertex_label_cardinality=CARD, vertices_embedding_size=32,
                          num_heads=8, num_layers=3, ff_hidden_size=64, latent_layer_size=32, fc_hidden=32,
                          dropout=0.15).to(device)
        model.seed(42)
        model.dag_offset = rank * local_batch
        opt = dopt.Adam(model.parameters(), lr=1e-4).attach(model)
        graphs, feats, dev_feats = make_batch(local_batch, seed=42 + rank, device=device)

        def step():
            return train_batch(dev_feats, model, opt, max_grad_norm=1.0, group=group)
        for _ in range(warmup):
            step()
        sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            last = step()
        sync()
        dt = time.perf_counter() - t0
        if distributed:
            t = torch.tensor([dt], device=device, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, last, model, step, graphs, feats

    # headline region
    local_batch = args.batch if args.scaling == "weak" else args.batch // world
    global_batch = local_batch * world
    log(f"{args.scaling} scaling: {local_batch} DAGs per GPU, global batch {global_batch}; warm-up + timed region")
    dt, last, model, step, graphs, feats = timed_run(local_batch, args.steps, args.warmup)
    loss_value = last[0]
    ms_per_step = dt / args.steps * 1e3
    value = global_batch * args.steps / dt
    log(f"timed region done: {ms_per_step:.3f} ms/step")
    if args.dump_outputs and rank == 0:
        names = dump_outputs(args.dump_outputs, last, model)
        log(f"outputs of the last timed step written: {', '.join(names)}")
    lib = dl.load()

    # ---- --full: per-kernel durations (HIP events on the launch stream), separate untimed steps --------------------------
    if args.full:
        prof_steps = 3
        lib.dvs_profile_enable(1)
        for _ in range(prof_steps):
            step()
        torch.cuda.synchronize()
        prof = dl.profile_collect(lib)
        lib.dvs_profile_enable(0)
        sync()

    # ---- --full: the other scaling mode, same process, N > 1 only (at N = 1 they coincide) -------------------------------
    other = None
    if args.full and world > 1:
        o_mode = "strong" if args.scaling == "weak" else "weak"
        o_local = args.batch // world if o_mode == "strong" else args.batch
        del step
        o_dt, _, _, _, _, _ = timed_run(o_local, args.steps, args.warmup)
        other = {"scaling": o_mode, "value": o_local * world * args.steps / o_dt, "unit": "DAGs/s",
                 "per_gpu_batch": o_local, "global_batch": o_local * world, "ms_per_step": o_dt / args.steps * 1e3,
                 "note": "the other reading of the metric, timed in the same process right after the headline region "
                         "(same model shape, fresh model and batch)"}
        log(f"{o_mode} scaling: {other['ms_per_step']:.3f} ms/step at {o_local} DAGs per GPU")

    if rank == 0:
        N, C = N_VERT + 3, CARD + 3
        # Which reading of BASELINE.json's metric the headline is (the line always says; with --full and N > 1 the OTHER reading
        # is timed in the same process and attached under its own key, so one launch per N gives both curves):
        #   weak   — 4096 DAGs PER GPU (global batch 4096 N): the reading this file has reported since round 1 and the one
        #            the driver's weak-scaling efficiency is computed on; one gradient all-reduce per step either way.
        #   strong — SURVEY.md 8d's reading: GLOBAL batch 4096, 4096 / N DAGs per GPU.  Below 1024 DAGs per GPU a step is
        #            bound by the latency of ONE DAG through the 42 phases, so this curve flattens by design.
        reading = ("strong scaling: GLOBAL batch fixed (SURVEY.md 8d), per-GPU batch = global / N" if args.scaling == "strong"
                   else "weak scaling: per-GPU batch fixed, global batch = per-GPU x N")
        out = {
            "metric": f"DAGs/sec VAE+predictor train step, n={N_VERT} batch {global_batch if args.scaling == 'strong' else local_batch}"
                      f"{'' if args.scaling == 'strong' else ' per GPU'}, at {world} MI355X",
            "metric_reading": reading,
            "value": value, "unit": "DAGs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32 (fwd bf16x6, bwd bf16x3 split products, fp32 accumulate)", "data": "synthetic",
            "config": {"workload": workload_desc + ", PACE-VAE train step: pack + fwd + bwd"
                                   " + clip_grad_norm_(1.0) + Adam(1e-4), train mode dropout 0.15",
                       "per_gpu_batch": local_batch, "global_batch": global_batch,
                       # dvs_api.hip: waves_per_wg — the narrow 4-wave mapping below 4 x #CU DAGs on the one-tile path
                       "waves_per_workgroup": 4 if (N <= 16 and C <= 16 and local_batch <= 4 * lib.dvs_device_cus()
                                                    and os.environ.get("DVS_WAVES_PER_WG") != "8") else 8,
                       "parallelism": f"dp{world}" if world > 1 else "single",
                       "last_loss_per_dag": loss_value / global_batch},
        }
        if args.full:
            P = sum(p.numel() for p in model.parameters())
            algo, executed = algo_flops_per_dag(N, C)
            kern = {k: {"launches_per_step": c // prof_steps, "avg_us": 1e3 * ms / c, "ms_per_step": ms / prof_steps}
                    for k, (c, ms) in prof.items()}
            dom = max(kern, key=lambda k: kern[k]["ms_per_step"])
            dom_key = dom if dom in executed else (dom[:-2] if dom.endswith("_w") else dom)      # wide-path kernels: same algorithmic work
            per_launch_s = kern[dom]["avg_us"] * 1e-6
            ach = algo.get(dom_key, 0.0) * local_batch / per_launch_s / 1e12
            hfu = executed.get(dom_key, 0.0) * local_batch / per_launch_s / 1e12
            step_flops = 3e6 * {8: 5.71, 11: 7.74, 12: 8.46, 37: 34.0}[N_VERT]      # 3 x forward MFLOP per DAG
            bpd = bytes_per_dag(N, C, P, local_batch)
            per_gpu_rate = value / world
            traffic, traffic_step, traffic_src = pmc_traffic(dom, args.workload, local_batch)
            busy, wait, sq_src = pmc_mfma_busy(dom, args.workload, local_batch)
            roofline = {
                "bound": "mfma", "kernel": dom, "achieved": ach, "peak": PEAK_F32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": ach / PEAK_F32_MFMA_TFLOPS,
                "frac_note": "algorithmic FLOPs of SURVEY.md 8d (backward = 2 x forward of the ops the launch owns, recompute NOT "
                             "counted) / HIP-event launch duration / fp32 matrix peak; arithmetic is delivered at fp32 accuracy, most "
                             "of it on the bf16 pipe with split operands, so this is delivered arithmetic, not pipe utilisation",
                "hfu": hfu / PEAK_F32_MFMA_TFLOPS, "hfu_note": "same with the backward's recompute of forward quantities counted",
                "traffic": traffic, "traffic_source": traffic_src,
                "traffic_note": "HBM bytes per launch from rocprofv3 --pmc FETCH_SIZE (x2, gfx950) + WRITE_SIZE passes collected by "
                                "the builder (tools/collect_profiles.sh) and replayed from the committed file; not measured in this run",
                "avg_launch_us": kern[dom]["avg_us"], "launches_per_step": kern[dom]["launches_per_step"],
                "algorithmic_flops_per_dag": algo.get(dom_key, 0.0), "executed_flops_per_dag": executed.get(dom_key, 0.0),
                **({"phases": STACK_PHASES[dom_key]} if dom_key in STACK_PHASES else {}),
                **({"mfma_pipe_busy": busy, "waves_waiting": wait, "counters_source": sq_src} if sq_src else {}),
                "whole_step": {"tflops": per_gpu_rate * step_flops / 1e12,
                               "frac_f32_mfma_peak": per_gpu_rate * step_flops / 1e12 / PEAK_F32_MFMA_TFLOPS,
                               "hbm_algorithmic_GBs": per_gpu_rate * bpd / 1e9,
                               "gpu_kernel_ms_per_step": sum(k["ms_per_step"] for k in kern.values())}}
            # the north star's contract figure, lifted to the top level: achieved fraction of the HBM roofline on ALGORITHMIC bytes
            # (bytes_per_DAG x DAGs/s / 8 TB/s), and how much more than that the counters say really moves
            hbm = {"algorithmic_bytes_per_dag": bpd, "algorithmic_GBs_per_gpu": per_gpu_rate * bpd / 1e9,
                   "frac_hbm_peak": per_gpu_rate * bpd / 1e9 / PEAK_HBM_GBS, "peak_GBs": PEAK_HBM_GBS}
            if traffic_step:
                hbm.update({"counter_bytes_per_step": traffic_step, "counter_GBs": traffic_step / (ms_per_step * 1e-3) / 1e9,
                            "counter_frac_hbm_peak": traffic_step / (ms_per_step * 1e-3) / 1e9 / PEAK_HBM_GBS,
                            "traffic_over_algorithmic": traffic_step / (bpd * local_batch), "counter_source": traffic_src})
            out.update({
                "frac_hbm_peak": hbm["frac_hbm_peak"],
                "hbm_roofline": hbm,
                "roofline": roofline,
                "kernels": {k: round(v["ms_per_step"], 4) for k, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms_per_step"])},
            })
            if other is not None:
                out[other["scaling"]] = other
            if world == 1 and not args.no_cpu_baseline:
                out["cpu_baseline"] = cpu_baseline(graphs, feats)
                out["speedup_vs_cpu_baseline"] = value / out["cpu_baseline"]["value"]
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(out), flush=True)
        os.dup2(2, 1)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
