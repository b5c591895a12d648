#!/usr/bin/env python
"""Throughput of the SA-VQA model_v=3 training step on MI355X (BASELINE.json metric).

A step = forward + label-smoothed loss (+ MIL-NCE) + backward + Adam over one synthetic
batch already resident in HBM (cfg 2: fp32, 256 samples/GPU, 36 regions x 2048-d,
14-token questions, 59 scene-graph nodes, d=512, 8 heads, 6+6 layers per stack, training
dropout 0.5 = the reference's default, main_itp_ddp_tar_super_node.py:466, submit.py:98).
N GPUs = one process per GPU (torch.distributed.run), weak scaling, RCCL all-reduce of
the live gradients streamed out of the backward (savqa_amd.ddp).

A plain run sets up, warms up, times --steps steps and prints ONE JSON line (rank 0).
--dump-outputs DIR also writes what the last timed step computed as DIR/<name>.npy.
--full adds what takes runs of its own: the roofline of the dominant kernel (fp32 MFMA
GEMM, HIP-event timed, two probe steps), the per-kernel HBM report, the CPU oracle's
throughput on the host as cpu_baseline, and with N > 1 the collectives' timing over
--comm-steps diagnostic steps.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "QA-samples/sec training (model_v=3, 36 regions × 2048-d) at 1/2/4/8 MI355X"
FP32_MFMA_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 spec peak
BF16_MFMA_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: ~2.5 PF dense bf16 (no sparsity)
FP8_MFMA_PEAK_TFLOPS = 5000.0   # MI355X_MICROARCH.md: ~5 PF dense fp8 (no sparsity)
HBM_PEAK_GBS = 8000.0


def train_flops_per_sample(Tv=50, Ts=73, Lq=14, Nv=36, Ns=59, d=512, L=6, C=914, Hm=1024, K=5):
    """SURVEY.md 8(d) algorithmic count (fwd x 3)."""
    def stack(T):
        return (L * (22 * T * d * d + 4 * T * T * d) + L * (24 * d * d + 4 * T * d * d + 4 * T * d)
                + 2 * Lq * 300 * 2048 + 2 * T * 2048 * d)
    heads = 2 * (2 * d * d + d * C) + 4 * (d * d + d * C)
    mil = 2 * Ns * 300 * Hm + 4 * Nv * K * 300 * Hm + 2 * Nv * 2048 * Hm + 6 * Nv * K * Hm \
        + 2 * Ns * Hm * 2048
    return 3.0 * (stack(Tv) + stack(Ts) + heads + mil)


def _cpu_model():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


HBM_PEAK_GBS = 8000.0  # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md


def hbm_report(records, lp):
    """Per kernel family (LayerNorm, Adam, graph attention): launches per step, mean launch
    time (HIP events on the launch stream, stacks serialised), ALGORITHMIC bytes per launch and
    the rate they imply against the 8 TB/s HBM peak; attention also its MFMA rate."""
    torch.cuda.synchronize()
    agg = {}
    for tag, nb, fl, e0, e1 in records:
        a = agg.setdefault(tag, [0, 0.0, 0.0, 0.0])
        a[0] += 1
        a[1] += nb
        a[2] += fl
        a[3] += e0.elapsed_time(e1)
    out = {}
    for tag, (n, nb, fl, ms) in sorted(agg.items(), key=lambda kv: -kv[1][3]):
        gbs = nb / (ms * 1e-3) / 1e9
        r = {"launches_per_step": n // 2, "avg_us": round(ms / n * 1e3, 2),
             "bytes_per_launch": round(nb / n), "GB/s": round(gbs, 1),
             "hbm_frac": round(gbs / HBM_PEAK_GBS, 4)}
        if fl:
            tf = fl / (ms * 1e-3) / 1e12
            pk = BF16_MFMA_PEAK_TFLOPS if "bf16" in tag else FP32_MFMA_PEAK_TFLOPS
            r.update({"TFLOP/s": round(tf, 2), "mfma_frac": round(tf / pk, 4)})
        out[tag] = r
    return out


def _cgroup_cpus():
    """CPUs' worth of time the cgroup grants this process (cgroup v2 cpu.max / v1 cfs quota),
    or None when unlimited / unknown."""
    import math
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        if q != "max":
            return max(1, math.ceil(int(q) / int(p)))
        return None
    except (OSError, ValueError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us") as f:
            q = int(f.read())
        with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as f:
            p = int(f.read())
        return max(1, math.ceil(q / p)) if q > 0 else None
    except (OSError, ValueError):
        return None


def cpu_baseline(seconds=24.0, rate=0.5):
    """Time the CPU oracle (oracle/savqa_oracle.py, the parity checker) on the host, per
    SURVEY.md 8(d): forward+loss AND the full train step (fwd+loss+bwd+Adam), at the cfg-1
    shape B=4 and at the reference's per-GPU batch B=32, with torch.set_num_threads(every CPU
    the process may run on): the affinity mask (the survey's os.cpu_count()) capped by the
    cgroup's CPU quota -- the GPU box shows 256 CPUs but grants one GPU's job a 16-CPU share,
    and 256 threads on 16 CPUs' time made the oracle stall for minutes (a bench run was killed
    for silence). Both counts are reported. Bounded: ~seconds/4 per leg, progress on stderr.
    The headline `value` is the train step at B=32."""
    from oracle import hashfill
    from oracle import savqa_oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = _cgroup_cpus()
    threads = min(avail, quota) if quota else avail
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    torch.set_num_threads(threads)
    Nv, Lq, Ns, K = 36, 14, 59, 5
    P = hashfill.HashParams(requires_grad=True)
    state = {}

    def inputs(B):
        gen = torch.Generator().manual_seed(B)
        inp = {
            "vis_fea": torch.randn(B, Nv, 2048, generator=gen).clamp_min(0),
            "vis_mask": torch.ones(B, Nv, Nv, dtype=torch.int32),
            "q_ipt": torch.randint(0, 400000, (B, Lq), generator=gen),
            "q_mask": torch.ones(B, Lq, Lq, dtype=torch.int32),
            "q_graph": (torch.rand(B, Lq, Lq, generator=gen) < 0.2).int(),
            "macro_ipt": torch.randint(0, 400000, (B, Ns), generator=gen),
            "macro_mask": torch.ones(B, Ns, Ns, dtype=torch.int32),
            "macro_graph": (torch.rand(B, Ns, Ns, generator=gen) < 0.05).int(),
            "macro_obj_loc": torch.arange(Nv).repeat(B, 1),
            "micro_positive_obj": torch.randint(0, 400000, (B, Nv, K), generator=gen),
            "micro_negative_obj": torch.randint(0, 400000, (B, Nv, K), generator=gen),
            "micro_obj_mask": torch.ones(B, Nv, K, dtype=torch.int32),
        }
        return inp, torch.randint(1, 914, (B,), generator=gen)

    nstep = [0]

    def fwd_loss(inp, answer):
        with torch.no_grad():
            lc, lv, ls, mil, _ = O.attmodel_forward(P, inp)
            O.train_loss(lc, lv, ls, answer, mil)

    def train_step(inp, answer):
        nstep[0] += 1
        for p in P.values():
            p.grad = None
        drop = (1000 + nstep[0], rate) if rate > 0 else None
        lc, lv, ls, mil, _ = O.attmodel_forward(P, inp, drop=drop)
        loss, _ = O.train_loss(lc, lv, ls, answer, mil)
        loss.backward()
        with torch.no_grad():
            O.adam_step(P, {k: v.grad for k, v in P.items() if v.grad is not None}, state,
                        nstep[0])

    legs = {}
    for name, fn in (("train_step", train_step), ("fwd_loss", fwd_loss)):
        for B in (4, 32):
            inp, answer = inputs(B)
            fn(inp, answer)  # warm (the first call materialises the hash-filled params)
            n, t0 = 0, time.perf_counter()
            while True:
                fn(inp, answer)
                n += 1
                if time.perf_counter() - t0 >= seconds / 4:
                    break
            dt = time.perf_counter() - t0
            legs[f"{name}_b{B}"] = {"samples_per_s": round(B * n / dt, 3), "iters": n,
                                    "seconds": round(dt, 2), "threads": threads}
            print(f"cpu_baseline {name} B={B}: {B * n / dt:.2f} samples/s ({threads} threads)",
                  file=sys.stderr, flush=True)
    if omp and omp != threads:  # the same leg at the job's OMP_NUM_THREADS
        torch.set_num_threads(omp)
        inp, answer = inputs(32)
        train_step(inp, answer)
        n, t0 = 0, time.perf_counter()
        while True:
            train_step(inp, answer)
            n += 1
            if time.perf_counter() - t0 >= seconds / 4:
                break
        dt = time.perf_counter() - t0
        legs[f"train_step_b32_omp{omp}"] = {"samples_per_s": round(32 * n / dt, 3), "iters": n,
                                            "seconds": round(dt, 2), "threads": omp}
        torch.set_num_threads(threads)
    head = legs["train_step_b32"]
    return {"value": head["samples_per_s"], "unit": "QA-samples/s", "cores": threads,
            "kind": "port",
            "host_cpus": os.cpu_count(), "affinity_cpus": avail, "cgroup_cpus": quota,
            "cpu_model": _cpu_model(),
            "legs": legs,
            "sample": f"oracle/savqa_oracle.py on torch CPU ({threads} threads = the affinity "
                      f"mask capped by the cgroup CPU quota; extra leg at OMP_NUM_THREADS="
                      f"{omp or 'unset'} when different): train step "
                      f"(fwd+loss+bwd+Adam, dropout {rate}) and fwd+loss at the cfg-1 shape, "
                      f"B=4 and B=32 (value = train step, B=32), ~{seconds / 4:.0f}s per leg"}


WORKLOADS = {
    "cfg2": dict(d=512, H=8, Nv=36, Ns=59, batch=256,
                 desc="cfg2: model_v=3 train step (fwd+loss+bwd+Adam), fp32, 36 regions x 2048-d, "
                      "14 q-tokens, 59 nodes, d=512 h=8 L=6, MIL-NCE only_obj topN=5 H=1024, "
                      "914 classes, decMask"),
    "cfg3": dict(d=512, H=8, Nv=36, Ns=59, batch=512, prec="bf16",
                 desc="cfg3: model_v=3 train step, bf16-resident GEMM operands and attention "
                      "storage (fp32 accumulation, fp32 residual stream / LN / softmax / loss / "
                      "master weights / Adam), 36 regions x 2048-d, "
                      "14 q-tokens, 59 nodes, d=512 h=8 L=6, MIL-NCE only_obj topN=5 H=1024, "
                      "914 classes, decMask"),
    "rel": dict(d=512, H=8, Nv=36, Ns=36 + 4 + 36 * 35, batch=4, rel=True, maxlen=1600, hm=64,
                desc="relation mode (only_obj=False, submit.py:76 'with relations', :87 maxlen "
                     "1600, :101 hidden_size_mil 64): model_v=3 train step, fp32, 36 regions, "
                     "super-node graph of 1300 nodes (36 objects, 4 attributes, 1260 relation "
                     "nodes: T_syb=1314), 31,500 positive + 31,500 negative relation entries per "
                     "sample, 311 relation categories (R: 311x64x64), d=512 h=8 L=6, H_mil=64, "
                     "topN=5, decMask"),
    "cfg5": dict(d=512, H=8, Nv=36, Ns=59, batch=1024, prec="fp8",
                 desc="cfg5: model_v=3 train step, fp8-e4m3 region features (per-32 e8m0 block "
                      "scales, quantised outside the timed region as a loader would ship them) "
                      "into block-scaled fp8 MFMA (att_vis_grid.syb_mlp2, MIL_NCE.vis_mlp), bf16 "
                      "GEMM operands and attention storage elsewhere (fp32 accumulation, fp32 "
                      "residual stream / LN / softmax / loss / master weights / Adam), 36 regions "
                      "x 2048-d, 14 q-tokens, 59 nodes, d=512 h=8 L=6, MIL-NCE only_obj topN=5 "
                      "H=1024, 914 classes, decMask"),
    "cfg4": dict(d=1024, H=16, Nv=100, Ns=435, batch=32,
                 desc="cfg4: model_v=3 train step, fp32, 100 regions x 2048-d, 14 q-tokens, "
                      "435-node scene graph (T_vis=114, T_syb=449), d=1024 h=16 (h=12 does not "
                      "divide d=1024) L=6, MIL-NCE only_obj topN=5 H=1024, 914 classes, decMask"),
}

PROFILES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
# committed PMC passes of each workload's bench command (tools/profile_round.sh)
ROOFLINE_JSON = {w: f"r06_{w}_roofline.json" for w in ("cfg2", "cfg3", "cfg4", "cfg5", "rel")}


def committed_traffic(variant, workload="cfg2"):
    """HBM bytes per launch of `variant` from the committed PMC passes of this command
    (tools/summarize_prof.py: 2 x FETCH_SIZE + WRITE_SIZE, gfx950-corrected), or None."""
    name = ROOFLINE_JSON.get(workload)
    if name is None:
        return None
    try:
        with open(os.path.join(PROFILES, name)) as f:
            t = json.load(f)["traffic"].get(variant)
        return None if t is None else round(t["hbm_bytes_per_launch"])
    except (OSError, ValueError, KeyError):
        return None


DUMP_ROWS = 4096  # --dump-outputs: sampled elements per parameter tensor


def dump_outputs(path, model, loss, outs):
    """Write what the last timed step computed as path/<name>.npy (float32): the step's
    return values (the three heads' logits, the MIL-NCE terms, the loss) in full, and of its
    side effect on the model, the gradients and the Adam-updated parameters, a fixed seeded
    sample of up to DUMP_ROWS elements per live tensor in arena order (the whole arena is
    ~1.8 GB at cfg 2). ~10 MB in all at cfg 2.

    Inputs, weights and dropout seeds are the same from run to run, and every sum of the step
    has a fixed order, so two runs of one build write the same arrays."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {"loss": loss.detach().reshape(1)}
    for name, t in zip(("logits_concat", "logits_vis", "logits_syb", "mil_nce_obj",
                        "mil_nce_rel"), outs):
        if torch.is_tensor(t):  # the relation term is a plain 0 in objects-only mode
            arrays[name] = t.detach()
    arena = model._arena
    gen = torch.Generator().manual_seed(20240)
    idx = []
    for n in arena.live_names:
        o, shp = arena.offsets[n]
        numel = int(torch.Size(shp).numel())
        k = min(numel, DUMP_ROWS)
        idx.append(o + (torch.arange(numel) if k == numel
                        else torch.randint(0, numel, (k,), generator=gen).sort().values))
    idx = torch.cat(idx).to(arena.flat.device)
    arrays["params_sample"] = arena.flat[idx]
    if arena.grad is not None:
        arrays["grads_sample"] = arena.grad[idx]
    for name, t in arrays.items():
        np.save(os.path.join(path, name + ".npy"),
                np.ascontiguousarray(t.float().cpu().numpy().astype(np.float32)))


def _self_launch(n):
    """Run this command as `python -m torch.distributed.run --nproc-per-node n` (rendezvous on
    127.0.0.1, a free port) in a child process and return its exit status. Called before any
    HIP call, so the parent never holds a GPU context while its ranks run."""
    import socket
    import subprocess
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(n), "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    return subprocess.call(cmd, env=env)


def _rank_devices(dev, backend):
    """(rank, local device index, PCI bus, uuid) of every rank, gathered over the group."""
    p = torch.cuda.get_device_properties(dev)
    me = {"rank": dist.get_rank() if dist.is_initialized() else 0, "device": dev.index,
          "pci": f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}",
          "uuid": str(getattr(p, "uuid", ""))}
    if not dist.is_initialized():
        return [me]
    out = [None] * dist.get_world_size()
    dist.all_gather_object(out, me)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="samples per GPU (cfg2: 256)")
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="cfg2",
                    help="cfg2 = BASELINE config 2 (fp32, 256/GPU: the metric's workload); cfg3 = "
                         "config 3 (bf16, 512/GPU); cfg4 = the 100-region / 435-node scene-graph "
                         "stress shape (d=1024, 16 heads, T_syb=449); cfg5 = config 5 (fp8 region "
                         "features + bf16, 1024/GPU); rel = the super-node relation branch")
    ap.add_argument("--dropout", type=float, default=0.5,
                    help="dropout_rate (reference training default 0.5, main:466)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed (logits, "
                         "MIL-NCE terms, loss, a seeded sample of the gradients and the updated "
                         "parameters) as DIR/<name>.npy, float32 (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run the roofline probe steps, the CPU "
                         "oracle baseline (cfg2, 1 GPU) and, N > 1, the --comm-steps diagnostic "
                         "steps; a plain run reports null for them")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline")
    ap.add_argument("--cpu-seconds", type=float, default=24.0)
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the probe steps")
    ap.add_argument("--serial", action="store_true",
                    help="run both stacks on one stream (per-kernel profiling)")
    ap.add_argument("--bucket-mb", type=float, default=64.0,
                    help="N > 1: all-reduce bucket size of the streamed gradient exchange")
    ap.add_argument("--bwd-gate", default=None,
                    help="N > 1: backward schedule (engine.vis_gate): auto (= enc4 with an "
                         "all-reduce), concurrent, enc1..enc6, dec, syb_first")
    ap.add_argument("--comm-steps", type=int, default=2,
                    help="--full, N > 1: untimed diagnostic steps after the timed region whose "
                         "collectives are HIP-event timed (the line's 'comm' report)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # launcher-less form (`python bench.py --gpus N`): start the N ranks here, before
        # anything touches the GPU, as a torch.distributed.run child (the driver's own
        # launch line), and exit with its status -- one rank per GPU, main:517's mp.spawn role
        return _self_launch(args.gpus)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} "
              f"ranks", file=sys.stderr, flush=True)
        return 2
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("SAVQA_DIST_BACKEND", "nccl") != "nccl":  # rehearsal: ranks share GPUs
        local %= max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        # RCCL ("nccl" on ROCm) over xGMI; SAVQA_DIST_BACKEND=gloo only to rehearse the
        # N>1 code path with several ranks on one GPU (RCCL refuses duplicate devices)
        backend = os.environ.get("SAVQA_DIST_BACKEND", "nccl")
        dist.init_process_group(backend, device_id=dev if backend == "nccl" else None)
        if dist.get_world_size() != args.gpus:
            print(f"bench.py: process group has {dist.get_world_size()} ranks, --gpus "
                  f"{args.gpus}", file=sys.stderr, flush=True)
            return 2

    # the per-step dropout seeds come from torch's CPU generator: seed it, so that the same
    # arguments give the same inputs and masks from run to run
    torch.manual_seed(0)

    import savqa_amd  # noqa: F401
    from savqa_amd import ops
    from savqa_amd.AttModel_x3 import AttModel
    from savqa_amd.data import model_args, synthetic_batch
    from savqa_amd.ddp import GradReducer
    from savqa_amd.loss import smoothed_loss
    from savqa_amd.optim import Adam
    from savqa_amd.utils import init_params_

    W = WORKLOADS[args.workload]
    B = args.batch or W["batch"]
    d, H, Nv, Ns = W["d"], W["H"], W["Nv"], W["Ns"]
    hm = W.get("hm", 1024)  # hidden_size_mil (submit.py:101: 1024 objects-only, 64 with relations)
    model = AttModel(None, d, hm, 914, 40, W.get("maxlen", 450), 49, 6, H, args.dropout, 0.1, 311,
                     not W.get("rel", False), device=dev, init=False,
                     gemm_precision=W.get("prec", "fp32"))
    init_params_(model, seed=0)  # identical on every rank (same seed), like a broadcast
    model.train()
    if args.serial:
        model._engine.concurrent = False
    if args.bwd_gate:
        model._engine.bwd_order = args.bwd_gate
    opt = Adam(model, lr=1e-4)
    reducer = GradReducer(model._arena, bucket_mb=args.bucket_mb) if world > 1 else None
    if reducer:
        model.attach_reducer(reducer, batch_size=B)
    if W.get("rel"):
        from savqa_amd.data import model_args_rel, synthetic_relation_batch
        batch = synthetic_relation_batch(B, Nv=Nv, seed=1234 + rank, device=dev)
        margs = model_args_rel(batch)
    else:
        batch = synthetic_batch(B, Nv=Nv, Ns=Ns, seed=1234 + rank, device=dev)
        margs = model_args(batch)
    fwd_kw = {}
    if W.get("prec") == "fp8":
        # the loader ships e4m3 codes + e8m0 block scales (savqa_quant_fp8's layout)
        R, Dv = B * Nv, batch["vis_fea"].shape[-1]
        q8 = torch.empty(R, Dv, dtype=torch.uint8, device=dev)
        s8 = torch.empty(R, Dv // 32, dtype=torch.uint8, device=dev)
        ops.quant_fp8(batch["vis_fea"].reshape(R, Dv), R, Dv, Dv, q8, Dv, s8, Dv // 32)
        margs[0] = q8.view(torch.float8_e4m3fn).reshape(B, Nv, Dv)
        fwd_kw["vis_fea_scale"] = s8.reshape(B, Nv, Dv // 32)
        del batch["vis_fea"]

    def step():
        if reducer:
            reducer.begin()
        lc, lv, ls, mil, mil_rel = model(*margs, decMask=True, mcb=False, **fwd_kw)
        loss, _ = smoothed_loss(lc, lv, ls, batch["answer"], mil, with_milnce=True,
                                mil_nce_rel=mil_rel)
        opt.zero_grad()
        loss.backward()
        opt.step(reducer=reducer)
        return loss, (lc, lv, ls, mil, mil_rel)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss, outs = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, model, loss, outs)
    comm_steps = args.comm_steps if args.full else 0
    comm = None
    if world > 1:
        # per-rank diagnosis of the exchange (untimed steps): this rank's own step time from
        # the timed region, and over --comm-steps steps with HIP events around every
        # collective the summed collective time, the part that outlasted the backward
        # (exposed), and the dense / row bytes
        mine = {"rank": rank, "ms_per_step": round(elapsed / args.steps * 1e3, 3)}
        if comm_steps > 0:
            reducer.time_collectives(True)
            for _ in range(comm_steps):
                step()
            mine.update(reducer.comm_summary() or {})
            reducer.time_collectives(False)
        ranks_c = [None] * world
        dist.all_gather_object(ranks_c, mine)
        eng = model._engine
        comm = {"bucket_mb": args.bucket_mb, "bwd_order": eng.bwd_order,
                "bwd_schedule": (eng.AUTO_GATE if eng.multi_rank else "concurrent")
                if eng.bwd_order == "auto" else eng.bwd_order,
                "diag_steps": comm_steps, "ranks": ranks_c}
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t)
    final_loss = float(loss.detach())
    backend = dist.get_backend() if dist.is_initialized() else None
    dist_info = {"backend": ("rccl" if backend == "nccl" else backend),
                 "world_size": dist.get_world_size() if dist.is_initialized() else 1,
                 "ranks": _rank_devices(dev, backend)}

    value = world * B * args.steps / elapsed
    ms_step = elapsed / args.steps * 1e3
    fl = train_flops_per_sample(Tv=Nv + 14, Ts=Ns + 14, Nv=Nv, Ns=Ns, d=d, Hm=hm)
    lp = W.get("prec") in ("bf16", "fp8")
    peak = BF16_MFMA_PEAK_TFLOPS if lp else FP32_MFMA_PEAK_TFLOPS

    roof = None
    if args.full and not args.no_roofline:
        # per-kernel timing needs kernels that do not share the GPU: run the probe steps
        # with both stacks on one stream (the timed region above overlaps them)
        probe = ops.GemmProbe()
        kprobe = []
        model._engine.concurrent = False
        ops.set_gemm_probe(probe)
        ops.set_kernel_probe(kprobe)
        for _ in range(2):
            step()
        ops.set_gemm_probe(None)
        ops.set_kernel_probe(None)
        model._engine.concurrent = not args.serial
        agg = probe.summary()
        var, (n, flops, ms) = max(agg.items(), key=lambda kv: kv[1][2])
        achieved = (flops / n) / (ms / n * 1e-3) / 1e12
        kpeak = peak
        basis = None
        if var.startswith("gemm_lp"):  # bf16 operands, or fp8 (gemm_lp_kernel<...,true>)
            kpeak = FP8_MFMA_PEAK_TFLOPS if var.endswith(",true>") else BF16_MFMA_PEAK_TFLOPS
        elif var.startswith("gemm_x6"):
            # fp32 GEMM issued as six bf16 MFMA products per fp32 product (exact 3-term
            # splits): the kernel's ceiling is the dense bf16 peak / 6 = 416.7 TF of fp32 work,
            # so that is `peak`; the fp32 MFMA peak (157.3 TF), which this kernel can pass, is
            # reported beside it
            kpeak = round(BF16_MFMA_PEAK_TFLOPS / 6, 1)
            basis = {"fp32_mfma_peak": FP32_MFMA_PEAK_TFLOPS,
                     "frac_vs_fp32_mfma_peak": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4),
                     "basis": "gemm_x6.hip: exact 3-term bf16 split, 6 v_mfma_f32_16x16x32_bf16 "
                              "products per fp32 product; peak = 2.5 PF dense bf16 / 6"}
        allfl = sum(v[1] for v in agg.values())
        allms = sum(v[2] for v in agg.values())
        roof = {"bound": "mfma", "kernel": var, "launches_per_step": n // 2,
                "avg_launch_us": round(ms / n * 1e3, 2), "flops_per_launch": flops / n,
                "achieved": round(achieved, 2), "peak": kpeak, "unit": "TFLOP/s",
                "frac": round(achieved / kpeak, 4),
                "traffic": committed_traffic(var, args.workload),
                "all_gemm_tflops": round(allfl / (allms * 1e-3) / 1e12, 2),
                "gemm_ms_per_step": round(allms / 2, 2)}
        if basis:
            roof["x6"] = basis
        roof["hbm_kernels"] = hbm_report(kprobe, lp)

    if rank == 0:
        cpu = None
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload == "cfg2":
            cpu = cpu_baseline(args.cpu_seconds, rate=args.dropout)
        out = {
            "metric": METRIC, "value": round(value, 2), "unit": "QA-samples/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_step, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": {"bf16": "bf16 (GEMM operands; fp32 accumulate)",
                      "fp8": "fp8-e4m3 region features + bf16 (GEMM operands; fp32 accumulate)"
                      }.get(W.get("prec"), "fp32"),
            "data": "synthetic (collate_fn tensor contract; random-init weights)",
            "config": {"workload": W["desc"] + f", dropout {args.dropout}",
                       "per_gpu_batch": B, "global_batch": world * B,
                       "parallelism": f"dp{world}"},
            "model_tflops": round(value * fl / 1e12, 2),
            "model_mfma_frac": round(value * fl / 1e12 / (peak * world), 4),
            "loss": round(final_loss, 4),
            "dist": dist_info,
            "comm": comm,
            "roofline": roof,
            "cpu_baseline": cpu,
        }
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
