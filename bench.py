#!/usr/bin/env python
"""Benchmark of the expertsim GAN training step on MI355X (BASELINE.json metric).

Default workload = BASELINE configs[2]: neutron 44x44 ZDC GAN with SDI diversity + auxiliary coord
regressor (always on in the reference), 1 expert, batch 1024 per GPU, synthetic data resident in HBM,
in fp32 arithmetic (split-fp32 MFMA: every fp32 operand as the exact sum of three bf16 planes, six
plane products per fp32 product accumulated in fp32, deterministic reductions: the mode the golden
parity tests pin; --fp32-mfma exact runs the convs on the fp32 MFMA instead).  One "step" = ``MoEWrapper.train_step`` (router, G fwd x2 + bwd x2, D fwd
x4 + bwd x4, aux regressor fwd/bwd, losses, four fused Adam updates; with N > 1 also the RCCL
gradient all-reduces, SyncBN by default).

    python bench.py [--gpus N --steps K --warmup W --batch B --experts E --arch neutron|proton]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

A plain run sets up, warms up, times the K steps and prints ONE JSON line (rank 0) with the metric.
``--dump-outputs DIR`` also writes what the last timed step produced (its metric scalars and the
model state it left) as ``DIR/<name>.npy``; the inputs and seeds are fixed, so two builds can be
compared array for array.  ``--full`` adds the legs that take runs of their own: a live-measured
roofline of the dominant kernel (HIP events on its launch stream inside eager steps of the same
model), the bf16 performance mode (bf16 GEMM operands, fp32 accumulation) as ``perf_bf16`` and the
CPU baseline (the oracle, a CPU fp32 restatement of the same step, timed on this host's cores on a
bounded sample); ``--no-probe``, ``--other-steps 0`` and ``--no-cpu-baseline`` drop single legs of it.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd")
sys.path.insert(0, PKG_DIR)
sys.path.insert(0, ROOT)

# algorithmic FLOPs per image per train_step (torch FlopCounterMode on the
# reference): neutron 10.573 GFLOP, proton 28.566 GFLOP; the declared 56x56 extension (configs[4],
# no reference model) 16.868 GFLOP = 6*2746.3 + 12*8.05 + 3*97.9 MFLOP (same counter on the oracle)
STEP_FLOP_PER_IMAGE = {"neutron": 10.573e9, "proton": 28.566e9, "neutron56": 16.868e9}
PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}   # MI355X dense MFMA peaks (MI355X_MICROARCH.md)
# split-fp32 (train.fp32_mfma: split): one fp32 product = 6 bf16 plane products, all executed on the
# bf16 MFMA pipe, so the roofline of a split kernel is the EXECUTED bf16 work against the 2.5 PF/s
# dense bf16 peak (no derived "split peak"); the executed work is the library's own tally
# timed loop: at most this many replayed steps queued ahead of the GPU (a replay is ~1000 AQL packets;
# an unbounded loop queued ~10.5k packets, which is where a profiled run aborted, profiles/r03t_*)
MAX_INFLIGHT = 2
IMAGE = {"neutron": "44x44", "proton": "56x30", "neutron56": "56x56"}


def traffic_json(arch, batch, precision, mode):
    """Committed PMC passes of the roofline kernel: bf16 tools/gpu_traffic.sh -> tools/traffic_json.py,
    fp32 tools/gpu_traffic32.sh -> tools/traffic32.py."""
    name = (f"traffic_{arch}_c5_{mode}_b{batch}.json" if precision == "bf16"
            else f"traffic32{'s' if FP32_MFMA == 'split' else ''}_{arch}_c5_{mode}_b{batch}.json")
    p = os.path.join(ROOT, "profiles", name)
    return p if os.path.exists(p) else None




def workload_label(arch, E, batch, world):
    """Which BASELINE.json config the flags reproduce (configs[0] is the CPU plumbing run)."""
    gb = batch * world
    if arch == "neutron" and E == 1 and gb == 512 and world == 1:
        k = "configs[1]"
    elif arch == "neutron" and E == 1 and gb == 1024 and world == 1:
        k = "configs[2]"
    elif arch == "neutron" and E == 4 and gb == 2048:
        k = "configs[3]"
    elif arch == "neutron56" and E == 8 and gb == 4096:
        k = "configs[4], declared 56x56 extension, parity unpinned"
    elif E == 1 and batch in (512, 1024) and world > 1:
        k = f"configs[{1 if batch == 512 else 2}] per GPU, weak-scaled over {world} GPUs"
    else:
        k = "not a BASELINE config"
    return (f"{arch} {IMAGE[arch]} MoE-GAN train_step (hinge + SDI + intensity + aux regressor), "
            f"E={E}, B={batch} per GPU, global {gb} ({k})")


# Forward FLOPs per image of the probed generator convs (= the algorithmic count charged to each of
# their fwd / dgrad / wgrad ops, as torch's flop counter does), by (arch, op key)
PROBED = {
    "neutron": {"c5": 2 * 46 * 46 * 128 * (256 * 9)},      # conv_layers.5: 256x48x48 -> 128x46x46, k3
    "neutron56": {"c5": 2 * 58 * 58 * 128 * (256 * 9)},    # conv_layers.5: 256x60x60 -> 128x58x58, k3
    # conv_layers.1: 512x36x20 (x2 upsample of 18x10) -> 256x35x19, k4 p1 (sub-pixel split ring);
    # conv_layers.5: 256x56x30 (resize of 35x19) -> 128x55x29, k4 p1 (register-staged fp32 MFMA)
    "proton": {"c1": 2 * 35 * 19 * 256 * (512 * 16), "c5": 2 * 55 * 29 * 128 * (256 * 16)},
}
LAYER_NAME = {"c1": "conv_layers.1", "c5": "conv_layers.5"}


def conv_flops_per_image(arch):
    """Algorithmic forward FLOPs per image of the arch's conv_layers.5 (the headline's roofline conv)."""
    return PROBED[arch]["c5"]


FP32_MFMA = "split"   # train.fp32_mfma of the fp32 line (--fp32-mfma)


def build(arch, E, precision, seed, device):
    import torch
    from expertsim.config import inject_shared, load_config
    from expertsim.models import build_model
    from expertsim.models.moe import MoEWrapper
    from expertsim.train.training_setup import setup_optimizers
    ov = [f"model.architecture={arch}", f"model.n_experts={E}", f"train.precision={precision}",
          f"train.rng_seed={seed}", f"train.fp32_mfma={FP32_MFMA}"]
    if E > 1:
        ov.append("model.router.diff_strength=1e-6")     # default.yaml '1-6' 
    cfg = inject_shared(load_config(overrides=ov))
    torch.manual_seed(seed)
    parts = [build_model(f"{arch}.{k}", getattr(cfg.model, k), device) for k in ("generator", "discriminator", "aux_reg")]
    router = build_model("router_v1", cfg.model.router, device)
    moe = MoEWrapper(*parts, router, E, cfg, image_shape=tuple(parts[0].image_shape)).to(device)
    return moe, setup_optimizers(moe, cfg), cfg


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_threads():
    """Threads for the CPU baseline: every CPU this process's affinity allows, capped by the cgroup's
    CPU quota (a GPU box exposes the whole host's CPUs but grants a share of them); both stated."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = max(1, int(int(q) // int(per)))
    except (OSError, ValueError):
        pass
    return (min(aff, quota) if quota else aff), aff, quota


def cpu_baseline(arch, batch=1024, small=64, steps=2, budget_s=20.0):
    """The oracle (torch CPU fp32 restatement of the same step, pinned to the reference's goldens)
    timed on this host, on every CPU the affinity / cgroup quota allows.  Reported value: the bench's
    own workload (BASELINE configs[2], B = 1024), the median of ``steps`` train steps after the
    warm-up; the warm-up is B = ``small`` steps (also reported, median of those that fit
    ``budget_s``).  The reference's CPU throughput is flat in B."""
    import torch
    from oracle import expertsim_oracle as O
    from expertsim.utils.synthetic import make_batch
    threads, aff, quota = cpu_threads()
    torch.set_num_threads(threads)
    m = O.OracleMoE(arch, 1, dict(O.DEFAULT_CFG), seed=1234)
    g = torch.Generator().manual_seed(0)
    noise_fn = lambda e, w, shape: torch.randn(shape, generator=g)
    res = {}
    for b_, n_max in ((small, 21), (batch, steps)):
        b = make_batch(b_, arch, seed=0)
        t = {k: torch.from_numpy(v) for k, v in b.items()}
        times = []
        t_start = time.perf_counter()
        for i in range(n_max + (1 if b_ == small else 0)):     # + one untimed warm-up step at B = small
            t0 = time.perf_counter()
            m.train_step(0, t["cond"], t["real_images"].unsqueeze(1), t["true_positions"], t["std"], t["intensity"],
                         noise_fn, torch.empty(b_, 1).exponential_(generator=g))
            times.append(time.perf_counter() - t0)
            if b_ == small and time.perf_counter() - t_start > budget_s and len(times) >= 4:
                break
        timed_ = times[1:] if b_ == small else times
        res[b_] = (b_ / statistics.median(timed_), len(timed_), sum(timed_))
    return {"value": round(res[batch][0], 3), "unit": "images/s", "cores": threads, "kind": "port",
            "cpu_model": cpu_model(), "host_cpus": os.cpu_count(), "affinity_cpus": aff, "cgroup_cpu_quota": quota,
            "by_batch": {str(k): round(v[0], 3) for k, v in res.items()},
            "sample": "; ".join(f"{arch} E=1 B={k}: median of {v[1]} train step(s) ({v[2]:.1f} s)"
                                for k, v in res.items())
                      + f" (after one untimed B={small} step); oracle/expertsim_oracle.py (torch CPU fp32) on "
                        f"{threads} threads (affinity {aff} CPUs, cgroup quota {quota if quota else 'none'})"}


def timed(step, steps, world):
    """K steps between barrier + synchronize; the host stays at most MAX_INFLIGHT steps ahead of the
    GPU (it waits on the event of step i - MAX_INFLIGHT before issuing step i, which keeps the queue
    fed: a step is ~45 ms of GPU work against ~1 ms of host issue)."""
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    evs = [torch.cuda.Event() for _ in range(MAX_INFLIGHT)]
    last = None
    t0 = time.perf_counter()
    for i in range(steps):
        if i >= MAX_INFLIGHT:
            evs[i % MAX_INFLIGHT].synchronize()
        last = step()
        evs[i % MAX_INFLIGHT].record()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    return time.perf_counter() - t0, last


def make_step(moe, step_args, use_graph):
    """The timed step: returns the step's metric dict (device scalars), as train_step does."""
    def eager_step():
        return moe.train_step(*step_args)
    if not use_graph:
        return eager_step, None
    from expertsim.graph import StepGraph
    sg = StepGraph(moe, step_args, warmup=1, allow_dp=True)
    return sg.replay, sg


# --dump-outputs: at most this many bytes in all (float32 / float64 elements; larger arrays are sampled)
DUMP_BUDGET_BYTES = 48 << 20


def dump_outputs(path, metrics, moe):
    """What a caller of the timed step holds after its last step: the metric dict it returned
    (``metric.<key>.npy``, float32 scalars) and the model state it left behind (``state.<key>.npy``:
    every state_dict tensor of the generators, discriminators, aux regressors and router; floating
    tensors as float32, integer ones as float64).  An array above the per-array limit that keeps the
    whole dump within DUMP_BUDGET_BYTES is stored as a fixed seeded sample of its flattened elements."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    arrays = {f"metric.{k}": v for k, v in metrics.items()}
    arrays.update({f"state.{k}": v for k, v in moe.state_dict().items() if torch.is_tensor(v)})
    host = {}
    for k, v in arrays.items():
        v = v.detach()
        host[k] = (v.float() if v.is_floating_point() else v.double()).cpu().numpy()
    budget = DUMP_BUDGET_BYTES // 8          # elements, each charged as a float64
    limit = budget
    while sum(min(a.size, limit) for a in host.values()) > budget:
        limit = limit * 3 // 4
    for k, a in host.items():
        if a.size > limit:
            ix = np.sort(np.random.default_rng(0).integers(0, a.size, size=limit))
            a = a.reshape(-1)[ix]
        np.save(os.path.join(path, k + ".npy"), a)


def exec_flops(reset=False):
    """Host tally of the executed conv MFMA work (es_conv_exec_flops): [bf16 pipe, fp32 MFMA, VALU]."""
    import ctypes
    from expertsim import hip
    out = (ctypes.c_double * 3)()
    hip.call("es_conv_exec_flops", out, 1 if reset else 0)
    return list(out)


def aggregate_expert_ops(raw, counts, ef, arch, batch):
    """Multi-expert probe: per-expert op summaries {"G<e>.<layer>.<pass>": {count, total_ms,
    exec_flops_per_op, ...}} of capacity-B launches -> per op type "G*.<layer>.<pass>" with each
    expert's work scaled by its routed share B_e / B.  counts: per probe step, the E routed counts.
    ef: the step's capacity-B executed-work tally [bf16 pipe, fp32 MFMA, VALU].  Returns (stats,
    live shares, ef scaled to the live work)."""
    experts = len(counts[0])
    # each image is routed to one expert: B_e / B = the expert's share of the step's counts (under
    # data parallelism the counts are global, the share the same in expectation)
    tot = [sum(c) for c in counts]
    live = [sum(c[e] / t for c, t in zip(counts, tot)) / len(counts) for e in range(experts)]
    # the experts share one architecture: the capacity-B tally of a step is E x one expert's, its
    # live work sum_e B_e / B of one expert's
    ef = [v * sum(live) / experts for v in ef]
    stats = {}
    for lab, v in raw.items():
        e = int(lab.split(".")[0][1:])
        op = "G*." + lab.split(".", 1)[1]
        agg = stats.setdefault(op, {"count": 0, "total_ms": 0.0, "exec": [0.0, 0.0, 0.0], "alg": 0.0,
                                    "kernel_launches_per_op": v.get("kernel_launches_per_op")})
        agg["count"] += v["count"]
        agg["total_ms"] += v["total_ms"]
        ex = v.get("exec_flops_per_op", [0.0, 0.0, 0.0])
        agg["exec"] = [a + x * live[e] * v["count"] for a, x in zip(agg["exec"], ex)]
        agg["alg"] += PROBED[arch][op.split(".")[1]] * batch * live[e] * v["count"]
    for agg in stats.values():
        agg["avg_ms"] = agg["total_ms"] / agg["count"]
        agg["exec_flops_per_op"] = [x / agg["count"] for x in agg["exec"]]
        agg["alg_per_op"] = agg["alg"] / agg["count"]
    return stats, live, ef


def probe_dominant(moe, eager_step, steps, arch, batch, precision, experts=1):
    """Per-launch HIP events around the probed generator convs' ops (on their launch stream) over eager
    steps of the same model and batch -> the roofline object of the op with the largest total time.
    Executed MFMA work per op comes from the library's own tally (es_conv_exec_flops, read around each
    op: sub-pixel 4-class convs, split-fp32's 6 plane products, exact fp32 MFMA), so `achieved` is
    executed FLOPs / kernel time against the dense peak of the pipe the op ran on.
    experts > 1: every expert's ops are probed in eager steps (experts one after another, no graphs);
    an expert's op runs on capacity-B buffers with its routed count B_e live (dynamic rows), so its
    algorithmic and executed work are scaled by B_e / B (the step's counts, averaged over the probe
    steps; the <= 15 padding images of its last row group are not counted) and the op types are
    summed over the experts (label "G*.<layer>.<pass>")."""
    import torch
    from expertsim import layers
    keys = list(PROBED[arch])
    probe = layers.KernelProbe([f"G{e}.{k}.{m}" for e in range(experts) for k in keys
                                for m in ("fwd", "dgrad", "wgrad")])
    layers.set_probe(probe)
    exec_flops(reset=True)
    graphs = moe.expert_graphs
    moe.expert_graphs = False
    counts = []
    try:
        # one unprobed step first: the eager (graph-free) path allocates its own buffers on first use
        layers.set_probe(None)
        eager_step()
        torch.cuda.synchronize()
        exec_flops(reset=True)
        layers.set_probe(probe)
        for _ in range(steps):
            met = eager_step()
            if experts > 1:
                counts.append([met[f"n_choosen_experts_mean_epoch_{e}"] for e in range(experts)])
    finally:
        moe.expert_graphs = graphs
    torch.cuda.synchronize()
    ef = [v / steps for v in exec_flops(reset=True)]
    layers.set_probe(None)
    raw = probe.summary()
    if experts > 1:
        stats, live, ef = aggregate_expert_ops(raw, [[float(x) for x in c] for c in counts], ef, arch, batch)
    else:
        stats = raw

    def rate(label, v):
        alg = v.get("alg_per_op", PROBED[arch][label.split(".")[1]] * batch)
        ex = v.get("exec_flops_per_op", [alg, 0.0, 0.0])
        pipe = "bf16" if ex[0] >= ex[1] else "fp32"
        exe = ex[0] if pipe == "bf16" else ex[1]
        t = v["avg_ms"] * 1e-3
        return alg, exe, pipe, exe / t / 1e12, alg / t / 1e12
    dom = max(stats, key=lambda k: stats[k]["total_ms"])
    alg, exe, pipe, achieved, alg_rate = rate(dom, stats[dom])
    avg_ms = stats[dom]["avg_ms"]
    peak = PEAK_TFLOPS[pipe]
    layer = LAYER_NAME[dom.split(".")[1]]
    split = precision == "fp32" and pipe == "bf16"
    traffic, tnote, mfma_busy = None, None, None
    tj_path = (traffic_json(arch, batch, precision, dom.split(".")[-1])
               if dom.split(".")[1] == "c5" and experts == 1 else None)
    if tj_path:
        tj = json.load(open(tj_path))
        traffic = tj["traffic_bytes"]
        mfma_busy = tj.get("mfma_busy_frac")
        tnote = (f"HBM bytes per op: FETCH_SIZE x2 {tj['fetch_bytes']} + WRITE_SIZE {tj['write_bytes']} "
                 f"(algorithmic {tj['algorithmic_bytes']}), {os.path.relpath(tj_path, ROOT)}")
    kname = ("bf16 MFMA" if precision == "bf16" else
             "split-fp32, 6 x v_mfma_f32_16x16x32_bf16 per fp32 product" if split else
             "fp32, v_mfma_f32_16x16x4_f32")
    out_note = (f"; {experts} experts on dynamic rows: the op type summed over the experts' eager ops, work "
                f"scaled by each expert's mean live fraction {[round(x, 3) for x in live]}" if experts > 1 else "")
    return {"bound": "mfma", "kernel": f"{dom} (generator {layer}, {kname})",
            "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
            "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_note": tnote,
            "achieved_fp32_equiv_alg": round(alg_rate, 2),
            "note": f"achieved = EXECUTED MFMA FLOPs per op ({exe:.4g}, the library's tally es_conv_exec_flops "
                    f"read around the op; the reference's FLOPs are {alg:.4g}: sub-pixel 4-class convs execute "
                    f"es_subpixel_taps / 4RS of them, split-fp32 6 bf16 products per fp32 product) / op time, "
                    f"against the dense {pipe} MFMA peak {peak} TFLOP/s (MI355X_MICROARCH.md); "
                    "achieved_fp32_equiv_alg = the reference's FLOPs / op time (an algorithmic rate, not a utilisation)"
                    + out_note,
            "mfma_busy_pmc": mfma_busy,
            "flop_per_launch": alg, "exec_flop_per_launch": exe,
            "avg_ms": round(avg_ms, 4), "launches": stats[dom]["count"],
            "step_exec_flops": {"bf16_pipe": ef[0], "fp32_mfma": ef[1], "valu_thin": ef[2]},
            "kernel_launches_per_op": stats[dom].get("kernel_launches_per_op"),
            "launch_note": "avg_ms is per op; an fp32 op over > 1 GiB operands runs as image chunks "
                           "(kernel_launches_per_op MFMA kernels, rocprof lists each chunk separately)",
            "all_probed": {k: (lambda r: {"avg_ms": round(v["avg_ms"], 4), "kernels": v.get("kernel_launches_per_op"),
                                          "pipe": r[2], "exec_tflops": round(r[3], 2),
                                          "frac": round(r[3] / PEAK_TFLOPS[r[2]], 4)})(rate(k, v))
                           for k, v in stats.items()}}


def alg_fracs(step_flops_per_s):
    """The step's algorithmic FLOP rate over the dense fp32 and bf16 MFMA peaks (labelled rates)."""
    return {f"step_alg_over_{p}_peak": round(step_flops_per_s / 1e12 / PEAK_TFLOPS[p], 4) for p in ("fp32", "bf16")}


def step_exec_frac(roof, ms_per_step):
    """Executed conv MFMA work of one step (es_conv_exec_flops over the probe's eager steps) at the
    dense peaks of the pipes it ran on, as a fraction of the measured step time: the share of the step
    the MFMA pipes would be busy if every conv ran at peak."""
    if not roof or "step_exec_flops" not in roof:
        return None
    e = roof["step_exec_flops"]
    t = e["bf16_pipe"] / (PEAK_TFLOPS["bf16"] * 1e12) + e["fp32_mfma"] / (PEAK_TFLOPS["fp32"] * 1e12)
    return round(t / (ms_per_step * 1e-3), 4)


def run_mode(args, precision, steps, warmup, dev, rank, world, ddp, probe_steps, dump_dir=None):
    """Build a model in ``precision``, warm up, time ``steps`` steps; returns (value, dt, roof, launch).
    dump_dir: rank 0 writes the last timed step's outputs there (dump_outputs)."""
    import torch
    import torch.distributed as dist
    from expertsim.train.ddp import DataParallel
    from expertsim.utils.synthetic import make_batch
    moe, (og, od, oa, orr), cfg = build(args.arch, args.experts, precision, 1234, dev)
    if ddp:
        moe.ddp = DataParallel(sync_bn=args.sync_bn)
        moe.rank = rank
    b = make_batch(args.batch, args.arch, seed=1000 + rank)
    t = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    real = t["real_images"].unsqueeze(1).contiguous()
    step_args = (0, t["cond"], real, t["true_positions"], t["std"], t["intensity"], oa, og, od, orr, None, dev)
    use_graph = args.graph == "on" or (args.graph == "auto" and not ddp)
    if use_graph:
        from expertsim.graph import graph_supported
        # several RCCL ranks: capture only when asked for (--graph on keeps the ranks in lockstep)
        use_graph = graph_supported(moe, allow_dp=args.graph == "on")
    eager = lambda: moe.train_step(*step_args)   # (returns the metric dict)
    for _ in range(warmup):
        eager()
    step, sg = make_step(moe, step_args, use_graph)
    dt, last = timed(step, steps, world)
    if sg is not None:
        sg.sync_host_state([*og, *od, *oa, orr])
    if dump_dir and rank == 0:
        dump_outputs(dump_dir, last, moe)
    del last
    # the probe's eager steps run without the captured graphs: release their pools first
    del step, sg
    step = sg = None
    if getattr(moe, "_egraphs", None) is not None:
        moe._egraphs.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    roof = None
    if probe_steps:
        # every rank runs the probed eager steps (their gradient all-reduces are collectives);
        # rank 0 reports
        roof = probe_dominant(moe, eager, probe_steps, args.arch, args.batch, precision, args.experts)
        if rank != 0:
            roof = None
    value = args.batch * world * steps / dt
    del moe, og, od, oa, orr, step, sg, t, real, step_args
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return value, dt, roof, ("hip_graph" if use_graph else "eager")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=1024, help="images per GPU")
    ap.add_argument("--arch", default="neutron", choices=["neutron", "proton", "neutron56"])
    ap.add_argument("--experts", type=int, default=1)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="headline: fp32 = the reference's precision (split-fp32 or exact fp32 MFMA, the mode "
                         "the golden parity tests pin); bf16 = bf16 GEMM operands, fp32 accumulation")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs of its own: the per-kernel roofline probe, the other "
                         "precision's secondary line and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (metric scalars, model state) as DIR/<name>.npy")
    ap.add_argument("--other-steps", type=int, default=50,
                    help="--full: timed steps of the other precision's secondary line (0: skip)")
    ap.add_argument("--fp32-mfma", choices=["exact", "split"], default="split",
                    help="fp32 conv arithmetic: exact fp32 MFMA, or split-fp32 (three bf16 planes, six products)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-probe", action="store_true", help="--full: skip the per-kernel HIP-event probe")
    ap.add_argument("--graph", choices=["auto", "on", "off"], default="auto",
                    help="replay the step as a captured HIP graph (auto: single process)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="data parallel: global BatchNorm / SDI / router statistics (single-device semantics); "
                         "the default with N > 1 (the reference's global-batch objective)")
    ap.add_argument("--no-sync-bn", action="store_true",
                    help="data parallel: per-rank BatchNorm / SDI statistics (torch DDP without SyncBatchNorm)")
    ap.add_argument("--ddp", action="store_true",
                    help="run the data-parallel code path even on one process (1-rank RCCL group)")
    ap.add_argument("--backend", choices=["nccl", "gloo"], default="nccl",
                    help="process-group backend (nccl = RCCL over xGMI; gloo only to rehearse several ranks "
                         "on one GPU)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    # measured lines come from the default build and kernel paths only: no ES_* environment override
    # (ES_LIB would load another build; INTEGRATION.md §2 lists the test hooks)
    stray = sorted(k for k in os.environ if k.startswith("ES_"))
    if stray:
        sys.exit(f"bench.py: refusing to run with experimental switches set: {', '.join(stray)}")
    global FP32_MFMA
    FP32_MFMA = args.fp32_mfma

    # stdout carries exactly the one JSON line: RCCL's init banner and gloo's connection messages are
    # written to fd 1 by native code, so fd 1 is pointed at stderr and the JSON goes to a saved copy
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # one rank per GPU; ranks beyond the visible devices (gloo rehearsals on a 1-GPU box) share them
    local = local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    ddp = world > 1 or args.ddp
    args.sync_bn = (args.sync_bn or world > 1) and not args.no_sync_bn
    if ddp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    # E > 1: the probe runs eager steps (the experts' ops visible to the host) and scales each expert's
    # work by its routed share of the batch (dynamic rows)
    probe_steps = 5 if args.full and not args.no_probe else 0
    value, dt, roof, launch = run_mode(args, args.precision, args.steps, args.warmup, dev, rank, world, ddp,
                                       probe_steps, args.dump_outputs)
    other = None
    other_p = "bf16" if args.precision == "fp32" else "fp32"
    if args.full and args.other_steps > 0 and world == 1:
        vo, dto, roofo, launcho = run_mode(args, other_p, args.other_steps, 5, dev, rank, world, ddp,
                                           3 if probe_steps else 0)
        other = {"dtype": other_p, "value": round(vo, 2), "unit": "images/s", "steps": args.other_steps,
                 "ms_per_step": round(dto / args.other_steps * 1e3, 3), "step_launch": launcho,
                 "step_pipe_busy_frac": step_exec_frac(roofo, dto / args.other_steps * 1e3),
                 **alg_fracs(STEP_FLOP_PER_IMAGE[args.arch] * vo),
                 "roofline": roofo,
                 "note": ("bf16 performance mode: bf16 GEMM operands, fp32 accumulation / statistics / "
                          "parameters; validated statistically (tests/test_bf16_stats_gpu.py)" if other_p == "bf16"
                          else "exact fp32 MFMA parity mode")}

    if rank == 0:
        step_flops = STEP_FLOP_PER_IMAGE[args.arch] * value
        out = {
            "metric": "GAN-step images/sec (44x44 ZDC) at 1/2/4/8 MI355X; conv MFMA util %",
            "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True,
            "step_launch": launch,
            "scaling": "weak", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
            "config": {"workload": workload_label(args.arch, args.experts, args.batch, world),
                       "arch": args.arch, "n_experts": args.experts, "batch_per_gpu": args.batch,
                       "global_batch": args.batch * world, "image": IMAGE[args.arch],
                       "parallelism": f"dp{world}", "sync_bn": bool(args.sync_bn) if ddp else None},
            "step_tflops_alg": round(step_flops / 1e12, 2),
            **alg_fracs(step_flops),
            "step_pipe_busy_frac": step_exec_frac(roof, dt / args.steps * 1e3),
            "step_frac_note": "step_alg_over_{fp32,bf16}_peak = the reference's FLOPs per step (step_tflops_alg: "
                              f"{STEP_FLOP_PER_IMAGE[args.arch] / 1e9:.3f} GFLOP/image x images/s) / the dense fp32 "
                              "(157.3) or bf16 (2500 TFLOP/s) MFMA peak: algorithmic rates, NOT utilisations (the "
                              "sub-pixel convs execute 4/9 of the reference's MACs and split-fp32 runs on the bf16 "
                              "pipe, so the fp32 one can exceed 1); step_pipe_busy_frac = EXECUTED conv MFMA FLOPs "
                              "per step (bf16 pipe incl. split-fp32 plane products at 2500 TF, exact fp32 MFMA at "
                              "157.3 TF) / step time, how busy the pipes the convs run on would be at peak",
            "roofline": roof,
        }
        if args.precision == "fp32":
            out["fp32_mfma"] = FP32_MFMA
            out["precision_note"] = (
                "fp32 = the reference's arithmetic precision, deterministic reductions; the golden parity tests "
                "pin this mode within 1e-4. "
                + ("split-fp32 convs: each fp32 operand is the exact sum of three bf16 planes, the six plane "
                   "products with p + q <= 2 run on v_mfma_f32_16x16x32_bf16 into fresh fp32 accumulators that are "
                   "added to the running sums with round-to-nearest (dropped terms < 2^-23 |a b| per product)"
                   if FP32_MFMA == "split"
                   else "exact fp32 MFMA (v_mfma_f32_16x16x4_f32)"))
        else:
            out["precision_note"] = "bf16 GEMM operands, fp32 accumulation"
        if other is not None:
            out["perf_bf16" if other_p == "bf16" else "parity_fp32"] = other
        if args.full and world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(args.arch)
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if ddp:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
