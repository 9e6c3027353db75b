"""Timing of the device sliced Wasserstein distance of whole images (expertsim/train/sliced.py) on one device,
against the host formulation (numpy's fp64 product, scipy.stats.wasserstein_distance per direction).

    python tools/sliced_bench.py [--n 16384] [--proj 256] [--out profiles/sliced.json]

One process, 1 warm-up + 5 timed runs per device figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: neutron 44x44 fp32 synthetic images, N real (seed 11) against N
generated (seed 12), resident on the device, P directions of train.sliced.directions; E = 1 (the joint segment and
one expert holding everything) and E = 4 (a seeded uniform expert vector).

Timed: es_sliced_project alone on the real side (device events), with its FLOP/s as 2 N D P over the time, that
rate as a share of the chip's 78.6 TFLOP/s fp64 figure (the fp64 VECTOR peak: the guides give no fp64 matrix rate
for this chip, so the share says how the kernel compares with the vector pipe, not how full the matrix pipe is),
its image bytes N D 4 over the time against the 6.29 TB/s measured HBM rate, and which of the two lower bounds is the
larger; es_sliced_directions alone; per E es_wasserstein_1d alone on the two projection tables (all (E + 1) x P
problems) and sliced() end to end (directions, both projections, the dispatch, the distances, the moments and the
one device-to-host copy) by the host clock around a synchronise; then MoEWrapper.evaluate_device of a freshly
initialised model at epoch 0 without and with sliced=True, the two ALTERNATING run by run in the same process.
Baseline, ONE timed run on the host, the joint segment only: the copy of both image sets and the directions out,
the fp64 X @ theta.T of both sides, scipy.stats.wasserstein_distance per direction.
"""
import argparse
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd"))

FP64_FLOPS = 78.6e12          # the chip's fp64 vector figure (spec); no fp64 matrix rate is documented
HBM_BYTES_PER_S = 6.29e12     # measured


class StepTimeout(Exception):
    pass


def limited(seconds, fn, *a, **kw):
    def on_alarm(signum, frame):
        raise StepTimeout(f"step exceeded {seconds} s")
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    try:
        return fn(*a, **kw)
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def summary(out):
    return {"median_s": statistics.median(out), "min_s": min(out), "max_s": max(out), "all_s": out}


def timed(fn, sync, warmup=1, reps=5):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return summary(out)


def alternating(fn_a, fn_b, sync, warmup=1, reps=5):
    """a, b, a, b, ...: both under the same drift of the box."""
    out = ([], [])
    for i in range(warmup + reps):
        for k, fn in enumerate((fn_a, fn_b)):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if i >= warmup:
                out[k].append(time.perf_counter() - t0)
    return summary(out[0]), summary(out[1])


def by_events(fn, torch, warmup=1, reps=5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for i in range(warmup + reps):
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        if i >= warmup:
            out.append(ev[0].elapsed_time(ev[1]) * 1e-3)
    return summary(out)


def host_sliced(np, real_dev, fake_dev, theta_dev):
    """The host formulation of the joint segment: seconds per part and the swd."""
    from scipy.stats import wasserstein_distance
    t0 = time.perf_counter()
    real, fake, theta = real_dev.cpu().numpy(), fake_dev.cpu().numpy(), theta_dev.cpu().numpy()
    t1 = time.perf_counter()
    n = real.shape[0]
    pr = real.reshape(n, -1).astype(np.float64) @ theta.T
    pf = fake.reshape(fake.shape[0], -1).astype(np.float64) @ theta.T
    t2 = time.perf_counter()
    w = [wasserstein_distance(pr[:, p], pf[:, p]) for p in range(theta.shape[0])]
    t3 = time.perf_counter()
    return {"copy_out_s": t1 - t0, "fp64_product_s": t2 - t1, "scipy_per_direction_s": t3 - t2, "seconds": t3 - t0,
            "swd": float(np.mean(w)), "swd_max": float(np.max(w))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--proj", type=int, default=256)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="skip the evaluate_device figures")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("sliced_bench needs a HIP device (no CPU fallback)")
    from expertsim.train import sliced as S
    from expertsim.train.utils import wasserstein_1d_device
    from expertsim.segments import expert_segments
    from expertsim.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    N, P = args.n, args.proj
    sync = torch.cuda.synchronize
    batch = limited(args.step_limit, make_batch, N, "neutron", seed=11)
    real_img = torch.from_numpy(batch["real_images"]).to(dev)
    fake_img = torch.from_numpy(limited(args.step_limit, make_batch, N, "neutron", seed=12)["real_images"]).to(dev)
    H, W = int(real_img.shape[-2]), int(real_img.shape[-1])
    D = H * W
    theta = S.directions(P, D, seed=1)
    flops, image_bytes = 2.0 * N * D * P, 4.0 * N * D
    res = {"n": N, "h": H, "w": W, "d": D, "n_proj": P, "device": torch.cuda.get_device_name(0), "warmup": 1, "reps": 5,
           "fp64_figure_flops": FP64_FLOPS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "note": "one run on one box"}
    out_r = torch.empty(N, P, dtype=torch.float64, device=dev)
    pr = limited(args.step_limit, by_events, lambda: S.project(real_img, theta, out=out_r), torch)
    t = pr["median_s"]
    t_flops, t_bytes = flops / FP64_FLOPS, image_bytes / HBM_BYTES_PER_S
    pr.update(flops=flops, image_bytes=image_bytes, flops_per_s=flops / t,
              share_of_78_6_tflops_fp64_vector_figure=flops / t / FP64_FLOPS,
              image_bytes_per_s=image_bytes / t, share_of_hbm_rate=image_bytes / t / HBM_BYTES_PER_S,
              least_time_by_flops_s=t_flops, least_time_by_bytes_s=t_bytes,
              larger_bound="flops" if t_flops > t_bytes else "bytes",
              fp64_matrix_rate="not documented for this chip: the share above is against the fp64 vector figure")
    res["sliced_project_events"] = pr
    res["sliced_directions_events"] = limited(args.step_limit, by_events, lambda: S.directions(P, D, seed=1), torch)
    out_f = S.project(fake_img, theta).clone()
    rs = np.random.RandomState(20261021)
    experts = {1: torch.zeros(N, dtype=torch.int32, device=dev),
               4: torch.from_numpy(rs.randint(0, 4, N).astype(np.int32)).to(dev)}
    for E, expert in experts.items():
        perm, seg, _ = expert_segments(expert, E, N, dev, joint=True)
        one = {"problems": (E + 1) * P}
        one["wasserstein_1d_events"] = limited(
            args.step_limit, by_events,
            lambda: wasserstein_1d_device(out_r, out_f, seg, seg, perm, perm, u_cap=N, v_cap=N), torch)
        one["sliced_end_to_end"] = limited(args.step_limit, timed,
                                           lambda: S.sliced(real_img, fake_img, expert, E, n_proj=P, seed=1), sync)
        one["values"] = S.sliced(real_img, fake_img, expert, E, n_proj=P, seed=1)
        res[f"E{E}"] = one

    if not args.no_model:
        from expertsim.config import load_config
        from expertsim.train.loop import setup_moe_system
        cond = torch.from_numpy(batch["cond"]).to(dev)
        for E in experts:
            cfg = load_config(overrides=["model.architecture=neutron", f"dataset.input_image_shape=[{H},{W}]",
                                         f"model.n_experts={E}", "train.precision=fp32"])
            torch.manual_seed(4)
            moe = setup_moe_system(cfg, dev)
            moe.eval()
            off, on = limited(2 * args.step_limit, alternating,
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1),
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1, sliced=True, sliced_proj=P),
                              sync)
            res[f"E{E}"]["evaluate_device"] = {"without": off, "with_sliced": on, "order": "alternating",
                                               "added_median_s": on["median_s"] - off["median_s"],
                                               "ranges_disjoint": on["min_s"] > off["max_s"]}

    if not args.no_baseline:
        host = limited(args.step_limit, host_sliced, np, real_img, fake_img, theta)
        host.update(how="copy of both image sets and the directions out, fp64 X @ theta.T of both sides, "
                        "scipy.stats.wasserstein_distance per direction; the joint segment only; host, at most 16 "
                        "threads, one run", runs=1)
        res["host_baseline"] = host
        res["ranges_disjoint"] = {f"E{E}_sliced_vs_host": res[f"E{E}"]["sliced_end_to_end"]["max_s"] < host["seconds"]
                                  for E in experts}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
