"""Timing of the device k-means (expertsim/utils/clustering.py) on one device, against scikit-learn on the host.

    python tools/cluster_bench.py [--n 131072] [--out profiles/cluster.json]

One process, 2 warm-up + 7 timed runs per device figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: proton 56x30 structured images (one Gaussian spot per image
at one of four mode positions plus jitter, Poisson counts, log1p, fp32; drawn on the device from a seed),
N = 2^17, K = 4, resident on the device.

Timed: (1) one Lloyd iteration, es_kmeans_assign + es_kmeans_update, by device events, and each call alone;
N cols 4 bytes of x over that time is reported as a share of the achievable HBM rate -- the iteration reads x
TWICE (once per call), so the memory system moves twice the reported figure; (2)
kmeans(n_init=10) end to end, the per-iteration host copies included; (3) prepare_dataset from host images
with and without n_clusters=4 (the upload included, no file I/O).
Baseline, one run each: sklearn.cluster.KMeans(algorithm="lloyd") on the box's host, for fp64 and for fp32 input
-- the fp32 run is scikit-learn's fast mode (fp32 arithmetic), NOT the same arithmetic as the device's fp64 --
from the same initial centres (n_init=1; time per iteration = total / n_iter_) and with init="k-means++",
n_init=10 end to end.
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

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12


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


def timed(fn, sync, warmup=2, reps=7):
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


def by_events(fn, torch, warmup=2, reps=7):
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


def spot_images(torch, n, h, w, K, seed, dev, chunk=8192):
    g = torch.Generator(device=dev).manual_seed(seed)
    modes = torch.stack([torch.rand(K, generator=g, device=dev) * 0.6 * h + 0.2 * h,
                         torch.rand(K, generator=g, device=dev) * 0.6 * w + 0.2 * w], dim=1)
    yy = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    xx = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    out = torch.empty(n, h, w, dtype=torch.float32, device=dev)
    for lo in range(0, n, chunk):
        m = min(chunk, n - lo)
        which = torch.randint(0, K, (m,), generator=g, device=dev)
        centre = modes[which] + 1.5 * torch.randn(m, 2, generator=g, device=dev)
        width = 1.5 + 1.5 * torch.rand(m, generator=g, device=dev)
        amp = torch.exp(torch.log(torch.tensor(40.0, device=dev)) + 0.5 * torch.randn(m, generator=g, device=dev))
        r2 = (yy - centre[:, 0, None, None]) ** 2 + (xx - centre[:, 1, None, None]) ** 2
        lam = amp[:, None, None] * torch.exp(-0.5 * r2 / width[:, None, None] ** 2)
        out[lo:lo + m] = torch.log1p(torch.poisson(lam, generator=g))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 17)
    ap.add_argument("--seed", type=int, default=20261021)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("cluster_bench needs a HIP device (no CPU fallback)")
    from expertsim.utils import clustering as CL
    from expertsim.utils import data_preparation as DP
    from expertsim.utils.data_transformations import COND_COLUMNS
    dev = torch.device("cuda", 0)
    N, H, W, K = args.n, 56, 30, 4
    sync = torch.cuda.synchronize
    images = limited(args.step_limit, spot_images, torch, N, H, W, K, args.seed, dev)
    x = images.reshape(N, H * W)
    nbytes = N * H * W * 4
    res = {"n": N, "shape": [H, W], "K": K, "dtype": "float32", "seed": args.seed, "device": torch.cuda.get_device_name(0),
           "warmup": 2, "reps": 7, "x_bytes": nbytes, "note": "one run on one box"}

    u = np.random.Generator(np.random.Philox(key=[0, 0])).random((K, CL.kmeans_trials(K)))
    init, _ = CL.kmeans_plusplus_raw(x, K, u)
    run = CL._Lloyd(x, K)
    run.assign(init, run.labels[0], None)
    c_new = torch.empty_like(init)

    def iteration():
        run.assign(init, run.labels[0], run.labels[1])
        run.update(run.labels[0], init, c_new)

    res["lloyd_iteration_events"] = limited(args.step_limit, by_events, iteration, torch)
    res["assign_events"] = limited(args.step_limit, by_events,
                                   lambda: run.assign(init, run.labels[0], run.labels[1]), torch)
    res["update_events"] = limited(args.step_limit, by_events, lambda: run.update(run.labels[0], init, c_new), torch)
    res["plusplus_events"] = limited(args.step_limit, by_events, lambda: CL.kmeans_plusplus_raw(x, K, u), torch)
    for k in ("lloyd_iteration_events", "assign_events", "update_events"):
        res[k]["x_bytes_per_s"] = nbytes / res[k]["median_s"]
        res[k]["share_of_hbm_achievable"] = res[k]["x_bytes_per_s"] / HBM_ACHIEVABLE
    res["lloyd_iteration_events"]["x_reads_per_iteration"] = 2

    single = CL.kmeans_raw(x, init)
    res["kmeans_raw_n_iter"] = int(single[3])
    res["kmeans_raw"] = limited(args.step_limit, timed, lambda: CL.kmeans_raw(x, init), sync)
    best = CL.kmeans(x, K, n_init=10, seed=0)
    res["kmeans_n_init10_inertia"] = float(best[2])
    res["kmeans_n_init10"] = limited(args.step_limit, timed, lambda: CL.kmeans(x, K, n_init=10, seed=0), sync)

    import pandas as pd
    rs = np.random.RandomState(1)
    cond = np.repeat(rs.randint(0, 4, (N // 4, 9)).astype(np.float64), 4, axis=0)
    cond[:, 0] += np.repeat(np.arange(N // 4), 4)
    frame = pd.DataFrame(cond, columns=COND_COLUMNS)
    host = images.cpu().numpy()
    res["prepare_without_clusters"] = limited(args.step_limit, timed,
                                              lambda: DP.prepare_dataset(host, frame, "proton"), sync)
    res["prepare_with_clusters"] = limited(args.step_limit, timed,
                                           lambda: DP.prepare_dataset(host, frame, "proton", n_clusters=K), sync)

    if not args.no_baseline:
        from sklearn.cluster import KMeans
        init_host = init.cpu().numpy()
        base = {"how": "sklearn.cluster.KMeans(algorithm='lloyd'), host, at most 16 threads, one run each",
                "fp32_note": "fp32 input is scikit-learn's fast mode (fp32 arithmetic): not the device's arithmetic"}
        for name, dtype in (("fp64", np.float64), ("fp32", np.float32)):
            X = host.reshape(N, H * W).astype(dtype)

            def one():
                t0 = time.perf_counter()
                km = KMeans(n_clusters=K, init=init_host.astype(dtype), n_init=1, algorithm="lloyd").fit(X)
                return time.perf_counter() - t0, km

            def ten():
                t0 = time.perf_counter()
                km = KMeans(n_clusters=K, init="k-means++", n_init=10, algorithm="lloyd", random_state=0).fit(X)
                return time.perf_counter() - t0, km

            s1, km1 = limited(args.step_limit, one)
            s10, km10 = limited(args.step_limit, ten)
            base[name] = {"same_init_s": s1, "same_init_n_iter": int(km1.n_iter_), "per_iteration_s": s1 / km1.n_iter_,
                          "same_init_inertia": float(km1.inertia_), "n_init10_s": s10,
                          "n_init10_inertia": float(km10.inertia_), "runs": 1}
            if name == "fp64":
                base[name]["labels_equal_device"] = bool(np.array_equal(km1.labels_, single[0].cpu().numpy()))
                base[name]["n_iter_equal_device"] = bool(int(km1.n_iter_) == int(single[3]))
            del X
        res["host_baseline"] = base
        res["ranges_disjoint"] = {
            "iteration_vs_host_fp64": res["lloyd_iteration_events"]["max_s"] < base["fp64"]["per_iteration_s"],
            "iteration_vs_host_fp32": res["lloyd_iteration_events"]["max_s"] < base["fp32"]["per_iteration_s"],
            "n_init10_vs_host_fp64": res["kmeans_n_init10"]["max_s"] < base["fp64"]["n_init10_s"],
            "n_init10_vs_host_fp32": res["kmeans_n_init10"]["max_s"] < base["fp32"]["n_init10_s"],
            "prepare_with_vs_without_clusters": res["prepare_without_clusters"]["max_s"]
            < res["prepare_with_clusters"]["min_s"]}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
