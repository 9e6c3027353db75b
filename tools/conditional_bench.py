"""Timing of the device conditional profile (expertsim/train/conditional.py) on one device, against the host
formulation (np.quantile, np.searchsorted, scipy's wasserstein_distance and ks_2samp per bin and observable).

    python tools/conditional_bench.py [--n 16384] [--bins 8] [--out profiles/conditional.json]

One process, 1 warm-up + 5 timed runs per device figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: neutron 44x44 fp32 synthetic images, N real (seed 11) against N
generated (seed 12), their ten observables (train.distances.observables) resident on the device, binned by column 0
of the conditions (the energy); E = 1 (one expert holding everything) and E = 4 (a seeded uniform expert vector).

Timed per E, by device events: es_segment_quantiles alone over the 1 + (1 + E) x bins segments of the profile,
es_bin_dispatch alone over the (expert, bin) classes, and es_router_dispatch on the same class vector (the kernel
es_bin_dispatch stands in for: one workgroup that walks all rows once per class; it takes the classes as given, so
the figure leaves the binning out); profile() end to end by the host clock around a synchronise; then
MoEWrapper.evaluate_device of a freshly initialised model at epoch 0 with conditional=True and without, the two
ALTERNATING in one process, the difference of the medians being the added cost.
Baseline, ONE timed run on the host, the joint bins only: the copy of both tables and the column out, np.quantile
edges, np.searchsorted, then per bin and observable np.quantile (three probabilities, both sides), scipy's
wasserstein_distance and ks_2samp; its cond_ws is compared with the device's.
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


def alternating(fn_off, fn_on, sync, warmup=1, reps=5):
    for _ in range(warmup):
        fn_off()
        fn_on()
    sync()
    off, on = [], []
    for _ in range(reps):
        for fn, out in ((fn_off, off), (fn_on, on)):
            t0 = time.perf_counter()
            fn()
            sync()
            out.append(time.perf_counter() - t0)
    return summary(off), summary(on)


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


def host_profile(np, real_dev, fake_dev, by_dev, n_bins, probs):
    """The host formulation of the joint bins: seconds per part and cond_ws_<column> / cond_ws."""
    from scipy.stats import ks_2samp, wasserstein_distance
    t0 = time.perf_counter()
    real, fake, by = real_dev.cpu().numpy(), fake_dev.cpu().numpy(), by_dev.cpu().numpy().astype(np.float64)
    t1 = time.perf_counter()
    edges = np.quantile(by, [k / n_bins for k in range(1, n_bins)])
    bins = np.searchsorted(edges, by, side="left")
    t2 = time.perf_counter()
    cols = real.shape[1]
    n = np.bincount(bins, minlength=n_bins)
    ws, ks = np.zeros((n_bins, cols)), np.zeros((n_bins, cols))
    tq = tw = tk = 0.0
    for b in range(n_bins):
        r, f = real[bins == b], fake[bins == b]
        for c in range(cols):
            a = time.perf_counter()
            np.quantile(r[:, c], probs), np.quantile(f[:, c], probs)
            q = time.perf_counter()
            ws[b, c] = wasserstein_distance(r[:, c], f[:, c])
            w = time.perf_counter()
            ks[b, c] = ks_2samp(r[:, c], f[:, c]).statistic
            tq, tw, tk = tq + q - a, tw + w - q, tk + time.perf_counter() - w
    q_all = np.quantile(real, [probs[0], probs[2]], axis=0)
    scale = (q_all[1] - q_all[0]) / 2.0
    scale = np.where(scale == 0, 1.0, scale)
    cond_ws_cols = (n[:, None] * ws).sum(axis=0) / n.sum()
    t3 = time.perf_counter()
    return {"copy_out_s": t1 - t0, "edges_and_bins_s": t2 - t1, "np_quantile_s": tq, "wasserstein_distance_s": tw,
            "ks_2samp_s": tk, "seconds": t3 - t0, "cond_ws": float((cond_ws_cols / scale).mean()),
            "cond_ws_columns": cond_ws_cols.tolist(),
            "cond_ks_columns": ((n[:, None] * ks).sum(axis=0) / n.sum()).tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--bins", type=int, default=8)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="skip the evaluate_device figures")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("conditional_bench needs a HIP device (no CPU fallback)")
    from expertsim import hip
    from expertsim.train import conditional as K
    from expertsim.train import distances as D
    from expertsim.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    N, B = args.n, args.bins
    sync = torch.cuda.synchronize
    batch = limited(args.step_limit, make_batch, N, "neutron", seed=11)
    real_img = torch.from_numpy(batch["real_images"]).to(dev)
    fake_img = torch.from_numpy(limited(args.step_limit, make_batch, N, "neutron", seed=12)["real_images"]).to(dev)
    obs_real, obs_gen = D.observables(real_img), D.observables(fake_img)
    cond = torch.from_numpy(batch["cond"]).to(dev)
    by = cond[:, 0]
    rs = np.random.RandomState(20261021)
    res = {"n": N, "cols": int(obs_real.shape[1]), "bins": B, "probs": list(K.PROBS),
           "device": torch.cuda.get_device_name(0), "warmup": 1, "reps": 5, "note": "one run on one box"}
    experts = {1: torch.zeros(N, dtype=torch.int32, device=dev),
               4: torch.from_numpy(rs.randint(0, 4, N).astype(np.int32)).to(dev)}
    names = D.OBSERVABLE_NAMES
    for E, expert in experts.items():
        raw = K.profile_device(obs_real, obs_gen, by, B, expert, E)
        real2 = torch.cat([obs_real, obs_real])
        fake2 = torch.cat([obs_gen, obs_gen])
        seg, idx = raw["seg"], raw["idx"]
        one = {"segments": int(seg.shape[0]), "classes": E * B,
               "count": raw["count"].cpu().numpy().tolist(),
               "quantile_workspace_bytes": hip.segment_quantiles_workspace(int(seg.shape[0]), 10, N, N),
               "padded_problem": 2 * N if 2 * N > hip.WS_LDS_MAX else None}
        one["segment_quantiles_events"] = limited(
            args.step_limit, by_events,
            lambda: K.segment_quantiles(real2, fake2, K.PROBS, idx, seg, N, idx, seg, N), torch)
        edges = raw["edges"]
        out3 = K.bin_dispatch(by, edges, B, expert, E)
        one["bin_dispatch_events"] = limited(args.step_limit, by_events,
                                             lambda: K.bin_dispatch(by, edges, B, expert, E, out=out3), torch)
        cls = (expert * B + raw["bin"]).to(torch.int32).contiguous()
        perm, offs = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(E * B + 1, dtype=torch.int32, device=dev)
        one["router_dispatch_events"] = limited(
            args.step_limit, by_events,
            lambda: hip.call("es_router_dispatch", hip.ptr(cls), N, E * B, hip.ptr(perm), hip.ptr(offs),
                             hip.stream_ptr()), torch)
        one["dispatches_agree"] = bool(torch.equal(perm, out3[1]) and torch.equal(offs, out3[2]))
        one["profile_end_to_end"] = limited(args.step_limit, timed,
                                            lambda: K.profile(obs_real, obs_gen, by, B, expert, E, names=names), sync)
        one["values"] = K.profile(obs_real, obs_gen, by, B, expert, E, names=names)
        res[f"E{E}"] = one

    if not args.no_model:
        from expertsim.config import load_config
        from expertsim.train.loop import setup_moe_system
        for E in experts:
            cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                         f"model.n_experts={E}", "train.precision=fp32"])
            torch.manual_seed(4)
            moe = setup_moe_system(cfg, dev)
            moe.eval()
            off, on = limited(args.step_limit, alternating,
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1),
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1, conditional=True,
                                                          conditional_bins=B), sync)
            res[f"E{E}"]["evaluate_device"] = {"without": off, "with_conditional": on, "alternating": True,
                                               "added_median_s": on["median_s"] - off["median_s"],
                                               "ranges_disjoint": on["min_s"] > off["max_s"]}

    if not args.no_baseline:
        host = limited(args.step_limit, host_profile, np, obs_real, obs_gen, by, B, K.PROBS)
        host.update(how="copy of both [N, 10] fp64 tables and the column out, np.quantile edges, np.searchsorted, per "
                        "bin and observable np.quantile, wasserstein_distance and ks_2samp; the joint bins only; host, "
                        "at most 16 threads, one run", runs=1)
        dev_ws = res["E1"]["values"]["cond_ws"]
        host["cond_ws_device"] = dev_ws
        host["cond_ws_relative_difference"] = abs(dev_ws - host["cond_ws"]) / abs(host["cond_ws"])
        res["host_baseline"] = host
        res["ranges_disjoint"] = {f"E{E}_profile_vs_host": res[f"E{E}"]["profile_end_to_end"]["max_s"] < host["seconds"]
                                  for E in experts}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
