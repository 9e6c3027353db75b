"""Timing of the expert diagnostics (expertsim/train/diagnostics.py) on one device.

    python tools/diagnostics_bench.py [--n 16384] [--out profiles/diagnostics.json]

One process, 2 warm-up + 7 timed calls per figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: the neutron model with E = 4 experts (fresh weights), N
synthetic conditions already on the device (utils.synthetic.make_batch; the last two columns, mass and charge
in the reference, quantised to three values each, so that whole waves meet in one bin), routed and simulated
once outside the timed region: the expert vector and the photon sums of the generated images are resident.

Timed: (1) expert_diagnostics() on the resident inputs -- one dispatch, three histogram calls, one KDE call,
torch.unique and the one copy out; (2) es_segment_histogram over the [N, 9] conditions (right = 1, 50 bins)
and es_segment_kde over the 8 continuous columns (100 points) alone, by device events; (3) the reference's
formulation on the host, which is the baseline: the device-to-host copies of the conditions and the photon
sums, then per expert np.histogram of the photon sums, per expert and variable pd.cut(include_lowest=True)
counts, per expert and continuous variable scipy.stats.gaussian_kde(bw_method='scott') on the 100-point
grid (skipped below 5 samples or 1e-12 standard deviation), and the counts per value of the last variable.
No speed-up is promised: the ranges are reported, and whether they are disjoint.
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


def by_events(fn, warmup=2, reps=7):
    import torch
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


def host_reference(cond_dev, ps_dev, expert_dev, E, bins, points):
    """The reference's formulation: copies out, then numpy / pandas / scipy per expert and variable."""
    import numpy as np
    import pandas as pd
    from scipy.stats import gaussian_kde
    cond = cond_dev.cpu().numpy().astype(np.float64)
    ps = ps_dev.cpu().numpy()
    expert = expert_dev.cpu().numpy()
    C = cond.shape[1]
    edges = np.linspace(ps.min(), ps.max(), bins + 1)
    out = {"photon_sum_hist": [np.histogram(ps[expert == e], bins=edges)[0] for e in range(E)]}
    cuts = [np.linspace(cond[:, c].min(), cond[:, c].max(), bins + 1) for c in range(C)]
    hist = np.zeros((E, C, bins), dtype=np.int64)
    kde = np.full((E, C - 1, points), np.nan)
    for c in range(C):
        lo, hi = cond[:, c].min(), cond[:, c].max()
        if lo == hi:
            lo, hi = lo - 1e-6, hi + 1e-6
        grid = np.linspace(lo, hi, points)
        for e in range(E):
            d = cond[expert == e, c]
            if len(np.unique(cuts[c])) == bins + 1:
                codes = pd.cut(d, bins=cuts[c], include_lowest=True, labels=False)
                hist[e, c] = np.bincount(codes[~np.isnan(codes)].astype(np.int64), minlength=bins)
            if c < C - 1 and len(d) >= 5 and np.std(d) >= 1e-12:
                kde[e, c] = gaussian_kde(d, bw_method="scott")(grid)
    values = np.unique(cond[:, -1])
    out.update(cond_hist=hist, cond_kde=kde,
               cat_count=[[int((cond[expert == e, -1] == v).sum()) for v in values] for e in range(E)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--experts", type=int, default=4)
    ap.add_argument("--seed", type=int, default=20261020)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("diagnostics_bench needs a HIP device (no CPU fallback)")
    from expertsim.config import load_config
    from expertsim.train import diagnostics as D
    from expertsim.train.loop import setup_moe_system
    from expertsim.utils.data_preparation import photon_sums_and_peaks
    from expertsim.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    N, E, bins, points = args.n, args.experts, 50, 100
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", "train.precision=fp32"])
    torch.manual_seed(args.seed)
    moe = setup_moe_system(cfg, dev)
    moe.eval()
    cond = make_batch(N, "neutron", seed=args.seed % (2 ** 31))["cond"].astype(np.float32)
    cond[:, -2:] = np.sign(np.round(cond[:, -2:] / (np.abs(cond[:, -2:]).max(axis=0) + 1e-30) * 1.49))
    cond_dev = torch.from_numpy(cond).to(dev)
    sim = limited(args.step_limit, moe.simulate, cond_dev, seed=args.seed, domain="photons")
    expert = sim["expert"]
    ps, _ = photon_sums_and_peaks(sim["images"], check=False)
    del sim
    sync = torch.cuda.synchronize
    sync()
    C = cond.shape[1]
    counts = torch.bincount(expert.long(), minlength=E).cpu().tolist()
    res = {"n": N, "experts": E, "cond_columns": C, "bins": bins, "points": points, "seed": args.seed,
           "expert_counts": counts, "distinct_values_last_two_columns": [int(len(np.unique(cond[:, c]))) for c in (-2, -1)],
           "device": torch.cuda.get_device_name(0), "warmup": 2, "reps": 7}
    res["expert_diagnostics_resident"] = limited(
        args.step_limit, timed, lambda: D.expert_diagnostics(cond_dev, expert, E, ps, bins=bins, points=points), sync)
    perm, seg, _ = D.expert_segments(expert, E, N, dev)
    res["es_segment_histogram_events"] = limited(
        args.step_limit, by_events, lambda: D.segment_histogram_raw(cond_dev, seg, perm, None, bins, True))
    res["es_segment_kde_events"] = limited(
        args.step_limit, by_events, lambda: D.segment_kde_raw(cond_dev, seg, perm, None, points, cols=C - 1))
    exps = N * points * (C - 1)
    res["es_segment_kde_events"]["exponentials"] = exps
    res["es_segment_kde_events"]["exponentials_per_s"] = exps / res["es_segment_kde_events"]["median_s"]
    try:
        res["host_reference"] = limited(args.step_limit * 4, timed,
                                        lambda: host_reference(cond_dev, ps, expert, E, bins, points), sync)
        res["host_reference"]["how"] = "D2H copies, np.histogram, pd.cut, scipy gaussian_kde per expert and variable"
        res["ranges_disjoint"] = {
            "resident_vs_host_reference":
                res["expert_diagnostics_resident"]["max_s"] < res["host_reference"]["min_s"]
                or res["host_reference"]["max_s"] < res["expert_diagnostics_resident"]["min_s"]}
        # the two paths compute the same thing
        mine = D.expert_diagnostics(cond_dev, expert, E, ps, bins=bins, points=points)
        host = host_reference(cond_dev, ps, expert, E, bins, points)
        res["agreement"] = {
            "photon_sum_hist_equal": bool(np.array_equal(mine["photon_sum_hist"], np.stack(host["photon_sum_hist"]))),
            "cond_hist_equal": bool(np.array_equal(mine["cond_hist"], host["cond_hist"])),
            "cat_count_equal": bool(np.array_equal(mine["cat_count"], np.asarray(host["cat_count"]))),
            "cond_kde_max_rel": float(np.nanmax(np.abs(mine["cond_kde"] - host["cond_kde"])
                                                / np.maximum(np.abs(host["cond_kde"]), 1e-300))),
            "cond_kde_valid_equal": bool(np.array_equal(np.isnan(mine["cond_kde"]), np.isnan(host["cond_kde"])))}
    except ImportError as e:
        res["host_reference"] = {"unavailable": str(e)}
    res["note"] = "one run on one box"
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
