"""Timing of the device precision / recall / density / coverage (expertsim/train/fidelity.py) on one device, against
the `prdc` formulation on scikit-learn on the host.

    python tools/fidelity_bench.py [--n 16384] [--out profiles/fidelity.json]

One process, 1 warm-up + 5 timed runs per device figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: neutron 44x44 fp32 synthetic images, N real (seed 11) against N
generated (seed 12, the first half +-2 % perturbations of four of its rows: a half-collapsed generator), k = 5,
resident on the device; E = 1 (the joint segment and one expert holding everything: every pair twice) and E = 4
(a seeded uniform expert vector: the joint segment and four quarters).

Timed per E: es_knn_radius alone (the real side), es_prdc_count alone (radii given), by device events, and prdc()
end to end (the dispatch, both radii, the counts and the one device-to-host copy of the totals) by the host clock
around a synchronise.  pairs x cols x 3 fp64 operations (subtract, multiply, add: the contract allows no FMA) over
the kernel time is reported as a share of the fp64 vector peak counted in instructions: 78.6 TFLOP/s (spec, FMA
= 2) is 39.3e12 lane-instructions/s.
Baseline, one timed run: the `prdc` package's formulation at the same N on the host -- three
sklearn.metrics.pairwise_distances in fp64, np.partition, the four reductions -- for the joint segment only (the
device's E = 1 figure does twice that work).
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

FP64_VECTOR_FLOPS = 78.6e12                  # spec, an FMA counted as two
FP64_VECTOR_INSTR = FP64_VECTOR_FLOPS / 2    # lane-instructions per second


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


def inputs(np, n, seed=20261021):
    from expertsim.utils.synthetic import make_batch
    real = make_batch(n, "neutron", seed=11)["real_images"].reshape(n, -1)
    fake = make_batch(n, "neutron", seed=12)["real_images"].reshape(n, -1).copy()
    rs = np.random.RandomState(seed)
    half = n // 2
    base = fake[half:half + 4].astype(np.float64)
    noise = 1.0 + 0.02 * rs.uniform(-1.0, 1.0, (half, fake.shape[1]))
    fake[:half] = np.clip(base[np.arange(half) % 4] * noise, 0.0, None).astype(np.float32)
    return real, fake, rs


def host_prdc(np, real, fake, k):
    from sklearn.metrics import pairwise_distances
    real, fake = real.astype(np.float64), fake.astype(np.float64)

    def kth(x):
        d = pairwise_distances(x, metric="euclidean", n_jobs=None)
        return np.partition(d, k, axis=-1)[:, :k + 1].max(axis=-1)

    r_nn, f_nn = kth(real), kth(fake)
    d = pairwise_distances(real, fake, metric="euclidean")
    inside = d < r_nn[:, None]
    return [int(inside.any(axis=0).sum()), int((d < f_nn[None, :]).any(axis=1).sum()), int(inside.sum()),
            int((d.min(axis=1) < r_nn).sum())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("fidelity_bench needs a HIP device (no CPU fallback)")
    from expertsim.train import fidelity as FD
    dev = torch.device("cuda", 0)
    N, k = args.n, args.k
    sync = torch.cuda.synchronize
    real_h, fake_h, rs = limited(args.step_limit, inputs, np, N)
    cols = real_h.shape[1]
    real, fake = torch.from_numpy(real_h).to(dev), torch.from_numpy(fake_h).to(dev)
    res = {"n": N, "cols": cols, "k": k, "dtype": "float32", "device": torch.cuda.get_device_name(0), "warmup": 1,
           "reps": 5, "fp64_vector_peak_instr_per_s": FP64_VECTOR_INSTR, "ops_per_pair_element": 3,
           "note": "one run on one box"}
    experts = {1: torch.zeros(N, dtype=torch.int32, device=dev),
               4: torch.from_numpy(rs.randint(0, 4, N).astype(np.int32)).to(dev)}
    for E, expert in experts.items():
        perm, seg, _ = FD.expert_segments(expert, E, N, dev, joint=True)
        seg_h = seg.cpu().numpy().astype(np.int64)
        pairs = int(((seg_h[:, 1] - seg_h[:, 0]) ** 2).sum())          # both sides share the segments
        ops = 3.0 * pairs * cols
        r_rad = FD.knn_radius(real, k, perm, seg, N)
        f_rad = FD.knn_radius(fake, k, perm, seg, N)
        one = {"segments": seg_h.tolist(), "pairs_per_matrix": pairs, "fp64_ops_per_matrix": ops}
        one["knn_radius_events"] = limited(args.step_limit, by_events,
                                           lambda: FD.knn_radius(real, k, perm, seg, N, out=r_rad), torch)
        one["prdc_count_events"] = limited(
            args.step_limit, by_events,
            lambda: FD.prdc_raw(real, fake, k, perm, seg, N, perm, seg, N, r_radius2=r_rad, f_radius2=f_rad,
                                per_row=False), torch)
        for key in ("knn_radius_events", "prdc_count_events"):
            one[key]["fp64_ops_per_s"] = ops / one[key]["median_s"]
            one[key]["share_of_fp64_vector_peak"] = one[key]["fp64_ops_per_s"] / FP64_VECTOR_INSTR
        one["prdc_end_to_end"] = limited(args.step_limit, timed,
                                         lambda: FD.prdc(real, fake, k=k, expert=expert, n_experts=E), sync)
        one["prdc_end_to_end"]["share_of_fp64_vector_peak"] = 3 * ops / one["prdc_end_to_end"]["median_s"] / FP64_VECTOR_INSTR
        m = FD.prdc(real, fake, k=k, expert=expert, n_experts=E, details=True)
        one["totals"] = m["totals"].cpu().numpy().tolist()
        one["metrics"] = {key: v for key, v in m.items() if isinstance(v, float)}
        res[f"E{E}"] = one

    if not args.no_baseline:
        t0 = time.perf_counter()
        host = limited(args.step_limit, host_prdc, np, real_h, fake_h, k)
        dt = time.perf_counter() - t0
        joint = res["E1"]["totals"][0][3:7]
        res["host_baseline"] = {"how": "three sklearn.metrics.pairwise_distances (fp64, euclidean), np.partition and "
                                       "the four reductions of prdc.compute_prdc; the joint segment only; host, at "
                                       "most 16 threads, one run", "seconds": dt, "runs": 1, "totals": host,
                                "totals_equal_device": host == joint}
        res["ranges_disjoint"] = {f"E{E}_end_to_end_vs_host": res[f"E{E}"]["prdc_end_to_end"]["max_s"] < dt
                                  for E in experts}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
