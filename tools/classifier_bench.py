"""Timing of the device classifier two-sample test (expertsim/train/classifier.py) on one device, against the host
formulation (scikit-learn's LogisticRegression(newton-cholesky), roc_auc_score, scipy's ks_2samp).

    python tools/classifier_bench.py [--n 16384] [--out profiles/classifier.json]

One process, 1 warm-up + 5 timed runs per device figure, median [min, max]; every step under its own time limit
(SIGALRM) and at most 16 host threads.  Workload: neutron 44x44 fp32 synthetic images, N real (seed 11) against N
generated (seed 12), their ten observables (train.distances.observables) resident on the device, degree 2 (65
features); E = 1 (the joint segment and one expert holding everything) and E = 4 (a seeded uniform expert vector).

Timed per E: es_logit_fit alone over all E + 1 training halves (with its iteration counts and the time per pass: the
fit always issues its 1 + 2 (max_iter + 1) launches, so the figure is also taken at max_iter = the iterations the
problems needed, which bounds what the early-out launches cost), es_logit_scores and es_rank_stats alone over the
held-out halves, by device events, and c2st() end to end by the host clock around a synchronise; then
MoEWrapper.evaluate_device of a freshly initialised model at epoch 0 with classifier=True and without, the two
ALTERNATING in one process, the difference of the medians being the added cost.
Baseline, ONE timed run on the host, the joint segment only: the copy of both feature tables out,
LogisticRegression(C=1, solver="newton-cholesky", tol=1e-9 -- on scikit-learn's gradient scale) on the training half,
roc_auc_score and ks_2samp on the held-out scores.
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


def host_c2st(np, xr_dev, xf_dev):
    """The host formulation of the joint segment: seconds per part and the values."""
    from scipy.stats import ks_2samp
    from sklearn.linear_model import LogisticRegression
    from sklearn.metrics import roc_auc_score
    t0 = time.perf_counter()
    xr, xf = xr_dev.cpu().numpy(), xf_dev.cpu().numpy()
    t1 = time.perf_counter()
    n = len(xr)
    h = (n + 1) // 2
    X = np.concatenate([xr[:h], xf[:h]])
    y = np.concatenate([np.ones(h), np.zeros(h)])
    clf = LogisticRegression(C=1.0, solver="newton-cholesky", tol=1e-9, max_iter=100).fit(X, y)
    t2 = time.perf_counter()
    sr, sf = clf.decision_function(xr[h:]), clf.decision_function(xf[h:])
    auc = roc_auc_score(np.concatenate([np.ones(len(sr)), np.zeros(len(sf))]), np.concatenate([sr, sf]))
    t3 = time.perf_counter()
    ks = ks_2samp(sr, sf).statistic
    t4 = time.perf_counter()
    return {"copy_out_s": t1 - t0, "logistic_regression_s": t2 - t1, "roc_auc_score_s": t3 - t2, "ks_2samp_s": t4 - t3,
            "seconds": t4 - t0, "n_iter": int(clf.n_iter_[0]), "auc": float(auc), "ks": float(ks)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--no-model", action="store_true", help="skip the evaluate_device figures")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    torch.set_num_threads(min(16, torch.get_num_threads()))
    if not torch.cuda.is_available():
        raise SystemExit("classifier_bench needs a HIP device (no CPU fallback)")
    from expertsim.train import classifier as K
    from expertsim.train import distances as D
    from expertsim.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    N, degree, max_iter = args.n, 2, 50
    sync = torch.cuda.synchronize
    batch = limited(args.step_limit, make_batch, N, "neutron", seed=11)
    real_img = torch.from_numpy(batch["real_images"]).to(dev)
    fake_img = torch.from_numpy(limited(args.step_limit, make_batch, N, "neutron", seed=12)["real_images"]).to(dev)
    obs_real, obs_gen = D.observables(real_img), D.observables(fake_img)
    rs = np.random.RandomState(20261021)
    res = {"n": N, "cols": int(obs_real.shape[1]), "degree": degree, "max_iter": max_iter, "gtol": 1e-9, "l2": 1.0,
           "device": torch.cuda.get_device_name(0), "warmup": 1, "reps": 5, "note": "one run on one box"}
    experts = {1: torch.zeros(N, dtype=torch.int32, device=dev),
               4: torch.from_numpy(rs.randint(0, 4, N).astype(np.int32)).to(dev)}
    joint_tables = None
    for E, expert in experts.items():
        raw = K.c2st_device(obs_real, obs_gen, expert, E, degree, max_iter=max_iter)
        xr, xf = raw["real"], raw["fake"]
        if joint_tables is None:
            joint_tables = (xr[:N], xf[:N])
        tr = dict(r_seg=raw["train_seg"], f_seg=raw["f_train_seg"], r_cap=(N + 1) // 2, f_cap=(N + 1) // 2)
        te = dict(r_seg=raw["test_seg"], f_seg=raw["f_test_seg"], r_cap=N // 2, f_cap=N // 2)
        stat = raw["stat"].cpu().numpy()
        iters = int(stat[:, 2].max())
        one = {"features": int(xr.shape[1]), "segments": int(stat.shape[0]), "iterations": stat[:, 2].tolist(),
               "status": stat[:, 3].tolist(), "passes": iters + 1, "launches": 1 + 2 * (max_iter + 1)}
        fit_out = (raw["theta"].clone(), raw["stat"].clone())
        one["logit_fit_events"] = limited(args.step_limit, by_events,
                                          lambda: K.logit_fit(xr, xf, max_iter=max_iter, out=fit_out, **tr), torch)
        one["logit_fit_events"]["ms_per_pass"] = one["logit_fit_events"]["median_s"] * 1e3 / (iters + 1)
        one["logit_fit_no_spare_launches_events"] = limited(
            args.step_limit, by_events, lambda: K.logit_fit(xr, xf, max_iter=max(iters, 1), out=fit_out, **tr), torch)
        one["logit_scores_events"] = limited(args.step_limit, by_events,
                                             lambda: K.logit_scores(xr, xf, raw["theta"], **te), torch)
        sr, sf = raw["r_scores"].reshape(-1, 1), raw["f_scores"].reshape(-1, 1)
        one["rank_stats_events"] = limited(
            args.step_limit, by_events,
            lambda: K.rank_stats(sr, sf, u_seg=raw["score_r_seg"], v_seg=raw["score_f_seg"], u_cap=N // 2,
                                 v_cap=N // 2, out=raw["rank"]), torch)
        one["c2st_end_to_end"] = limited(args.step_limit, timed,
                                         lambda: K.c2st(obs_real, obs_gen, expert, E, degree, max_iter=max_iter), sync)
        one["values"] = K.c2st(obs_real, obs_gen, expert, E, degree, max_iter=max_iter)
        res[f"E{E}"] = one

    if not args.no_model:
        from expertsim.config import load_config
        from expertsim.train.loop import setup_moe_system
        cond = torch.from_numpy(batch["cond"]).to(dev)
        for E in experts:
            cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                         f"model.n_experts={E}", "train.precision=fp32"])
            torch.manual_seed(4)
            moe = setup_moe_system(cfg, dev)
            moe.eval()
            off, on = limited(args.step_limit, alternating,
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1),
                              lambda: moe.evaluate_device(0, cond, real_img, cfg, seed=1, classifier=True), sync)
            res[f"E{E}"]["evaluate_device"] = {"without": off, "with_classifier": on, "alternating": True,
                                               "added_median_s": on["median_s"] - off["median_s"],
                                               "ranges_disjoint": on["min_s"] > off["max_s"]}

    if not args.no_baseline:
        host = limited(args.step_limit, host_c2st, np, *joint_tables)
        host.update(how="copy of both [N, 65] fp64 feature tables out, LogisticRegression(newton-cholesky) on the "
                        "training half, roc_auc_score and ks_2samp on the held-out scores; the joint segment only; "
                        "host, at most 16 threads, one run", runs=1)
        res["host_baseline"] = host
        res["ranges_disjoint"] = {f"E{E}_c2st_vs_host": res[f"E{E}"]["c2st_end_to_end"]["max_s"] < host["seconds"]
                                  for E in experts}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
