"""Wall time of one evaluation call: MoEWrapper.evaluate (host routing, unfused generator passes, scipy
Wasserstein distances) against MoEWrapper.evaluate_device (simulate path + es_wasserstein_1d), one process.

Workload: neutron, fp32 and bf16, E = 1 and E = 4, one test batch of N = 4096 and one of N = 16384,
epoch 20 (n_calc = 5).  The images arrive as a host tensor and the conditions on the device, as
loop.evaluate_epoch passes them.  The two paths alternate call by call (so drift hits both alike):
warm-up calls first, then the timed ones; a call is timed by the wall clock between two device
synchronisations, because the host work is what is being compared.  Prints one JSON line: per case the
median [min, max] milliseconds of each path, the ratio of the medians and whether the two [min, max]
ranges are disjoint (the difference is outside the run-to-run spread).

    python tools/eval_bench.py [--n 4096 16384] [--experts 1 4] [--repeats 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd"))


def build(E, precision, dev):
    import torch
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", f"train.precision={precision}"])
    torch.manual_seed(1234)
    return setup_moe_system(cfg, dev).eval(), cfg


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(ms):
    return {"median": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--experts", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--precisions", nargs="+", default=["fp32", "bf16"])
    ap.add_argument("--epoch", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from expertsim.utils.synthetic import make_batch
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "epoch": args.epoch, "n_calc": min(args.epoch // 5 + 1, 5),
           "repeats": args.repeats, "warmup": args.warmup, "unit": "ms per call (wall clock, device synchronised)",
           "cases": {}}
    batches = {}
    for n in args.n:
        b = make_batch(n, "neutron", seed=1)
        batches[n] = {k: torch.from_numpy(b[k]) for k in ("real_images", "cond", "true_positions", "std", "intensity")}
    for precision in args.precisions:
        for E in args.experts:
            moe, cfg = build(E, precision, dev)
            for n in args.n:
                b = batches[n]
                cond, x = b["cond"].to(dev), b["real_images"]
                host = lambda: moe.evaluate(args.epoch, cond, x, b["true_positions"], b["std"], b["intensity"], cfg, dev)
                device = lambda: moe.evaluate_device(args.epoch, cond, x, cfg, seed=1234)
                ms = {"evaluate": [], "evaluate_device": []}
                last = {}
                for i in range(args.warmup + args.repeats):
                    for name, fn in (("evaluate", host), ("evaluate_device", device)):
                        t, out = wall_ms(fn)
                        last[name] = float(out["ws_mean"])
                        if i >= args.warmup:
                            ms[name].append(t)
                h, d = stats(ms["evaluate"]), stats(ms["evaluate_device"])
                res["cases"][f"{precision}.E{E}.N{n}"] = {
                    "evaluate": h, "evaluate_device": d, "speedup_of_medians": round(h["median"] / d["median"], 3),
                    "ranges_disjoint": bool(h["min"] > d["max"] or d["min"] > h["max"]),
                    "ws_mean": {k: round(v, 4) for k, v in last.items()}}
            del moe
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
