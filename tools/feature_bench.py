"""Cost of the shower-shape pass inside MoEWrapper.simulate (images/s), one process, HIP events.

Neutron, E = 1, N conditions in chunks of 1024, sums on, fp32 and bf16 (the settings of tools/sim_bench.py
leg a).  Two legs, timed ALTERNATING (off, on, off, on, ...) after a warm-up of both, so that drift of the
shared host falls on both alike:
  off  simulate(features=False)   the path as it was, the baseline
  on   simulate(features=True)    one es_image_features launch per chunk inside the chunk graph, plus the
                                  copies of the chunk's [n,5] / [n,2] results into the call's outputs
kernel: es_image_features alone over the N finished fp32 images, in N/chunk launches as simulate issues
them (ms per call, and the GB/s of the N*H*W*4 bytes it has to read), to say what the difference is made of.
Prints one JSON line: per leg the median images/s over the repeats and the min / max.

    python tools/feature_bench.py [--n 16384] [--chunk 1024] [--repeats 7] [--warmup 2] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def once(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from expertsim.train.utils import image_features
    from expertsim.utils.synthetic import make_batch
    from sim_bench import build
    dev = torch.device("cuda", 0)
    cond = torch.from_numpy(make_batch(args.n, "neutron", seed=1)["cond"]).to(dev)
    res = {"device": torch.cuda.get_device_name(0), "n": args.n, "chunk": args.chunk, "repeats": args.repeats,
           "warmup": args.warmup, "unit": "images/s", "order": "alternating off/on", "legs": {}}
    for precision in ("fp32", "bf16"):
        moe = build(1, precision, dev)
        legs = {"off": lambda: moe.simulate(cond, batch_size=args.chunk, sums=True),
                "on": lambda: moe.simulate(cond, batch_size=args.chunk, sums=True, features=True)}
        for _ in range(args.warmup):
            for fn in legs.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, fn in legs.items():
                ms[k].append(once(fn))
        for k, v in ms.items():
            ips = sorted(args.n / (m * 1e-3) for m in v)
            res["legs"][f"{precision}.{k}"] = {"median": round(statistics.median(ips)), "min": round(ips[0]),
                                               "max": round(ips[-1]), "ms_median": round(statistics.median(v), 3),
                                               "ms": [round(m, 3) for m in v]}
        images = moe.simulate(cond, batch_size=args.chunk, sums=True)["images"]

        def kernel_only():
            for s in range(0, args.n, args.chunk):
                image_features(images[s:s + args.chunk])
        for _ in range(args.warmup):
            kernel_only()
        torch.cuda.synchronize()
        kms = sorted(once(kernel_only) for _ in range(args.repeats))
        med = statistics.median(kms)
        res["legs"][f"{precision}.kernel"] = {
            "ms_median": round(med, 3), "ms_min": round(kms[0], 3), "ms_max": round(kms[-1], 3),
            "launches": -(-args.n // args.chunk),
            "read_GBps": round(images.numel() * 4 / (med * 1e-3) / 1e9, 1)}
        del moe
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
