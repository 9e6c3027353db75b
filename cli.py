"""CLI — reference: cli.py:37-118 (same flags: --config, --override/-o key=value ...).

    python cli.py --config generative-dnn-for-physics-simulations-cern_amd/expertsim/config/default.yaml \
        -o model.architecture=neutron dataset.input_image_shape=[44,44] model.n_experts=1 train.batch_size=64
Multi-GPU: python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 cli.py ...
The reference's CUDA_LAUNCH_BLOCKING / cudnn flags / anomaly detection (cli.py:27-34) are dropped.

Simulation (conditions in, calorimeter images out; MoEWrapper.simulate) from a saved checkpoint:
    python cli.py -o model.architecture=neutron dataset.input_image_shape=[44,44] model.n_experts=3 \
        --simulate --checkpoint DIR [--checkpoint-epoch E] (--cond FILE.npy | --num-samples N) --out FILE.npz \
        [--features] [--real FILE.npy [--prdc-k K] [--distances] [--sliced [--sliced-proj P]]
                                      [--classifier [--classifier-degree D]]
                                      [--conditional [--conditional-bins B] [--conditional-column J]]]
--real FILE.npy (real images [N,H,W] in the log1p domain, aligned with --cond) adds the sample-level precision /
recall / density / coverage of the simulated images against them at K neighbours (default 5), jointly and per
expert (expertsim/train/fidelity.py), as prdc_* entries of the .npz and on stdout.  --distances adds the Frechet
and kernel distances of the ten shower observables (expertsim/train/distances.py) next to them as dist_* entries.
--sliced adds the sliced Wasserstein distance of whole images in the log1p domain at P random directions (default
256; expertsim/train/sliced.py) as swd* entries.  --classifier adds the classifier two-sample test of the ten shower
observables (held-out AUC, KS, accuracy and log-loss of a logistic regression on the observables and, at D = 2,
their pairwise products; expertsim/train/classifier.py) as c2st_* entries.  --conditional adds the conditional
profile of the ten shower observables in B equally populated bins (default 8) of column J (default 0, the energy) of
the conditions: the count-weighted per-bin Wasserstein distance, median bias, width difference and KS statistic as
cond_* scalars and the response / resolution curves as cond_* arrays (expertsim/train/conditional.py).

Dataset preparation (raw responses + particle conditions in, the three pickles of dataset.source=pickle out;
expertsim/utils/data_preparation.py) for the detector named by dataset.zdc_type:
    python cli.py -o dataset.zdc_type=neutron --prepare --images FILE.npy|.pkl --conditions FILE.pkl|.npy \
        [--cond-columns NAME ...] [--raw] [--min-photon-sum X] [--max-photon-sum X] --out-dir DIR \
        [--clusters K [--cluster-seed S] [--cluster-restarts R]]
--clusters K (proton sets) writes the expert_number column from a k-means of the images into K clusters
(expertsim/utils/clustering.py).

Expert diagnostics (MoEWrapper.diagnose: per-expert histograms and kernel density estimates of the photon
sums and the conditioning variables, as arrays) from a saved checkpoint:
    python cli.py -o model.n_experts=3 --diagnose --checkpoint DIR [--checkpoint-epoch E] \
        --conditions FILE.npy|.pkl --out FILE.npz [--embedding [--embedding-iters K]] [--expert-number FILE.npy]
--embedding adds the PCA and exact t-SNE embedding of the conditions by expert (expertsim/train/embedding.py).
--expert-number adds the router's agreement with that class vector (confusion matrix, accuracy, macro
precision / recall / F1, matched accuracy, adjusted Rand index) as router_agreement.* arrays.
"""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd"))

logging.basicConfig(level=logging.INFO, format="%(asctime)s [%(levelname)s] %(message)s",
                    handlers=[logging.StreamHandler(sys.stdout)])
logger = logging.getLogger(__name__)


def parse_args(args=None):
    p = argparse.ArgumentParser(description="Run Mixture-of-Experts GAN experiments (MI355X build).")
    p.add_argument("--config", type=str, default=None, help="YAML config (default: expertsim/config/default.yaml)")
    p.add_argument("--override", "-o", nargs="*", default=[], help="key=value overrides")
    p.add_argument("--max-steps-per-epoch", type=int, default=None)
    g = p.add_argument_group("simulation (instead of training)")
    g.add_argument("--simulate", action="store_true", help="simulate images for conditions from a checkpoint")
    g.add_argument("--checkpoint", type=str, default=None, help="directory holding the checkpoint's .pth files")
    g.add_argument("--checkpoint-epoch", type=int, default=None, help="epoch to load (default: the latest saved)")
    g.add_argument("--cond", type=str, default=None, help=".npy file of conditions [N, cond_dim]")
    g.add_argument("--num-samples", type=int, default=None, help="synthetic conditions instead of --cond")
    g.add_argument("--out", type=str, default=None, help="output .npz (images, expert, sums, cond)")
    g.add_argument("--seed", type=int, default=0, help="seed of the simulation's noise and routing draws")
    g.add_argument("--sim-batch-size", type=int, default=None, help="conditions per chunk")
    g.add_argument("--features", action="store_true",
                   help="also write the shower-shape observables: features [N,5], peak [N,2]")
    g.add_argument("--real", type=str, default=None,
                   help=".npy real images [N,H,W] (log1p domain, aligned with --cond): also precision / recall / "
                        "density / coverage of the simulated images against them")
    g.add_argument("--prdc-k", type=int, default=5, help="neighbours of the --real metrics")
    g.add_argument("--distances", action="store_true",
                   help="with --real: also the Frechet and kernel distances of the ten shower observables (dist_*)")
    g.add_argument("--sliced", action="store_true",
                   help="with --real: also the sliced Wasserstein distance of whole images (swd, swd_err, swd_max)")
    g.add_argument("--sliced-proj", type=int, default=256, help="random directions of --sliced")
    g.add_argument("--classifier", action="store_true",
                   help="with --real: also the classifier two-sample test of the ten shower observables (c2st_*)")
    g.add_argument("--classifier-degree", type=int, default=2, choices=(1, 2),
                   help="features of --classifier: 1 the observables, 2 also their pairwise products")
    g.add_argument("--conditional", action="store_true",
                   help="with --real: also the conditional profile of the ten shower observables by condition bin "
                        "(cond_*)")
    g.add_argument("--conditional-bins", type=int, default=8, help="equally populated bins of --conditional")
    g.add_argument("--conditional-column", type=int, default=0,
                   help="column of the conditions that --conditional bins (0: the energy)")
    x = p.add_argument_group("expert diagnostics (instead of training)")
    x.add_argument("--diagnose", action="store_true",
                   help="per-expert histograms and KDEs for --conditions FILE from --checkpoint DIR, written to --out")
    x.add_argument("--embedding", action="store_true",
                   help="with --diagnose: also the PCA / exact t-SNE embedding of the conditions by expert")
    x.add_argument("--embedding-iters", type=int, default=1000, help="t-SNE iterations of --embedding")
    x.add_argument("--expert-number", type=str, default=None,
                   help="with --diagnose: .npy class vector [N] (expert_number) to compare the routing against")
    d = p.add_argument_group("dataset preparation (instead of training)")
    d.add_argument("--prepare", action="store_true",
                   help="compute std, group_number, photon sums and peak positions; write the pickle data source")
    d.add_argument("--images", type=str, default=None, help=".npy file or pickle of the images [N,H,W]")
    d.add_argument("--conditions", type=str, default=None,
                   help="pickle of the conditions frame, or .npy [N,C] matrix named by --cond-columns")
    d.add_argument("--cond-columns", nargs="*", default=None,
                   help="column names of a .npy conditions matrix (default: the 9 conditioning columns)")
    d.add_argument("--raw", action="store_true", help="the images are photon counts: np.log1p is applied first")
    d.add_argument("--min-photon-sum", type=float, default=None, help="keep samples with photon sum >= this")
    d.add_argument("--max-photon-sum", type=float, default=None, help="keep samples with photon sum <= this")
    d.add_argument("--out-dir", type=str, default=None, help="directory for the three pickles")
    d.add_argument("--clusters", type=int, default=None,
                   help="proton sets: write expert_number from a k-means of the images into this many clusters")
    d.add_argument("--cluster-seed", type=int, default=0, help="seed of the k-means++ draws of --clusters")
    d.add_argument("--cluster-restarts", type=int, default=10, help="k-means restarts of --clusters")
    return p.parse_args(args)


def _load_checkpointed_moe(args, flag):
    """(cfg, moe in eval mode, epoch) for --simulate / --diagnose: the model of the config with the
    checkpoint's weights."""
    import glob
    import re
    import torch
    from expertsim.config import DEFAULT_PATH, load_config
    from expertsim.train.loop import setup_moe_system
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import load_checkpoint
    cfg = load_config(args.config or DEFAULT_PATH, args.override)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    moe = setup_moe_system(cfg, device)
    ckpt = args.checkpoint
    if not glob.glob(os.path.join(ckpt, "*.pth")) and os.path.isdir(os.path.join(ckpt, "models")):
        ckpt = os.path.join(ckpt, "models")
    epoch = args.checkpoint_epoch
    if epoch is None:
        found = [int(m.group(1)) for f in glob.glob(os.path.join(ckpt, "router_network_epoch_*.pth"))
                 for m in [re.search(r"_epoch_(\d+)\.pth$", f)] if m]
        if not found:
            raise SystemExit(f"{flag}: no checkpoint files in {ckpt}")
        epoch = max(found)
    load_checkpoint(ckpt, epoch, moe, *setup_optimizers(moe, cfg), None, device)
    moe.eval()
    return cfg, moe, epoch


def simulate(args):
    """--simulate: load the checkpoint, run MoEWrapper.simulate(sums=True), write the .npz."""
    import numpy as np
    import torch
    if not args.checkpoint or not args.out or (args.cond is None) == (args.num_samples is None):
        raise SystemExit("--simulate needs --checkpoint DIR, --out FILE.npz and one of --cond FILE.npy / --num-samples N")
    if args.conditional and args.real is None:
        raise SystemExit("--conditional needs --real FILE.npy")
    if not torch.cuda.is_available():
        raise RuntimeError("expertsim simulates on a HIP device only (no CPU fallback)")
    cfg, moe, epoch = _load_checkpointed_moe(args, "--simulate")
    if args.cond is not None:
        cond = np.load(args.cond).astype(np.float32)
    else:
        from expertsim.utils.synthetic import make_batch
        cond = make_batch(args.num_samples, str(cfg.model.architecture), seed=args.seed)["cond"]
    moe.eval()
    res = moe.simulate(torch.from_numpy(cond), seed=args.seed, batch_size=args.sim_batch_size, sums=True,
                       features=args.features)
    extra = {k: res[k].cpu().numpy() for k in ("features", "peak")} if args.features else {}
    if args.real is not None:
        from expertsim.train.fidelity import prdc
        real = np.load(args.real).astype(np.float32)
        if real.shape[0] != cond.shape[0]:
            raise SystemExit(f"--real has {real.shape[0]} images for {cond.shape[0]} conditions")
        device = res["images"].device
        m = prdc(torch.from_numpy(real).to(device), torch.log1p(res["images"]), k=args.prdc_k,
                 expert=res["expert"], n_experts=moe.n_experts, details=True)
        for name, v in m.items():
            if isinstance(v, float):
                extra[f"prdc_{name}"] = np.float64(v)
                logger.info("prdc_%s = %.6f", name, v)
        extra["prdc_totals"] = m["totals"].cpu().numpy()
        extra["prdc_k"] = np.int64(args.prdc_k)
        if args.distances:
            from expertsim.train import distances as dist
            feat = res["features"] if args.features else None
            obs_real = dist.observables(torch.from_numpy(real).to(device), log_domain=True)
            obs_gen = dist.observables(res["images"], log_domain=False, sums=res["sums"], features=feat)
            obs_real, obs_gen, _ = dist.normalise(obs_real, obs_gen)
            for name, v in dist.distances(obs_real, obs_gen, res["expert"], moe.n_experts).items():
                extra[f"dist_{name}"] = np.float64(v)
                logger.info("dist_%s = %.6g", name, v)
        if args.sliced:
            from expertsim.train.sliced import sliced
            for name, v in sliced(torch.from_numpy(real).to(device), torch.log1p(res["images"]), res["expert"],
                                  moe.n_experts, n_proj=args.sliced_proj, seed=args.seed).items():
                extra[name] = np.float64(v)
                logger.info("%s = %.6g", name, v)
            extra["swd_proj"] = np.int64(args.sliced_proj)
        if args.classifier:
            from expertsim.train import distances as dist
            from expertsim.train.classifier import c2st
            feat = res["features"] if args.features else None
            obs_real = dist.observables(torch.from_numpy(real).to(device), log_domain=True)
            obs_gen = dist.observables(res["images"], log_domain=False, sums=res["sums"], features=feat)
            for name, v in c2st(obs_real, obs_gen, res["expert"], moe.n_experts,
                                degree=args.classifier_degree).items():
                extra[name] = np.float64(v)
                logger.info("%s = %.6g", name, v)
            extra["c2st_degree"] = np.int64(args.classifier_degree)
        if args.conditional:
            from expertsim.train import distances as dist
            from expertsim.train.conditional import profile
            if not 0 <= args.conditional_column < cond.shape[1]:
                raise SystemExit(f"--conditional-column {args.conditional_column} outside the {cond.shape[1]} columns")
            feat = res["features"] if args.features else None
            obs_real = dist.observables(torch.from_numpy(real).to(device), log_domain=True)
            obs_gen = dist.observables(res["images"], log_domain=False, sums=res["sums"], features=feat)
            by = torch.from_numpy(np.ascontiguousarray(cond[:, args.conditional_column])).to(device)
            for name, v in profile(obs_real, obs_gen, by, args.conditional_bins, res["expert"], moe.n_experts,
                                   names=dist.OBSERVABLE_NAMES, details=True).items():
                if isinstance(v, float):
                    extra[name] = np.float64(v)
                    logger.info("%s = %.6g", name, v)
                elif name in ("ws", "ks"):
                    extra[f"cond_{name}_bins"] = v.cpu().numpy()
                elif name not in ("seg", "idx", "q_all"):
                    extra[f"cond_{name}"] = v.cpu().numpy()
            extra["cond_column"] = np.int64(args.conditional_column)
    elif args.classifier:
        raise SystemExit("--classifier needs --real FILE.npy")
    elif args.distances:
        raise SystemExit("--distances needs --real FILE.npy")
    elif args.sliced:
        raise SystemExit("--sliced needs --real FILE.npy")
    np.savez(args.out, images=res["images"].cpu().numpy(), expert=res["expert"].cpu().numpy(),
             sums=res["sums"].cpu().numpy(), cond=cond, **extra)
    logger.info("Simulated %d images (epoch %d checkpoint) -> %s", cond.shape[0], epoch, args.out)


def diagnose(args):
    """--diagnose: load the checkpoint, run MoEWrapper.diagnose over the conditions, write the .npz."""
    import numpy as np
    import torch
    from expertsim.train.diagnostics import save_diagnostics
    if not args.checkpoint or not args.conditions or not args.out:
        raise SystemExit("--diagnose needs --checkpoint DIR, --conditions FILE and --out FILE.npz")
    if not torch.cuda.is_available():
        raise RuntimeError("expertsim computes the diagnostics on a HIP device only (no CPU fallback)")
    cfg, moe, epoch = _load_checkpointed_moe(args, "--diagnose")
    cond = _load_array_or_pickle(args.conditions)
    names = args.cond_columns
    if hasattr(cond, "columns"):
        from expertsim.utils.data_transformations import COND_COLUMNS
        names = names or [c for c in COND_COLUMNS if c in cond.columns]
        cond = cond[names].to_numpy()
    cond = np.asarray(cond, dtype=np.float32)
    expert_number = np.load(args.expert_number) if args.expert_number else None
    diag = moe.diagnose(torch.from_numpy(cond), seed=args.seed, names=names, embedding=args.embedding,
                        embedding_iters=args.embedding_iters, expert_number=expert_number)
    path = save_diagnostics(args.out, diag)
    logger.info("Diagnostics of %d conditions over %d experts (epoch %d checkpoint) -> %s", cond.shape[0],
                moe.n_experts, epoch, path)
    return path


def _load_array_or_pickle(path):
    import numpy as np
    import pandas as pd
    return np.load(path) if path.endswith(".npy") else pd.read_pickle(path)


def prepare(args):
    """--prepare: images + conditions -> the three pickles of the pickle data source."""
    import numpy as np
    import pandas as pd
    import torch
    from expertsim.config import DEFAULT_PATH, load_config
    from expertsim.utils import data_preparation as DP
    if not args.images or not args.conditions or not args.out_dir:
        raise SystemExit("--prepare needs --images FILE, --conditions FILE and --out-dir DIR")
    if not torch.cuda.is_available():
        raise RuntimeError("expertsim prepares datasets on a HIP device only (no CPU fallback)")
    cfg = load_config(args.config or DEFAULT_PATH, args.override)
    zdc = str(cfg.dataset.zdc_type)
    torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
    images = np.asarray(_load_array_or_pickle(args.images))
    if args.raw:
        images = np.log1p(images.astype(np.float64))
    cond = _load_array_or_pickle(args.conditions)
    if not isinstance(cond, pd.DataFrame):
        cond = pd.DataFrame(np.asarray(cond), columns=args.cond_columns or DP.COND_COLUMNS)
    images, cond_out, positions = DP.prepare_dataset(images, cond, zdc, args.min_photon_sum, args.max_photon_sum,
                                                     n_clusters=args.clusters, cluster_seed=args.cluster_seed,
                                                     cluster_restarts=args.cluster_restarts)
    paths = DP.write_dataset(args.out_dir, zdc, images, cond_out, positions, cfg=cfg)
    group_col = "group_number_proton" if zdc == "proton" else "group_number"
    sizes = np.bincount(cond_out[group_col].to_numpy()) if len(cond_out) else np.zeros(0, dtype=np.int64)
    q = np.percentile(sizes, [25, 50, 75]).tolist() if len(sizes) else [0.0, 0.0, 0.0]
    logger.info("Prepared %d %s samples in %d groups; group-size quartiles %s (min %d, max %d)", len(cond_out), zdc,
                len(sizes), q, int(sizes.min()) if len(sizes) else 0, int(sizes.max()) if len(sizes) else 0)
    logger.info("Wrote %s", " ".join(f"dataset.{k}={v}" for k, v in paths.items()))
    return paths


def main():
    args = parse_args(sys.argv[1:])
    if args.simulate:
        return simulate(args)
    if args.prepare:
        return prepare(args)
    if args.diagnose:
        return diagnose(args)
    from expertsim.config import DEFAULT_PATH, load_config
    from expertsim.train.loop import train
    from expertsim.utils.data_transformations import get_train_test_data_loaders
    cfg = load_config(args.config or DEFAULT_PATH, args.override)
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    train_loader, test_loader = get_train_test_data_loaders(cfg, rank, world)
    train(cfg, train_loader, test_loader, max_steps_per_epoch=args.max_steps_per_epoch)
    logger.info("Training completed successfully.")


if __name__ == "__main__":
    main()
