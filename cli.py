"""CLI — reference: cli.py:37-118 (same flags: --config, --override/-o key=value ...).

    python cli.py --config generative-dnn-for-physics-simulations-cern_amd/expertsim/config/default.yaml \
        -o model.architecture=neutron dataset.input_image_shape=[44,44] model.n_experts=1 train.batch_size=64
Multi-GPU: python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 cli.py ...
The reference's CUDA_LAUNCH_BLOCKING / cudnn flags / anomaly detection (cli.py:27-34) are dropped.

Simulation (conditions in, calorimeter images out; MoEWrapper.simulate) from a saved checkpoint:
    python cli.py -o model.architecture=neutron dataset.input_image_shape=[44,44] model.n_experts=3 \
        --simulate --checkpoint DIR [--checkpoint-epoch E] (--cond FILE.npy | --num-samples N) --out FILE.npz \
        [--features]
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
    return p.parse_args(args)


def simulate(args):
    """--simulate: load the checkpoint, run MoEWrapper.simulate(sums=True), write the .npz."""
    import glob
    import re
    import numpy as np
    import torch
    from expertsim.config import DEFAULT_PATH, load_config
    from expertsim.train.loop import setup_moe_system
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import load_checkpoint
    if not args.checkpoint or not args.out or (args.cond is None) == (args.num_samples is None):
        raise SystemExit("--simulate needs --checkpoint DIR, --out FILE.npz and one of --cond FILE.npy / --num-samples N")
    if not torch.cuda.is_available():
        raise RuntimeError("expertsim simulates on a HIP device only (no CPU fallback)")
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
            raise SystemExit(f"--simulate: no checkpoint files in {ckpt}")
        epoch = max(found)
    load_checkpoint(ckpt, epoch, moe, *setup_optimizers(moe, cfg), None, device)
    if args.cond is not None:
        cond = np.load(args.cond).astype(np.float32)
    else:
        from expertsim.utils.synthetic import make_batch
        cond = make_batch(args.num_samples, str(cfg.model.architecture), seed=args.seed)["cond"]
    moe.eval()
    res = moe.simulate(torch.from_numpy(cond), seed=args.seed, batch_size=args.sim_batch_size, sums=True,
                       features=args.features)
    extra = {k: res[k].cpu().numpy() for k in ("features", "peak")} if args.features else {}
    np.savez(args.out, images=res["images"].cpu().numpy(), expert=res["expert"].cpu().numpy(),
             sums=res["sums"].cpu().numpy(), cond=cond, **extra)
    logger.info("Simulated %d images (epoch %d checkpoint) -> %s", cond.shape[0], epoch, args.out)


def main():
    args = parse_args(sys.argv[1:])
    if args.simulate:
        return simulate(args)
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
