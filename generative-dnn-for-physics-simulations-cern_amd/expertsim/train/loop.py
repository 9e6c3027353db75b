"""Training orchestration — reference: expertsim/train/loop.py:27-182,332-354.

Same entry points (``train``, ``train_epoch``, ``train_step``, ``setup_moe_system``); the per-batch
step is ``MoEWrapper.train_step`` on the HIP path.  Metrics are fetched to the host once per batch
(the reference does ``.cpu().item()`` per key, loop.py:136-148).  With WORLD_SIZE > 1 (torchrun),
every rank trains on its own shard and gradients are all-reduced over RCCL (expertsim/train/ddp.py).
``evaluate_epoch`` (loop.py:185-256) produces the Wasserstein metrics of MoEWrapper.evaluate on the
HIP path, or with ``train.eval_on_device`` those of
MoEWrapper.evaluate_device (everything up to the distances on the device).  Checkpoints (hooks.CheckpointSaver, training_utils) and the
EMAHelper (ema.py) follow loop.py:36-107,357-418; resume restores weights, optimizer moments and
the step counters.  W&B and the drawing of figures stay out of scope; the numbers behind the reference's
expert-specialisation plots are ``train.eval_diagnostics`` (MoEWrapper.diagnose, train/diagnostics.py).
"""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, List

import numpy as np
import torch

from ..models import build_model
from ..models.moe import MoEWrapper
from .ema import EMAHelper
from .hooks import CheckpointSaver
from .training_setup import setup_optimizers
from .training_utils import load_checkpoint

logger = logging.getLogger(__name__)


def setup_moe_system(cfg, device) -> MoEWrapper:
    from ..config import inject_shared
    inject_shared(cfg)
    generator = build_model(f"{cfg.model.architecture}.generator", cfg.model.generator, device)
    discriminator = build_model(f"{cfg.model.architecture}.discriminator", cfg.model.discriminator, device)
    aux_reg = build_model(f"{cfg.model.architecture}.aux_reg", cfg.model.aux_reg, device)
    router = build_model(f"{cfg.model.router.version}", cfg.model.router, device)
    return MoEWrapper(generator, discriminator, aux_reg, router, cfg.model.n_experts, cfg,
                      image_shape=tuple(cfg.dataset.input_image_shape)).to(device)


def train_step(batch, moe, gen_optims, disc_optims, aux_reg_optim, router_optim, cfg, device, epoch,
               ema_helper) -> Dict:
    real_images, _, cond, std, intensity, true_positions = batch
    real_images = real_images.unsqueeze(1).to(device, non_blocking=True)
    return moe.train_step(epoch, cond.to(device, non_blocking=True), real_images,
                          true_positions.to(device, non_blocking=True), std.to(device, non_blocking=True),
                          intensity.to(device, non_blocking=True), aux_reg_optim, gen_optims, disc_optims,
                          router_optim, ema_helper, device)


def setup_callbacks(cfg, moe, ema_helper=None) -> List:
    """loop.py:357-375 (the W&B logger is out of scope)."""
    callbacks = []
    cfg.generator_name = getattr(moe.generators[0], "name", "generator")
    cfg.discriminator_name = getattr(moe.discriminators[0], "name", "discriminator")
    cfg.router_name = getattr(moe.router, "name", "router")
    if cfg.train.get("save_experiment_data", False):
        callbacks.append(CheckpointSaver(dir_path=_dir_models(cfg), monitor="ws_mean",
                                         ws_threshold=cfg.train.ws_threshold_model_save, ema_helper=ema_helper))
    return callbacks


def _dir_models(cfg):
    d = cfg.train.get("dir_models")
    if d is None:
        exp = cfg.get_path("config.experiment_dir") or os.path.join(cfg.train.get("save_experiments_dir") or "",
                                                                     cfg.config.get("run_name", "experiment"))
        d = cfg.train.dir_models = f"{exp}/models/"
    return d


def train_epoch(moe, train_loader, gen_optims, disc_optims, aux_reg_optims, router_optim, cfg, device, epoch,
                ema_helper, max_steps=None) -> Dict:
    moe.train()
    sums: Dict[str, List[float]] = {}
    for i, batch in enumerate(train_loader):
        if max_steps is not None and i >= max_steps:
            break
        m = train_step(batch, moe, gen_optims, disc_optims, aux_reg_optims, router_optim, cfg, device, epoch,
                       ema_helper)
        if ema_helper is not None and cfg.train.get("ema_update", False):
            ema_helper.update(moe, range(moe.n_experts))     # build extension: the reference never updates
        keys = list(m)
        vals = torch.stack([torch.as_tensor(m[k], dtype=torch.float32, device=device).reshape(())
                            for k in keys]).cpu().numpy()   # ONE device->host copy per batch
        for k, v in zip(keys, vals):
            sums.setdefault(k, []).append(float(v))
    out = {k: float(np.mean(v)) for k, v in sums.items()}
    for i in range(moe.n_experts):
        out[f"G_steps_{i}"] = moe.g_steps[i]
        out[f"D_steps_{i}"] = moe.d_steps[i]
    return out


@torch.no_grad()
def evaluate_epoch(moe, test_loader, epoch: int, cfg, device, max_batches=None) -> Dict:
    """Reference loop.py:185-256 without the plots: per-batch MoEWrapper.evaluate, averaged.
    train.eval_on_device: MoEWrapper.evaluate_device instead (routing, generation and the Wasserstein
    distances on the device, seeded by train.rng_seed; a sample's draws depend on its position in the
    test set, not on the loader's batch size).  train.eval_features (with eval_on_device only): also the
    shower-shape metrics of evaluate_device(features=True), averaged like the others.
    train.eval_diagnostics (with eval_on_device only): after the last batch, MoEWrapper.diagnose once over
    the conditions of the whole test set (the reference concatenates the test set for its specialisation
    plots, loop.py:234-329) with seed = train.rng_seed and sample_offset = 0, under
    metrics["expert_diagnostics"]; with train.save_experiment_data and train.dir_info also written to
    diagnostics_epoch_<epoch>.npz there.  Off: the returned dict and the launches are unchanged.
    train.eval_embedding (with eval_diagnostics only): diagnose(embedding=True, embedding_iters=
    train.eval_embedding_iters, embedding_max=train.eval_embedding_max) -- the PCA / t-SNE keys of
    train/embedding.py join the diagnostics and the .npz.
    train.eval_prdc (with eval_on_device only): also the sample-level precision / recall / density / coverage of
    evaluate_device(prdc=True, prdc_k=train.eval_prdc_k), each key averaged over the batches in which it is finite
    (an expert with at most k rows in a batch gives NaN there); NaN if it is finite in none.  These metrics
    depend on the batch size (the number of samples on each side) and on k, so runs are comparable only at equal
    batch size and equal train.eval_prdc_k.
    train.eval_distances (with eval_on_device only): also the joint-distribution distances of
    evaluate_device(distances=True) (train/distances.py: dist_fpd, dist_kpd and their companions, jointly and per
    expert), each key averaged over the batches in which it is finite; NaN if it is finite in none.  Both
    statistics depend on the number of samples in a batch: compare runs at equal batch size.
    train.eval_sliced (with eval_on_device only): also the sliced Wasserstein distance of whole images of
    evaluate_device(sliced=True, sliced_proj=train.eval_sliced_proj) (train/sliced.py: swd, swd_err, swd_max, jointly
    and per expert), each key averaged over the batches in which it is finite; NaN if it is finite in none.  The
    value depends on train.eval_sliced_proj: compare runs at equal settings.
    train.eval_classifier (with eval_on_device only): also the classifier two-sample test of
    evaluate_device(classifier=True, classifier_degree=train.eval_classifier_degree) (train/classifier.py: c2st_auc,
    c2st_ks, c2st_acc, c2st_logloss, c2st_iter, c2st_converged, jointly and per expert), each key averaged over the
    batches in which it is finite; NaN if it is finite in none.  The classifier trains on the first half of a batch's
    rows and is scored on the second, so the values depend on the batch size: compare runs at equal batch size.
    train.eval_conditional (with eval_on_device only): also the conditional profile of
    evaluate_device(conditional=True, conditional_bins=train.eval_conditional_bins,
    conditional_column=train.eval_conditional_column) (train/conditional.py: cond_ws and per observable cond_ws_<o>,
    cond_bias_<o>, cond_width_<o>, cond_ks_<o>, jointly and cond_ws_<e>, cond_ws_<o>_<e> per expert), each key averaged
    over the batches in which it is finite; NaN if it is finite in none.  The bins are each batch's own quantiles of
    the column: compare runs at equal batch size and equal train.eval_conditional_bins."""
    on_device = bool(cfg.train.get("eval_on_device", False))
    features = bool(cfg.train.get("eval_features", False))
    diagnostics = bool(cfg.train.get("eval_diagnostics", False))
    embedding = bool(cfg.train.get("eval_embedding", False))
    prdc = bool(cfg.train.get("eval_prdc", False))
    prdc_k = int(cfg.train.get("eval_prdc_k", 5))
    distances = bool(cfg.train.get("eval_distances", False))
    sliced = bool(cfg.train.get("eval_sliced", False))
    sliced_proj = int(cfg.train.get("eval_sliced_proj", 256))
    classifier = bool(cfg.train.get("eval_classifier", False))
    classifier_degree = int(cfg.train.get("eval_classifier_degree", 2))
    conditional = bool(cfg.train.get("eval_conditional", False))
    conditional_bins = int(cfg.train.get("eval_conditional_bins", 8))
    conditional_column = int(cfg.train.get("eval_conditional_column", 0))
    if conditional and not on_device:
        raise ValueError("train.eval_conditional needs train.eval_on_device: the conditional profiles exist on the "
                         "device path only (MoEWrapper.evaluate_device)")
    if classifier and not on_device:
        raise ValueError("train.eval_classifier needs train.eval_on_device: the classifier two-sample test exists on "
                         "the device path only (MoEWrapper.evaluate_device)")
    if sliced and not on_device:
        raise ValueError("train.eval_sliced needs train.eval_on_device: the sliced Wasserstein distance exists on the "
                         "device path only (MoEWrapper.evaluate_device)")
    if distances and not on_device:
        raise ValueError("train.eval_distances needs train.eval_on_device: the distribution distances exist on the "
                         "device path only (MoEWrapper.evaluate_device)")
    if prdc and not on_device:
        raise ValueError("train.eval_prdc needs train.eval_on_device: the sample-level metrics exist on the device "
                         "path only (MoEWrapper.evaluate_device)")
    if embedding and not diagnostics:
        raise ValueError("train.eval_embedding needs train.eval_diagnostics: the embedding is part of the expert "
                         "diagnostics (MoEWrapper.diagnose(embedding=True))")
    if diagnostics and not on_device:
        raise ValueError("train.eval_diagnostics needs train.eval_on_device: the expert diagnostics exist on the "
                         "device path only (MoEWrapper.diagnose)")
    if features and not on_device:
        raise ValueError("train.eval_features needs train.eval_on_device: the shower-shape metrics exist on the "
                         "device path only (MoEWrapper.evaluate_device)")
    moe.eval()
    keys = ["ws_mean", *[f"ws_mean_{i}" for i in range(moe.n_experts)],
            "ws_std", *[f"ws_std_{i}" for i in range(moe.n_experts)]]
    if features:
        from .utils import FEATURE_NAMES
        for name in FEATURE_NAMES:
            keys += [f"ws_feat_{name}", f"ws_feat_std_{name}", *[f"ws_feat_{name}_{i}" for i in range(moe.n_experts)]]
    prdc_keys = []
    if prdc:
        from .fidelity import METRICS
        prdc_keys = [f"prdc_{name}" for name in METRICS]
        prdc_keys += [f"prdc_{name}_{i}" for i in range(moe.n_experts) for name in METRICS]
    if distances:
        from .distances import KEYS
        prdc_keys += [f"dist_{name}" for name in KEYS]
        prdc_keys += [f"dist_{name}_{i}" for i in range(moe.n_experts) for name in KEYS]
    if sliced:
        from .sliced import KEYS as SWD_KEYS
        prdc_keys += list(SWD_KEYS)
        prdc_keys += [f"{name}_{i}" for i in range(moe.n_experts) for name in SWD_KEYS]
    if classifier:
        from .classifier import KEYS as C2ST_KEYS
        prdc_keys += list(C2ST_KEYS)
        prdc_keys += [f"{name}_{i}" for i in range(moe.n_experts) for name in C2ST_KEYS]
    if conditional:
        from .conditional import scalar_keys
        from .distances import OBSERVABLE_NAMES
        prdc_keys += scalar_keys(OBSERVABLE_NAMES, moe.n_experts)
    acc: Dict[str, List[float]] = {k: [] for k in keys + prdc_keys}
    seen = 0                                   # test samples in earlier batches
    conds = []                                 # the batches' device conditions (eval_diagnostics)
    for b, batch in enumerate(test_loader):
        if max_batches is not None and b >= max_batches:
            break
        real_images, _, cond, std, intensity, true_positions = batch
        if on_device:
            cond_dev = cond.to(device)
            extra = dict(prdc=True, prdc_k=prdc_k) if prdc else {}
            if distances:
                extra["distances"] = True
            if sliced:
                extra.update(sliced=True, sliced_proj=sliced_proj)
            if classifier:
                extra.update(classifier=True, classifier_degree=classifier_degree)
            if conditional:
                extra.update(conditional=True, conditional_bins=conditional_bins,
                             conditional_column=conditional_column)
            m = moe.evaluate_device(epoch, cond_dev, real_images, cfg,
                                    seed=int(cfg.train.get("rng_seed", 1234)), sample_offset=seen,
                                    features=features, **extra)
            if diagnostics:
                conds.append(cond_dev)
            seen += int(cond.shape[0])
        else:
            m = moe.evaluate(epoch, cond.to(device), real_images, true_positions, std, intensity, cfg, device)
        for k in keys:
            acc[k].append(float(m[k]))
        for k in prdc_keys:
            if np.isfinite(m[k]):
                acc[k].append(float(m[k]))
    out = {k: (sum(acc[k]) / len(acc[k]) if acc[k] else 0.0) for k in keys}
    out.update({k: (sum(acc[k]) / len(acc[k]) if acc[k] else float("nan")) for k in prdc_keys})
    if diagnostics and conds:
        from .diagnostics import save_diagnostics
        extra = dict(embedding=True, embedding_iters=int(cfg.train.get("eval_embedding_iters", 1000)),
                     embedding_max=int(cfg.train.get("eval_embedding_max", 16384))) if embedding else {}
        diag = moe.diagnose(torch.cat(conds), seed=int(cfg.train.get("rng_seed", 1234)), sample_offset=0, **extra)
        out["expert_diagnostics"] = diag
        dir_info = cfg.train.get("dir_info")
        if dir_info and cfg.train.get("save_experiment_data", False):
            os.makedirs(str(dir_info), exist_ok=True)
            save_diagnostics(os.path.join(str(dir_info), f"diagnostics_epoch_{epoch}.npz"), diag)
    return out


def train(cfg, train_loader, test_loader=None, max_steps_per_epoch=None) -> List[Dict]:
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise RuntimeError("expertsim trains on a HIP device only (no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    torch.manual_seed(int(cfg.train.get("rng_seed", 1234)))
    moe = setup_moe_system(cfg, device)
    if world > 1:
        import torch.distributed as dist
        from .ddp import DataParallel
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("nccl", device_id=device)
        moe.ddp = DataParallel(sync_bn=bool(cfg.train.get("sync_bn", False)))
        moe.rank = dist.get_rank()
    gen_optims, disc_optims, aux_optims, router_optim = setup_optimizers(moe, cfg)
    ema_helper = EMAHelper(moe, decay=0.99)                 # loop.py:44
    history = []
    start = 0
    ckpt_dir, ckpt_epoch = cfg.train.get("checkpoint_experiment_dir"), cfg.train.get("epoch_to_load")
    if (ckpt_dir is None) != (ckpt_epoch is None):
        raise ValueError("You should set both checkpoint_experiment_dir and epoch_to_load parameters!")
    if ckpt_dir is not None:
        load_checkpoint(os.path.join(ckpt_dir, "models"), int(ckpt_epoch), moe, gen_optims, disc_optims, aux_optims,
                        router_optim, ema_helper, device)
        start = int(ckpt_epoch) + 1
    callbacks = setup_callbacks(cfg, moe, ema_helper if cfg.train.get("ema_update", False) else None)
    for epoch in range(start, int(cfg.train.epochs)):
        t0 = time.time()
        metrics = train_epoch(moe, train_loader, gen_optims, disc_optims, aux_optims, router_optim, cfg, device,
                              epoch, ema_helper, max_steps=max_steps_per_epoch)
        if test_loader is not None:
            metrics.update(evaluate_epoch(moe, test_loader, epoch, cfg, device))
        for cb in callbacks:
            if moe.rank == 0:
                cb.on_epoch_end(epoch, metrics, moe, gen_optims, disc_optims, aux_optims, router_optim)
        metrics["epoch_time"] = time.time() - t0
        metrics["epoch"] = epoch
        history.append(metrics)
        logger.info("Epoch %d: %.2fs gen_loss %.4f disc_loss %.4f", epoch, metrics["epoch_time"],
                    metrics.get("gen_loss", float("nan")), metrics.get("disc_loss", float("nan")))
    return history
