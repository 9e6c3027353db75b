"""Conditioning embeddings on the device -- the numbers behind the reference's plot_cond_pca_tsne
(train/utils.py:422-467): the standardised conditions projected to two dimensions with PCA and with t-SNE, to be
coloured by expert.  Nothing is drawn: the results are arrays.

HIP kernels (csrc/embedding.hip, defined in include/expertsim_hip.h):

* ``es_pca_project``      mean, covariance (ddof = 1), the symmetric eigenproblem by cyclic Jacobi, sklearn's sign
  rule and the scores, all fp64 in a fixed summation order.
* ``es_tsne_affinities``  sklearn's binary search for each row's beta at the given perplexity, on fp32 pair
  distances that numpy reproduces bit for bit.
* ``es_tsne_gradient`` / ``es_tsne_run``  exact (all-pairs) t-SNE, matrix-free: the joint P is recomputed per pair
  and never stored; sklearn's gradient-descent update and schedule, no host round trip.

There is no CPU fallback: without a HIP device the functions raise hip.HipError.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ..segments import is_f64, ld, work_buffer
from .diagnostics import _values

EMBEDDING_KEYS = ("embed_rows", "embed_expert", "pca", "pca_components", "pca_explained_variance",
                  "pca_explained_variance_ratio", "tsne", "tsne_kl")


def pca_project(values, n_components=2):
    """sklearn.decomposition.PCA(n_components, svd_solver='full') of values [N, C] (fp32 / fp64): a dict of device
    fp64 tensors "scores" [N, k], "components" [k, C], "explained_variance" [k], "explained_variance_ratio" [k],
    "mean" [C].  No host synchronisation; runs on the current stream."""
    x = _values(values)
    N, C, k = int(x.shape[0]), int(x.shape[1]), int(n_components)
    dev = x.device
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"scores": torch.zeros(N, max(k, 0), **f64), "components": torch.zeros(max(k, 0), C, **f64),
           "explained_variance": torch.zeros(max(k, 0), **f64),
           "explained_variance_ratio": torch.zeros(max(k, 0), **f64), "mean": torch.zeros(C, **f64)}
    with torch.cuda.device(dev):
        need = hip.pca_project_workspace(C)
        work = work_buffer(need, dev)
        hip.call("es_pca_project", hip.ptr(x), is_f64(x), ld(x), N, C, k,
                 hip.ptr(out["scores"]), hip.ptr(out["components"]), hip.ptr(out["explained_variance"]),
                 hip.ptr(out["explained_variance_ratio"]), hip.ptr(out["mean"]), hip.ptr(work), need,
                 hip.stream_ptr())
    return out


def _values32(values):
    x = _values(values)
    return x if x.dtype == torch.float32 else x.float().contiguous()


def tsne_affinities(values, perplexity=30.0):
    """es_tsne_affinities on values [N, C] (fp32; fp64 is rounded first): a dict of device tensors "beta" [N] fp64,
    "log_s" [N] fp64, "dmin" [N] fp32, "steps" [N] int32 -- the per-row scalars that define the joint P."""
    x = _values32(values)
    N, C = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    out = {"beta": torch.zeros(N, dtype=torch.float64, device=dev),
           "log_s": torch.zeros(N, dtype=torch.float64, device=dev),
           "dmin": torch.zeros(N, dtype=torch.float32, device=dev),
           "steps": torch.zeros(N, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        hip.call("es_tsne_affinities", hip.ptr(x), ld(x), N, C, float(perplexity), hip.ptr(out["beta"]),
                 hip.ptr(out["log_s"]), hip.ptr(out["dmin"]), hip.ptr(out["steps"]), hip.stream_ptr())
    return out


def _check_y(y, N, dev):
    if y.dtype != torch.float32 or tuple(y.shape) != (N, 2) or not y.is_contiguous() or y.device != dev:
        raise ValueError(f"y must be a contiguous device fp32 [{N}, 2] tensor")


def tsne_gradient(values, aff, y, exaggeration=1.0):
    """es_tsne_gradient: (g [N, 2] fp64, z_kl [2] fp64 = (Z, KL)) at the embedding y [N, 2] fp32, device tensors."""
    x = _values32(values)
    N, C = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    _check_y(y, N, dev)
    g = torch.zeros(N, 2, dtype=torch.float64, device=dev)
    z_kl = torch.zeros(2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        need = hip.tsne_workspace(N)
        work = work_buffer(need, dev)
        hip.call("es_tsne_gradient", hip.ptr(x), ld(x), N, C, hip.ptr(aff["beta"]), hip.ptr(aff["log_s"]),
                 hip.ptr(aff["dmin"]), hip.ptr(y), float(exaggeration), hip.ptr(g), hip.ptr(z_kl), hip.ptr(work), need,
                 hip.stream_ptr())
    return g, z_kl


def auto_learning_rate(rows, exaggeration=12.0):
    """sklearn's learning_rate='auto'."""
    return max(rows / exaggeration / 4.0, 50.0)


def tsne_run(values, aff, y, upd, gains, n_iter, iter0=0, log=None, exaggeration=12.0, exaggeration_iters=250,
             momentum0=0.5, momentum1=0.8, learning_rate="auto", min_gain=0.01, check_every=50):
    """es_tsne_run: the iterations iter0 .. iter0 + n_iter - 1 on y [N, 2] fp32 in place (upd, gains [N, 2] fp64
    are the optimiser's state).  Returns the log [rows, 2] fp64 of (KL, |g|), NaN where no row was written; pass
    the log of an earlier call to continue it.  No host synchronisation."""
    x = _values32(values)
    N, C = int(x.shape[0]), int(x.shape[1])
    dev = x.device
    _check_y(y, N, dev)
    n_iter, iter0, check_every = int(n_iter), int(iter0), int(check_every)
    lr = auto_learning_rate(N, float(exaggeration)) if learning_rate == "auto" else float(learning_rate)
    rows = max((iter0 + n_iter - 1) // max(check_every, 1) + 1, 1)
    if log is None:
        log = torch.full((rows, 2), float("nan"), dtype=torch.float64, device=dev)
    elif log.shape[0] < rows:
        log = torch.cat([log, torch.full((rows - log.shape[0], 2), float("nan"), dtype=torch.float64, device=dev)])
    with torch.cuda.device(dev):
        need = hip.tsne_workspace(N)
        work = work_buffer(need, dev)
        hip.call("es_tsne_run", hip.ptr(x), ld(x), N, C, hip.ptr(aff["beta"]), hip.ptr(aff["log_s"]),
                 hip.ptr(aff["dmin"]), hip.ptr(y), hip.ptr(upd), hip.ptr(gains), n_iter, iter0, float(exaggeration),
                 int(exaggeration_iters), float(momentum0), float(momentum1), lr, float(min_gain), check_every,
                 hip.ptr(log), int(log.shape[0]), hip.ptr(work), need, hip.stream_ptr())
    return log


def pca_init(values):
    """sklearn's init='pca' of TSNE: the first two PCA scores as fp32, divided by the standard deviation of the
    first column, times 1e-4.  A function of values alone."""
    return _scaled_scores(pca_project(values, 2)["scores"])


def _scaled_scores(scores):
    s = scores.to(torch.float32)
    return (s / s[:, 0].std(unbiased=False) * 1e-4).contiguous()


def tsne_embed(values, perplexity=30.0, n_iter=1000, init="pca", exaggeration=12.0, exaggeration_iters=250,
               learning_rate="auto", y0=None):
    """Exact t-SNE of values [N, C] to two dimensions with sklearn's schedule: a dict of device tensors "y" [N, 2]
    fp32, "kl_log" [ceil(n_iter / 50), 2] fp64 rows of (KL, |g|), "beta" [N] fp64 and "steps" [N] int32.
    init="pca" (sklearn's default) makes the whole result a function of values alone; y0 [N, 2] overrides it."""
    x = _values32(values)
    N = int(x.shape[0])
    if y0 is not None:
        y = torch.as_tensor(y0).to(device=x.device, dtype=torch.float32).contiguous().clone()
        if tuple(y.shape) != (N, 2):
            raise ValueError(f"y0 must be [{N}, 2], got {tuple(y.shape)}")
    elif init == "pca":
        if x.shape[1] < 2:
            raise ValueError("init='pca' needs at least two columns")
        y = pca_init(x)
    else:
        raise ValueError(f"init = {init!r}: 'pca' or a y0")
    aff = tsne_affinities(x, perplexity)
    upd = torch.zeros(N, 2, dtype=torch.float64, device=x.device)
    gains = torch.ones(N, 2, dtype=torch.float64, device=x.device)
    log = tsne_run(x, aff, y, upd, gains, n_iter, 0, None, exaggeration, exaggeration_iters,
                   learning_rate=learning_rate)
    return {"y": y, "kl_log": log, "beta": aff["beta"], "steps": aff["steps"]}


def embedding_rows(n_rows: int, max_rows: int) -> np.ndarray:
    """The rows cond_embedding keeps: all of them, or every ceil(N / max_rows)-th when N > max_rows."""
    n_rows, max_rows = int(n_rows), int(max_rows)
    if max_rows < 2:
        raise ValueError(f"max_rows = {max_rows}: at least 2")
    stride = -(-n_rows // max_rows) if n_rows > max_rows else 1
    return np.arange(0, n_rows, stride, dtype=np.int64)


def cond_embedding(cond, expert, n_experts, max_rows=16384, n_iter=1000, perplexity=30.0):
    """The numeric content of the reference's plot_cond_pca_tsne as host numpy arrays.  cond [N, C] (all
    conditioning columns are used), expert [N] int32 (None: all zero); with n the rows kept:

      embed_rows                    [n]     the rows ::ceil(N / max_rows) when N > max_rows, else all
      embed_expert                  [n]     their experts
      pca                           [n, 2]  PCA scores
      pca_components                [2, C]
      pca_explained_variance        [2]
      pca_explained_variance_ratio  [2]
      tsne                          [n, 2]  exact t-SNE (perplexity 30, sklearn's schedule, init='pca')
      tsne_kl                       [ceil(n_iter / 50)]  the KL divergence every 50 iterations and at the end

    Everything crosses to the host in one copy at the end."""
    c = _values(cond)
    N, C = int(c.shape[0]), int(c.shape[1])
    dev = c.device
    if int(n_experts) < 1:
        raise ValueError(f"cond_embedding: n_experts = {n_experts}")
    if C < 2:
        raise ValueError(f"cond_embedding: {C} conditioning variables (at least two)")
    if expert is None:
        expert = torch.zeros(N, dtype=torch.int32, device=dev)
    if tuple(expert.shape) != (N,):
        raise ValueError(f"expert must be [{N}], got {tuple(expert.shape)}")
    keep = embedding_rows(N, max_rows)
    n = int(keep.size)
    if n < 2 or not perplexity < n:
        raise ValueError(f"cond_embedding: {n} rows for perplexity {perplexity}")
    stride = int(keep[1] - keep[0])
    sub, sub_expert = (c, expert.to(device=dev)) if stride == 1 else (c[::stride].contiguous(),
                                                                       expert.to(device=dev)[::stride])
    pca = pca_project(sub, 2)
    ts = tsne_embed(sub, perplexity=perplexity, n_iter=n_iter, y0=_scaled_scores(pca["scores"]))
    rows = torch.arange(0, N, stride, device=dev)
    parts = {"embed_rows": rows, "embed_expert": sub_expert, "pca": pca["scores"], "pca_components": pca["components"],
             "pca_explained_variance": pca["explained_variance"],
             "pca_explained_variance_ratio": pca["explained_variance_ratio"], "tsne": ts["y"],
             "tsne_kl": ts["kl_log"][:, 0]}
    flat = torch.cat([parts[k].reshape(-1).to(torch.float64) for k in EMBEDDING_KEYS]).cpu().numpy()   # the one copy
    out, at = {}, 0
    for k in EMBEDDING_KEYS:
        m = parts[k].numel()
        a = flat[at:at + m].reshape(tuple(parts[k].shape))
        at += m
        out[k] = a.astype(np.int64) if k in ("embed_rows", "embed_expert") else a.copy()
    return out
