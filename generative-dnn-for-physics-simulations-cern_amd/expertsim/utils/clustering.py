"""K-means of calorimeter images on the device -- the proton sets' ``expert_number`` column.

The reference ships no clustering code: its proton pickles arrive with an ``expert_number`` column that
``transform_data_for_training`` requires and ``evaluate_router`` compares the router against.  This module
produces that column from the images with scikit-learn's ``KMeans(algorithm="lloyd")`` run where the images
already are.  HIP kernels (csrc/cluster.hip, defined in include/expertsim_hip.h):

* ``es_kmeans_assign``    nearest centre of every row by the sum of squared differences (fp64, fixed order; the
  lowest centre wins a tie), the changed-label count and the inertia;
* ``es_kmeans_update``    the centres from the labels with scikit-learn's empty-cluster relocation, and the
  squared centre shift;
* ``es_kmeans_plusplus``  scikit-learn's greedy k-means++ on the caller's uniform draws.

`kmeans_raw` is ``sklearn.cluster._kmeans._kmeans_single_lloyd`` (same tolerance, stopping rules and closing
E-step) without the mean-centring, which the difference form of the distance does not need.  The draws of
`kmeans` come from numpy's ``Generator(Philox(key=[seed, restart]))``: expertsim/utils/philox.py restates the
device's dropout generator and yields 32-bit words, not uniform doubles.

There is no CPU fallback: without a HIP device every function raises hip.HipError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import hip
from ..segments import is_f64, ld, unit_stride_matrix, work_buffer


def _matrix(x, device=None) -> torch.Tensor:
    """[rows, cols] fp32 / fp64 on the device with unit column stride (other dtypes widen to fp64; host data is
    copied)."""
    if not torch.cuda.is_available():
        raise hip.HipError("clustering needs a HIP device (no CPU fallback)")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() != 2:
        raise ValueError(f"x must be [rows, cols], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if not t.is_cuda:
        t = t.to(torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return unit_stride_matrix(t)


def _check(x, K):
    rows, cols, K = int(x.shape[0]), int(x.shape[1]), int(K)
    if not (1 <= cols <= hip.KMEANS_MAX_COLS and 1 <= K <= hip.KMEANS_MAX_K and K <= rows <= hip.KMEANS_MAX_ROWS):
        raise ValueError(f"k-means of [{rows}, {cols}] into {K} clusters is outside 1 <= cols <= "
                         f"{hip.KMEANS_MAX_COLS}, 1 <= K <= {hip.KMEANS_MAX_K}, K <= rows <= {hip.KMEANS_MAX_ROWS}")
    return rows, cols, K


class _Lloyd:
    """The buffers of a Lloyd run over x and the two kernel calls on them."""

    def __init__(self, x, K):
        self.x = x
        self.rows, self.cols, self.K = _check(x, K)
        dev = x.device
        self.f64 = is_f64(x)
        self.need = hip.kmeans_workspace(self.rows, self.cols, self.K)
        self.work = work_buffer(self.need, dev)
        self.labels = [torch.zeros(self.rows, dtype=torch.int32, device=dev) for _ in range(2)]
        self.dist = torch.zeros(self.rows, dtype=torch.float64, device=dev)
        # [changed (int64 bits), inertia, shift, threshold]: what the host reads once per iteration
        self.stat = torch.zeros(4, dtype=torch.float64, device=dev)

    def _stat(self, i):
        return C.c_void_p(self.stat.data_ptr() + 8 * i)

    def assign(self, centres, label, label_old):
        hip.call("es_kmeans_assign", hip.ptr(self.x), self.f64, ld(self.x), self.rows, self.cols, hip.ptr(centres),
                 self.K, hip.ptr(label_old), hip.ptr(label), hip.ptr(self.dist), self._stat(0), self._stat(1),
                 hip.ptr(self.work), self.need, hip.stream_ptr())

    def update(self, label, centres_old, centres_new):
        hip.call("es_kmeans_update", hip.ptr(self.x), self.f64, ld(self.x), self.rows, self.cols, hip.ptr(label),
                 hip.ptr(self.dist), hip.ptr(centres_old), self.K, hip.ptr(centres_new), self._stat(2),
                 hip.ptr(self.work), self.need, hip.stream_ptr())


def mean_variance(x) -> torch.Tensor:
    """mean(var(x, axis=0)) (ddof = 0) as a device fp64 scalar, from the two kernels: the column means are
    es_kmeans_update's centre of one all-row cluster and the summed squared deviations es_kmeans_assign's
    inertia against it.  No host synchronisation."""
    x = _matrix(x)
    with torch.cuda.device(x.device):
        run = _Lloyd(x, 1)
        zero = torch.zeros(1, run.cols, dtype=torch.float64, device=x.device)
        mean = torch.empty_like(zero)
        run.update(run.labels[0], zero, mean)
        run.assign(mean, run.labels[1], None)
        return run.stat[1] / float(run.rows * run.cols)


def kmeans_raw(x, init_centres, tol=1e-4, max_iter=300, threshold=None):
    """scikit-learn's ``_kmeans_single_lloyd`` on device tensors: x [rows, cols] fp32 / fp64, init_centres
    [K, cols].  The threshold is tol * mean(var(x, axis=0)) (`mean_variance`; or the device scalar `threshold`);
    each iteration assigns, then updates; the loop stops when no label changed (strict convergence) or when the
    squared centre shift is <= the threshold, and a stop that was not strict is followed by one closing
    assignment against the final centres.  Returns (labels int32 [rows], centres fp64 [K, cols], inertia fp64
    scalar, n_iter): device tensors and a host int.  One 32-byte device-to-host copy per iteration (changed
    count, inertia, shift, threshold) and no other."""
    x = _matrix(x)
    c0 = torch.as_tensor(init_centres)
    if c0.dim() != 2 or c0.shape[1] != x.shape[1]:
        raise ValueError(f"init_centres must be [K, {x.shape[1]}], got {tuple(c0.shape)}")
    if int(max_iter) < 1:
        raise ValueError(f"max_iter = {max_iter}")
    with torch.cuda.device(x.device):
        run = _Lloyd(x, c0.shape[0])
        centres = c0.to(device=x.device, dtype=torch.float64).contiguous().clone()
        centres_new = torch.empty_like(centres)
        if threshold is None:
            threshold = mean_variance(x) * float(tol)
        run.stat[3] = threshold
        label, label_old = run.labels
        strict, n_iter = False, 0
        for i in range(int(max_iter)):
            run.assign(centres, label, label_old if i > 0 else None)
            run.update(label, centres, centres_new)
            centres, centres_new = centres_new, centres
            host = run.stat.cpu().numpy()                       # the iteration's one copy
            n_iter = i + 1
            if int(host.view(np.int64)[0]) == 0:
                strict = True
                break
            if host[2] <= host[3]:
                break
            label, label_old = label_old, label
        if not strict:
            label, label_old = label_old, label
            run.assign(centres, label, None)
        return label, centres, run.stat[1].clone(), n_iter


def kmeans_trials(K: int) -> int:
    """scikit-learn's candidates per k-means++ step: 2 + int(ln K)."""
    return 2 + int(np.log(int(K)))


def kmeans_plusplus_raw(x, K, draws):
    """es_kmeans_plusplus: greedy k-means++ of x [rows, cols] on the uniform draws [K, trials] in [0, 1) (row 0
    uses its first entry only).  Returns (centres fp64 [K, cols], index int32 [K]) device tensors; no host
    synchronisation."""
    x = _matrix(x)
    rows, cols, K = _check(x, K)
    u = torch.as_tensor(np.asarray(draws, dtype=np.float64) if not isinstance(draws, torch.Tensor) else draws)
    if u.dim() != 2 or u.shape[0] != K or not 1 <= u.shape[1] <= 8:
        raise ValueError(f"draws must be [{K}, 1..8], got {tuple(u.shape)}")
    u = u.to(device=x.device, dtype=torch.float64).contiguous()
    centres = torch.zeros(K, cols, dtype=torch.float64, device=x.device)
    index = torch.zeros(K, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        need = hip.kmeans_plusplus_workspace(rows, cols, K)
        work = work_buffer(need, x.device)
        hip.call("es_kmeans_plusplus", hip.ptr(x), is_f64(x), ld(x), rows, cols, K,
                 hip.ptr(u), int(u.shape[1]), hip.ptr(centres), hip.ptr(index), hip.ptr(work), need,
                 hip.stream_ptr())
    return centres, index


def _generator(seed, restart):
    return np.random.Generator(np.random.Philox(key=[int(seed), int(restart)]))


def kmeans(x, K, init="k-means++", n_init=10, seed=0, tol=1e-4, max_iter=300):
    """K-means with restarts: (labels int32 [rows], centres fp64 [K, cols], inertia fp64 scalar, n_iter) of the
    restart of lowest inertia, the lowest restart on a tie.  init: "k-means++" (`kmeans_plusplus_raw` on host
    draws), "random" (K distinct rows) or an array [K, cols] (one run).  The draws of restart r come from numpy's
    Generator(Philox(key=[seed, r])), so the result is a function of (x, K, seed, n_init) only and a rerun is
    bitwise equal."""
    x = _matrix(x)
    rows, cols, K = _check(x, K)
    given = not isinstance(init, str)
    if not given and init not in ("k-means++", "random"):
        raise ValueError(f"init = {init!r}: 'k-means++', 'random' or an array")
    n_init = 1 if given else int(n_init)
    if n_init < 1:
        raise ValueError(f"n_init = {n_init}")
    threshold = mean_variance(x) * float(tol)
    runs = []
    for r in range(n_init):
        if given:
            c0 = init
        elif init == "k-means++":
            c0, _ = kmeans_plusplus_raw(x, K, _generator(seed, r).random((K, kmeans_trials(K))))
        else:
            pick = np.sort(_generator(seed, r).choice(rows, size=K, replace=False))
            c0 = x[torch.from_numpy(pick).to(x.device), :cols].double()
        runs.append(kmeans_raw(x, c0, tol, max_iter, threshold))
    inertia = torch.stack([r[2] for r in runs]).cpu().numpy()
    return runs[int(np.argmin(inertia))]                        # argmin: the first of equal minima


def renumber_by_brightness(centres):
    """order [K]: the clusters by ascending sum of their centre's pixels, the original index first on a tie
    (host numpy, fp64); new number of cluster order[i] is i."""
    s = np.asarray(centres, dtype=np.float64).sum(axis=1)
    return np.argsort(s, kind="stable")


def cluster_images(images, K, n_init=10, seed=0, init="k-means++", tol=1e-4, max_iter=300, device=None):
    """images [N,H,W] (log1p domain, fp32 / fp64, host or device) -> (expert_number int64 [N], centres fp64
    [K, H*W], inertia fp64 scalar), device tensors.  Clusters are renumbered by ascending sum of their centre's
    pixels (ties: the original index), so the column does not depend on the order in which the initialisation
    found the clusters and cluster 0 is the faintest class of showers."""
    from .data_preparation import _as_device_images
    x = _as_device_images(images, device)
    x = x.reshape(x.shape[0], x.shape[1] * x.shape[2])          # a copy only when an image is not dense
    labels, centres, inertia, _ = kmeans(x, K, init=init, n_init=n_init, seed=seed, tol=tol, max_iter=max_iter)
    order = torch.from_numpy(renumber_by_brightness(centres.cpu().numpy())).to(x.device)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel(), device=x.device)
    return rank[labels.long()], centres[order], inertia
