"""Expert-specialisation diagnostics on the device -- the numbers behind the reference's plots
(train/loop.py:234-329, train/utils.py:470-620 plot_expert_heatmap / plot_expert_specialization,
utils/utils_eval.py:44-51 plot_proton_photonsum_histograms_shared), computed where the conditions, the routing
and the images already are.  Nothing is drawn: the results are arrays.

Two HIP kernels (csrc/diagnostics.hip, defined in include/expertsim_hip.h):

* ``es_segment_histogram``  per (segment, column) bin counts with numpy's (``right=False``:
  ``np.histogram(x, bins=e)``) or pandas' (``right=True``: ``pd.cut(x, bins=e, include_lowest=True)``) binning,
  exactly; the edges are the caller's or ``np.linspace(min, max, bins + 1)`` of each column over all rows.
* ``es_segment_kde``  per (segment, column) ``scipy.stats.gaussian_kde(d, bw_method='scott')`` on a grid, fp64,
  in a fixed summation order; pairs with fewer than ``min_samples`` members or a standard deviation below
  ``std_eps`` are flagged invalid and their density is NaN (the reference skips them).

A segment is an expert's samples: one ``es_router_dispatch`` turns the expert vector into perm / offs and the
kernels read the rows through perm (no gather copy).  There is no CPU fallback: without a HIP device the
functions raise hip.HipError.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ..segments import check_segments, expert_segments, is_f64, ld, unit_stride_matrix, work_buffer


def _values(values, device=None) -> torch.Tensor:
    """[N, C] fp32 / fp64 on the device with unit column stride (a 1-D input is one column; other dtypes widen
    to fp64; host data is copied)."""
    if not torch.cuda.is_available():
        raise hip.HipError("expert diagnostics need a HIP device (no CPU fallback)")
    t = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.asarray(values))
    if t.dim() == 1:
        t = t[:, None]
    if t.dim() != 2:
        raise ValueError(f"values must be [N] or [N, C], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if not t.is_cuda:
        t = t.to(torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device()))
    return unit_stride_matrix(t)


def segment_histogram_raw(x, seg, idx=None, seg_cap=None, bins=50, right=False, edges=None, cols=None):
    """es_segment_histogram on device tensors: x [N, >= cols] fp32 / fp64 (unit column stride, any row stride),
    seg [n_seg, 2] int32 bounds of positions in idx (int32 [N]; None: the rows themselves), seg_cap a host upper
    bound of a segment's length (default N), edges [cols, bins + 1] fp64 or None (np.linspace of each column's
    range over all N rows).  Returns (counts [n_seg, cols, bins] int32, edges [cols, bins + 1] fp64,
    outside [n_seg, cols] int32).  No host synchronisation; runs on the current stream."""
    hip.require_device(x)
    N = int(x.shape[0])
    cols = int(x.shape[1]) if cols is None else int(cols)
    bins = int(bins)
    S = check_segments(x, seg, idx)
    counts = torch.zeros(S, cols, max(bins, 0), dtype=torch.int32, device=x.device)
    outside = torch.zeros(S, cols, dtype=torch.int32, device=x.device)
    edges_out = torch.zeros(cols, max(bins, 0) + 1, dtype=torch.float64, device=x.device)
    if edges is not None:
        edges = torch.as_tensor(edges).to(device=x.device, dtype=torch.float64).contiguous()
        if tuple(edges.shape) != (cols, bins + 1):
            raise ValueError(f"edges must be [{cols}, {bins + 1}], got {tuple(edges.shape)}")
        if N == 0 or S == 0:
            edges_out.copy_(edges)
    with torch.cuda.device(x.device):
        need = hip.segment_histogram_workspace(cols, bins)
        work = work_buffer(need, x.device)
        hip.call("es_segment_histogram", hip.ptr(x), is_f64(x), ld(x), N, cols,
                 hip.ptr(idx), hip.ptr(seg), S, int(seg_cap) if seg_cap is not None else max(N, 1), bins,
                 1 if right else 0, hip.ptr(edges), hip.ptr(edges_out), hip.ptr(counts), hip.ptr(outside),
                 hip.ptr(work), need, hip.stream_ptr())
    return counts, edges_out, outside


def segment_kde_raw(x, seg, idx=None, seg_cap=None, points=100, grid=None, min_samples=5, std_eps=1e-12, cols=None):
    """es_segment_kde on device tensors (arguments as segment_histogram_raw; grid [cols, points] fp64 or None:
    np.linspace of each column's range over all N rows, a constant column widened by 1e-6 either side).
    Returns {"density" [n_seg, cols, points], "grid" [cols, points], "bw" [n_seg, cols], "sd" [n_seg, cols]
    (fp64), "valid" [n_seg, cols] (int32)}; an invalid pair has a NaN density row and bw = sd = 0.  No host
    synchronisation; runs on the current stream."""
    hip.require_device(x)
    N = int(x.shape[0])
    cols = int(x.shape[1]) if cols is None else int(cols)
    points = int(points)
    S = check_segments(x, seg, idx)
    dev = x.device
    density = torch.full((S, cols, max(points, 0)), float("nan"), dtype=torch.float64, device=dev)
    bw = torch.zeros(S, cols, dtype=torch.float64, device=dev)
    sd = torch.zeros(S, cols, dtype=torch.float64, device=dev)
    valid = torch.zeros(S, cols, dtype=torch.int32, device=dev)
    grid_out = torch.zeros(cols, max(points, 0), dtype=torch.float64, device=dev)
    if grid is not None:
        grid = torch.as_tensor(grid).to(device=dev, dtype=torch.float64).contiguous()
        if tuple(grid.shape) != (cols, points):
            raise ValueError(f"grid must be [{cols}, {points}], got {tuple(grid.shape)}")
        if N == 0 or S == 0:
            grid_out.copy_(grid)
    cap = int(seg_cap) if seg_cap is not None else max(N, 1)
    with torch.cuda.device(dev):
        need = hip.segment_kde_workspace(S, cols, points, min(cap, max(N, 1))) if S > 0 else 0
        work = work_buffer(need, dev)
        hip.call("es_segment_kde", hip.ptr(x), is_f64(x), ld(x), N, cols, hip.ptr(idx),
                 hip.ptr(seg), S, cap, points, hip.ptr(grid), int(min_samples), float(std_eps), hip.ptr(grid_out),
                 hip.ptr(density), hip.ptr(bw), hip.ptr(valid), hip.ptr(sd), hip.ptr(work), need, hip.stream_ptr())
    return {"density": density, "grid": grid_out, "bw": bw, "sd": sd, "valid": valid}


def segment_histogram(values, expert=None, n_experts=1, bins=50, right=False, edges=None):
    """Per expert and per column of values [N, C] (or [N]) the bin counts: (counts [E, C, bins] int32,
    edges [C, bins + 1] fp64, outside [E, C] int32), device tensors.  right=False is np.histogram's binning,
    right=True pd.cut(include_lowest=True)'s; edges None: np.linspace(min, max, bins + 1) per column over all
    N samples.  expert [N] int32 (None: one segment over all samples)."""
    x = _values(values)
    perm, seg, _ = expert_segments(expert, n_experts, x.shape[0], x.device)
    return segment_histogram_raw(x, seg, perm, None, bins, right, edges)


def segment_kde(values, expert=None, n_experts=1, points=100, grid=None, min_samples=5, std_eps=1e-12):
    """Per expert and per column of values [N, C] (or [N]) the Gaussian KDE with Scott's bandwidth on a grid of
    `points` values (grid None: np.linspace(min, max, points) per column over all N samples): the dict of
    segment_kde_raw, device tensors."""
    x = _values(values)
    perm, seg, _ = expert_segments(expert, n_experts, x.shape[0], x.device)
    return segment_kde_raw(x, seg, perm, None, points, grid, min_samples, std_eps)


DIAGNOSTIC_KEYS = ("expert_count", "photon_sum_hist", "photon_sum_edges", "cond_hist", "cond_edges", "cond_kde",
                   "cond_kde_grid", "cond_kde_bw", "cond_kde_valid", "cat_values", "cat_count")


def expert_diagnostics(cond, expert, n_experts, photon_sum, names=None, bins=50, points=100):
    """The numeric content of the reference's specialisation plots as host numpy arrays.  cond [N, C]
    (C - 1 continuous variables, then one categorical), expert [N] int32, photon_sum [N]; E = n_experts:

      expert_count     [E]               samples routed to each expert
      photon_sum_hist  [E, bins]         np.histogram binning over the range of all samples
      photon_sum_edges [bins + 1]
      cond_hist        [E, C, bins]      pd.cut(include_lowest=True) binning per conditioning variable
      cond_edges       [C, bins + 1]
      cond_kde         [E, C - 1, points]  Gaussian KDE (Scott) of the continuous variables; NaN where invalid
      cond_kde_grid    [C - 1, points]
      cond_kde_bw      [E, C - 1]
      cond_kde_valid   [E, C - 1]        0: fewer than 5 samples or a standard deviation below 1e-12
      cat_values       [K]               distinct values of the last variable
      cat_count        [E, K]            samples per expert and distinct value
      cond_names       [C]               only with names

    One es_router_dispatch serves every kernel call.  torch.unique on the last variable is the one place that
    synchronises before the end (K sizes a tensor); everything crosses to the host in one copy."""
    c = _values(cond)
    N, C = int(c.shape[0]), int(c.shape[1])
    E = int(n_experts)
    dev = c.device
    if C < 2:
        raise ValueError(f"expert_diagnostics: {C} conditioning variables (at least one continuous and the categorical)")
    if names is not None and len(names) != C:
        raise ValueError(f"expert_diagnostics: {len(names)} names for {C} conditioning variables")
    ps = _values(photon_sum)
    if tuple(ps.shape) != (N, 1):
        raise ValueError(f"expert_diagnostics: photon_sum {tuple(ps.shape)} for {N} conditions")
    if expert is None:
        expert = torch.zeros(N, dtype=torch.int32, device=dev)
    perm, seg, offs = expert_segments(expert, E, N, dev)
    ps_hist, ps_edges, _ = segment_histogram_raw(ps, seg, perm, None, bins, False)
    c_hist, c_edges, _ = segment_histogram_raw(c, seg, perm, None, bins, True)
    kde = segment_kde_raw(c, seg, perm, None, points, cols=C - 1)
    cat_values, codes = torch.unique(c[:, C - 1], return_inverse=True)
    K = int(cat_values.numel())
    cat_edges = (torch.arange(K + 1, dtype=torch.float64, device=dev) - 0.5)[None]
    cat_count, _, _ = segment_histogram_raw(codes.to(torch.float64)[:, None], seg, perm, None, max(K, 1), False,
                                            cat_edges if K > 0 else None)
    parts = {"expert_count": (offs[1:] - offs[:-1]), "photon_sum_hist": ps_hist[:, 0], "photon_sum_edges": ps_edges[0],
             "cond_hist": c_hist, "cond_edges": c_edges, "cond_kde": kde["density"], "cond_kde_grid": kde["grid"],
             "cond_kde_bw": kde["bw"], "cond_kde_valid": kde["valid"], "cat_values": cat_values,
             "cat_count": cat_count[:, 0, :K]}
    flat = torch.cat([parts[k].reshape(-1).to(torch.float64) for k in DIAGNOSTIC_KEYS]).cpu().numpy()   # the one copy
    out, at = {}, 0
    for k in DIAGNOSTIC_KEYS:
        n = parts[k].numel()
        a = flat[at:at + n].reshape(tuple(parts[k].shape))
        at += n
        integer = k in ("expert_count", "photon_sum_hist", "cond_hist", "cond_kde_valid", "cat_count")
        out[k] = a.astype(np.int64) if integer else a.copy()
    if names is not None:
        out["cond_names"] = np.asarray([str(n) for n in names])
    return out


def confusion_matrix(pred, target, n_pred, n_true):
    """es_confusion_matrix: (counts int64 [n_true, n_pred], invalid int64 [1]) device tensors; counts[t, p] = the
    pairs with target == t and pred == p, invalid = the pairs with an index outside either range (in no cell).
    pred / target: integer tensors [n], host or device.  No host synchronisation; runs on the current stream."""
    if not torch.cuda.is_available():
        raise hip.HipError("the confusion matrix needs a HIP device (no CPU fallback)")
    p = pred if isinstance(pred, torch.Tensor) else torch.as_tensor(np.asarray(pred))
    t = target if isinstance(target, torch.Tensor) else torch.as_tensor(np.asarray(target))
    if p.dim() != 1 or t.shape != p.shape:
        raise ValueError(f"pred {tuple(p.shape)} and target {tuple(t.shape)} must be equal-length vectors")
    if p.is_floating_point() or t.is_floating_point():
        raise ValueError("pred and target must hold integers")
    n_pred, n_true = int(n_pred), int(n_true)
    if n_pred < 1 or n_true < 1 or n_pred * n_true > hip.CONFUSION_MAX_CELLS:
        raise ValueError(f"confusion matrix {n_true} x {n_pred} outside 1 <= cells <= {hip.CONFUSION_MAX_CELLS}")
    dev = p.device if p.is_cuda else (t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    lo, hi = torch.iinfo(torch.int32).min, torch.iinfo(torch.int32).max
    p = p.to(dev).clamp(lo, hi).to(torch.int32).contiguous()    # a wider index stays outside the ranges
    t = t.to(dev).clamp(lo, hi).to(torch.int32).contiguous()
    counts = torch.zeros(n_true, n_pred, dtype=torch.int64, device=dev)
    invalid = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        hip.call("es_confusion_matrix", hip.ptr(p), hip.ptr(t), int(p.numel()), n_true, n_pred, hip.ptr(counts),
                 hip.ptr(invalid), hip.stream_ptr())
    return counts, invalid


def agreement_metrics(counts) -> dict:
    """Host numbers from a confusion matrix counts[target, pred] (int, any shape; classes are 0 .. max(shape)-1):

      accuracy          trace / total (sklearn.metrics.accuracy_score)
      precision, recall, f1   macro averages over the classes that occur in pred or target, an undefined term
                        (0 / 0) counting as 0: precision_recall_fscore_support(average="macro", zero_division=0)
      adjusted_rand     sklearn.metrics.adjusted_rand_score, from the pair counts of the matrix
      matched_accuracy  the accuracy under the best one-to-one relabelling of the predictions
                        (scipy.optimize.linear_sum_assignment on the matrix)

    The last two do not depend on how the two sides number their classes.  An empty matrix gives zeros (and
    adjusted_rand 1, sklearn's value for trivial labelings)."""
    from scipy.optimize import linear_sum_assignment
    cm = np.asarray(counts, dtype=np.int64)
    k = max(cm.shape)
    sq = np.zeros((k, k), dtype=np.int64)
    sq[:cm.shape[0], :cm.shape[1]] = cm
    total = int(sq.sum())
    tp = np.diag(sq).astype(np.float64)
    n_t, n_p = sq.sum(axis=1).astype(np.float64), sq.sum(axis=0).astype(np.float64)
    present = (n_t + n_p) > 0

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(a), where=b > 0)

    prec, rec = ratio(tp, n_p), ratio(tp, n_t)
    f1 = ratio(2.0 * tp, n_t + n_p)
    macro = lambda v: float(v[present].mean()) if present.any() else 0.0
    # adjusted Rand index from the pair confusion matrix, in Python integers (no overflow)
    sum_sq = int((sq.astype(object) ** 2).sum())
    c11 = sum_sq - total
    c01 = int((sq.astype(object) * sq.sum(axis=0).astype(object)[None, :]).sum()) - sum_sq
    c10 = int((sq.astype(object) * sq.sum(axis=1).astype(object)[:, None]).sum()) - sum_sq
    c00 = total * total - c01 - c10 - sum_sq
    tn, fp, fn, tp2 = c00, c01, c10, c11
    if fn == 0 and fp == 0:
        ari = 1.0
    else:
        ari = 2.0 * (tp2 * tn - fn * fp) / ((tp2 + fn) * (fn + tn) + (tp2 + fp) * (fp + tn))
    rows, cols = linear_sum_assignment(-sq)
    return {"accuracy": float(np.diag(sq).sum()) / total if total else 0.0, "precision": macro(prec),
            "recall": macro(rec), "f1": macro(f1), "adjusted_rand": float(ari),
            "matched_accuracy": float(sq[rows, cols].sum()) / total if total else 0.0}


def router_agreement(pred, target, n_pred, n_true) -> dict:
    """How well the router's arg-max `pred` [n] agrees with a class vector `target` [n] (the proton sets'
    expert_number): {"confusion" int64 [n_true, n_pred] (host), "invalid" (pairs outside either range, counted
    in no cell), and the numbers of `agreement_metrics`}.  The matrix comes from es_confusion_matrix; one copy
    brings it to the host.  Cluster numbers and expert numbers are unrelated namings, so matched_accuracy and
    adjusted_rand are the ones to read across them."""
    counts, invalid = confusion_matrix(pred, target, n_pred, n_true)
    flat = torch.cat([counts.reshape(-1), invalid]).cpu().numpy()          # the one copy
    cm = flat[:-1].reshape(int(n_true), int(n_pred)).copy()
    return {"confusion": cm, "invalid": int(flat[-1]), **agreement_metrics(cm)}


def save_diagnostics(path, diag) -> str:
    """Write the dict of expert_diagnostics as an .npz; returns the path written.  A nested dict
    ("router_agreement") is written as "<key>.<entry>" arrays."""
    path = str(path)
    if not path.endswith(".npz"):
        path += ".npz"
    flat = {}
    for k, v in diag.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{sk}": np.asarray(sv) for sk, sv in v.items()})
        else:
            flat[k] = np.asarray(v)
    np.savez(path, **flat)
    return path
