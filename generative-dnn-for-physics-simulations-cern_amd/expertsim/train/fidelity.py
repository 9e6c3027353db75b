"""Sample-level fidelity and diversity on the device: k-NN precision, recall, density and coverage.

Every other evaluation statistic here is a one-dimensional marginal (channel sums, shower shapes) or a statistic
of the conditions; none sees a generated image as a point among the real images, so none can tell a sharp but
collapsed generator from a diverse but blurry one.  The metrics of Kynkaanniemi et al. 2019 (precision / recall)
and Naeem et al. 2020 (density / coverage, the ``prdc`` package) do, from three all-pairs distance matrices
(real-real, generated-generated, real-generated) over whole images.  HIP kernels (csrc/fidelity.hip, defined in
include/expertsim_hip.h):

* ``es_knn_radius``   per row the squared distance to its k-th neighbour within its segment (self included at 0);
* ``es_prdc_count``   the integer counts behind the four metrics, per row and per segment.

The distance is the sum of squared differences in fp64 in column order (not scikit-learn's expansion, which
cancels for near-duplicate images), no distance is ever stored, and the results are integers, so a rerun is
bit-equal.  Segments are es_router_dispatch's (joint + per expert) with its permutation as the row index on both
sides, as in train.utils.ws_across_experts_device.

The metrics depend on the number of samples on each side and on k: values are comparable only between runs at
equal settings.  There is no CPU fallback: without a HIP device every function raises hip.HipError.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ..segments import check_segments, expert_segments, ld, unit_stride_matrix, work_buffer

METRICS = ("precision", "recall", "density", "coverage")


def _matrix(x) -> torch.Tensor:
    """[rows, cols] fp32 on the device with unit column stride (images [rows, h, w] are flattened)."""
    if not torch.cuda.is_available():
        raise hip.HipError("the fidelity metrics need a HIP device (no CPU fallback)")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    hip.require_device(t)
    if t.dim() > 2:
        t = t.reshape(t.shape[0], -1)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"x must be [rows, cols] with at least one of each, got {tuple(t.shape)}")
    return unit_stride_matrix(t if t.dtype == torch.float32 else t.float())


def _segments(x, idx, seg, cap):
    """(idx, seg [n_seg, 2], n_seg, cap) as device int32 tensors; the default is one segment of all rows, and an
    idx longer than the rows is cut to them (no position past the rows is read)."""
    dev, rows = x.device, int(x.shape[0])
    if seg is None:
        seg = torch.tensor([[0, rows]], dtype=torch.int32, device=dev)
    seg = torch.as_tensor(seg).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    if idx is not None:
        idx = torch.as_tensor(idx).to(device=dev, dtype=torch.int32).contiguous()
        if idx.dim() != 1 or idx.shape[0] < rows:
            raise ValueError(f"idx must have the {rows} entries of x's rows, got {tuple(idx.shape)}")
        idx = idx[:rows]
    return idx, seg, check_segments(x, seg, idx), rows if cap is None else int(cap)


def knn_radius(x, k, idx=None, seg=None, cap=None, out=None) -> torch.Tensor:
    """es_knn_radius: radius2 [n_seg, cap] fp64 on the device, the squared distance of every segment member to its
    k-th neighbour inside the segment (the (k+1)-th smallest with itself included).  Entries past a segment's
    length keep what `out` held (a fresh result holds NaN there); a segment of at most k rows gives +inf."""
    x = _matrix(x)
    idx, seg, n_seg, cap = _segments(x, idx, seg, cap)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        need = hip.knn_radius_workspace(n_seg, cap, k)
        work = work_buffer(need, x.device)
        if out is None:
            out = torch.full((n_seg, max(cap, 0)), float("nan"), dtype=torch.float64, device=x.device)
        hip.call("es_knn_radius", hip.ptr(x), ld(x), rows, cols, hip.ptr(idx), hip.ptr(seg), n_seg, cap, int(k),
                 hip.ptr(out), hip.ptr(work), int(work.numel()) if need else 0, hip.stream_ptr())
    return out


def prdc_raw(real, fake, k, r_idx=None, r_seg=None, r_cap=None, f_idx=None, f_seg=None, f_cap=None,
             r_radius2=None, f_radius2=None, per_row=True):
    """es_knn_radius of each side (unless given) and es_prdc_count.  Returns the device tensors
    {"totals" int64 [n_seg, 8] = (n_r, n_f, valid, precision_hits, recall_hits, density_pairs, coverage_hits, 0),
    "r_radius2" [n_seg, r_cap], "f_radius2" [n_seg, f_cap] fp64, and with per_row "f_count" int32 [n_seg, f_cap],
    "r_hit" int32 [n_seg, r_cap], "r_min2" fp64 [n_seg, r_cap]}; entries past a segment's length are -1 / NaN."""
    real, fake = _matrix(real), _matrix(fake)
    if real.device != fake.device:
        raise ValueError("real and fake are on different devices")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real has {real.shape[1]} columns, fake {fake.shape[1]}")
    r_idx, r_seg, n_seg, r_cap = _segments(real, r_idx, r_seg, r_cap)
    f_idx, f_seg, f_n_seg, f_cap = _segments(fake, f_idx, f_seg, f_cap)
    if n_seg != f_n_seg:
        raise ValueError(f"{n_seg} real segments, {f_n_seg} generated")
    dev = real.device
    with torch.cuda.device(dev):
        if r_radius2 is None:
            r_radius2 = knn_radius(real, k, r_idx, r_seg, r_cap)
        if f_radius2 is None:
            f_radius2 = knn_radius(fake, k, f_idx, f_seg, f_cap)
        totals = torch.zeros(n_seg, 8, dtype=torch.int64, device=dev)
        f_count = r_hit = r_min2 = None
        if per_row:
            f_count = torch.full((n_seg, max(f_cap, 0)), -1, dtype=torch.int32, device=dev)
            r_hit = torch.full((n_seg, max(r_cap, 0)), -1, dtype=torch.int32, device=dev)
            r_min2 = torch.full((n_seg, max(r_cap, 0)), float("nan"), dtype=torch.float64, device=dev)
        need = hip.prdc_workspace(n_seg, r_cap, f_cap)
        work = work_buffer(need, dev)
        hip.call("es_prdc_count", hip.ptr(real), ld(real), int(real.shape[0]), hip.ptr(r_idx), hip.ptr(r_seg), r_cap,
                 hip.ptr(fake), ld(fake), int(fake.shape[0]), hip.ptr(f_idx), hip.ptr(f_seg), f_cap,
                 int(real.shape[1]), n_seg, int(k), hip.ptr(r_radius2), hip.ptr(f_radius2), hip.ptr(f_count),
                 hip.ptr(r_hit), hip.ptr(r_min2), hip.ptr(totals), hip.ptr(work), int(work.numel()) if need else 0,
                 hip.stream_ptr())
    out = {"totals": totals, "r_radius2": r_radius2, "f_radius2": f_radius2}
    if per_row:
        out.update(f_count=f_count, r_hit=r_hit, r_min2=r_min2)
    return out


def metrics_from_totals(totals, k) -> np.ndarray:
    """[n_seg, 4] float64 (precision, recall, density, coverage) from the host copy of es_prdc_count's totals:
    precision_hits / n_f, recall_hits / n_r, density_pairs / (k n_f), coverage_hits / n_r; NaN where the segment is
    not valid (either side has at most k rows).  A pure numpy function."""
    t = np.asarray(totals, dtype=np.int64).reshape(-1, 8)
    out = np.full((t.shape[0], 4), np.nan, dtype=np.float64)
    for s in range(t.shape[0]):
        n_r, n_f, valid = int(t[s, 0]), int(t[s, 1]), int(t[s, 2])
        if valid:
            out[s] = (t[s, 3] / n_f, t[s, 4] / n_r, t[s, 5] / (int(k) * n_f), t[s, 6] / n_r)
    return out


def prdc_device(real, fake, k=5, expert=None, n_experts=1, per_row=False):
    """The device half of `prdc`: prdc_raw's dict over the segments of `expert` (no host synchronisation)."""
    real, fake = _matrix(real), _matrix(fake)
    if expert is None:
        return prdc_raw(real, fake, k, per_row=per_row)
    if real.shape[0] != fake.shape[0] or tuple(expert.shape) != (real.shape[0],):
        raise ValueError(f"with an expert vector real, fake and expert are aligned: {real.shape[0]}, {fake.shape[0]}, "
                         f"{tuple(expert.shape)}")
    N = int(real.shape[0])
    perm, seg, _ = expert_segments(expert, n_experts, N, real.device, joint=True)
    raw = prdc_raw(real, fake, k, r_idx=perm, r_seg=seg, r_cap=N, f_idx=perm, f_seg=seg, f_cap=N, per_row=per_row)
    raw.update(perm=perm, seg=seg)
    return raw


def metrics_dict(totals, k, per_expert: bool) -> dict:
    """{"precision", "recall", "density", "coverage"} from segment 0 and `<name>_<e>` from segment 1 + e."""
    m = metrics_from_totals(totals, k)
    out = {name: float(m[0, i]) for i, name in enumerate(METRICS)}
    if per_expert:
        for e in range(m.shape[0] - 1):
            for i, name in enumerate(METRICS):
                out[f"{name}_{e}"] = float(m[1 + e, i])
    return out


def prdc(real, fake, k=5, expert=None, n_experts=1, details=False) -> dict:
    """Precision, recall, density and coverage of the generated rows `fake` against the real rows `real`
    ([rows, cols] or images [rows, h, w], fp32, on the device), at k nearest neighbours.

    expert [N] (then real and fake are aligned, N rows each): one es_router_dispatch; the joint metrics over all
    rows and `<name>_<e>` over the rows of expert e on both sides, with the dispatch permutation as the row index
    (no gather copy).  One device-to-host copy, of the integer totals; the four ratios are taken on the host in
    float64.  A segment in which either side has at most k rows gives NaN.  details=True adds prdc_raw's device
    tensors (the per-row ones included).

    The values depend on the sample counts and on k: compare runs at equal settings only."""
    raw = prdc_device(real, fake, k, expert, n_experts, per_row=bool(details))
    totals = raw["totals"].cpu().numpy()                                   # the one D2H copy
    out = metrics_dict(totals, k, expert is not None)
    if details:
        out.update(raw)
    return out
