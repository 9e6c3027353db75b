"""Conditional fidelity on the device: the response and resolution of every observable as a function of one
conditioning variable, real against generated, bin by bin.

Every other metric of the evaluation is marginal: it compares the pooled real rows with the pooled generated rows,
and a generator that ignores its condition but reproduces the pooled distribution scores perfectly on all of them.
The product is a conditional simulator, and what is checked first on one is the median and the width of each
observable per bin of the primary's energy.  The test rows are aligned with their conditions (real row i and
generated row i share cond[i]), so the segments of the segment kernels only have to be condition bins instead of
experts.  HIP kernels (csrc/quantile.hip, csrc/bins.hip, defined in include/expertsim_hip.h):

* ``es_segment_quantiles``  order statistics per (segment, column) and side by numpy's default quantile rule, bit
                            for bit, from the tagged sort es_wasserstein_1d uses;
* ``es_bin_dispatch``       rows to bins from device-resident edges (np.searchsorted side="left", pandas' (a, b]
                            intervals) and the stable grouping of the rows by (expert, bin), no atomics, no host
                            synchronisation.

There is no CPU fallback: without a HIP device every device function raises hip.HipError.  The host half
(`summary_from_tables`) is pure numpy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import hip
from ..segments import ld, work_buffer
from .classifier import _sides, rank_stats
from .distances import _segments, _table, segment_moments

PROBS = (0.16, 0.5, 0.84)               # the band of a Gaussian's one standard deviation around the median
STATS = ("ws", "bias", "width", "ks")


def _need_device():
    if not torch.cuda.is_available():
        raise hip.HipError("the conditional profiles need a HIP device (no CPU fallback)")


# ------------------------------------------------------------------------------------------ thin wrappers
def segment_quantiles(u, v=None, probs=PROBS, u_idx=None, u_seg=None, u_cap=None, v_idx=None, v_seg=None, v_cap=None,
                      out=None):
    """es_segment_quantiles: (q fp64 [n_seg, channels, 2, n_q], count int32 [n_seg, 2]) on the device for the columns
    of u / v [rows, channels] (cast to fp64): q[s, c, side, k] is np.quantile of column c of segment s's rows of side
    0 (u) or 1 (v) at probs[k], bit for bit, NaN where that side is empty there; count[s, side] the rows.  v=None is
    the one-sample form (side 1 is empty everywhere).  probs: 1 .. hip.QUANTILE_MAX_Q host numbers in [0, 1].
    Segments, idx and caps as train.utils.wasserstein_1d_device.  Values must be finite; -0.0 reads as +0.0.
    out: the two tensors to write into."""
    _need_device()
    u = _table(u).double()
    probs = [float(p) for p in np.atleast_1d(np.asarray(probs, dtype=np.float64))]
    if v is None:
        u_idx, u_seg, n_seg = _segments(u, u_idx, u_seg)
        u_cap = int(u.shape[0]) if u_cap is None else int(u_cap)
        v_rows, v_ld, v_cap = 0, 0, 0
    else:
        v = _table(v).double()
        u_idx, u_seg, u_cap, v_idx, v_seg, v_cap, n_seg = _sides(u, v, u_idx, u_seg, u_cap, v_idx, v_seg, v_cap)
        v_rows, v_ld = int(v.shape[0]), ld(v)
    ch, dev, n_q = int(u.shape[1]), u.device, len(probs)
    host = (C.c_double * max(n_q, 1))(*probs)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(n_seg, ch, 2, max(n_q, 1), dtype=torch.float64, device=dev),
                   torch.empty(n_seg, 2, dtype=torch.int32, device=dev))
        q, count = out
        need = hip.segment_quantiles_workspace(n_seg, ch, u_cap, v_cap)
        work = work_buffer(need, dev)
        hip.call("es_segment_quantiles", hip.ptr(u), ld(u), int(u.shape[0]), hip.ptr(u_idx), hip.ptr(u_seg),
                 hip.ptr(v), v_ld, v_rows, hip.ptr(v_idx) if v is not None else None,
                 hip.ptr(v_seg) if v is not None else None, n_seg, ch, u_cap, v_cap, C.cast(host, C.c_void_p), n_q,
                 hip.ptr(q), hip.ptr(count), hip.ptr(work), int(work.numel()) if need else 0, hip.stream_ptr())
    return q, count


def _column(x):
    """x as a 1-D fp32 / fp64 device tensor (a strided view stays a view: the kernel takes an element stride)."""
    _need_device()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    hip.require_device(t)
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.shape[0] < 1:
        raise ValueError(f"x must be [rows] with at least one row, got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.float64):
        t = t.double()
    if t.shape[0] > 1 and t.stride(0) < 1:
        t = t.contiguous()
    return t


def bin_dispatch(x, edges, n_bins, expert=None, n_experts=1, out=None):
    """es_bin_dispatch: (bin int32 [rows], perm int32 [rows], offs int32 [n_classes + 1]) on the device for x [rows]
    (fp32 or fp64, any element stride) and the ascending device edges fp64 [n_bins - 1] (None when n_bins == 1):
    bin = np.searchsorted(edges, x, side="left") (a value equal to an edge belongs to the lower bin), class = bin or,
    with expert int32 [rows], clamp(expert, 0, n_experts - 1) * n_bins + bin; perm / offs group the rows by class in
    es_router_dispatch's layout, each group in ascending row order (np.argsort(class, kind="stable")).  n_bins <=
    hip.BINS_MAX, n_classes <= 1024, rows <= 2^20.  No host synchronisation.  out: the three tensors to write into."""
    x = _column(x)
    rows, dev, B = int(x.shape[0]), x.device, int(n_bins)
    E = int(n_experts)
    if expert is None and E != 1:
        raise ValueError(f"n_experts = {E} needs an expert vector")
    if edges is not None:
        hip.require_device(edges)
        edges = edges.to(torch.float64).reshape(-1).contiguous()
        if edges.numel() != max(B - 1, 0) or edges.device != dev:
            raise ValueError(f"edges must be the {B - 1} device edges of {B} bins, got {tuple(edges.shape)}")
        if edges.numel() == 0:
            edges = None
    if expert is not None:
        if tuple(expert.shape) != (rows,):
            raise ValueError(f"expert must be [{rows}], got {tuple(expert.shape)}")
        expert = expert.to(device=dev, dtype=torch.int32).contiguous()
    n_classes = B * (E if expert is not None else 1)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(rows, dtype=torch.int32, device=dev), torch.empty(rows, dtype=torch.int32, device=dev),
                   torch.empty(max(n_classes, 0) + 1, dtype=torch.int32, device=dev))
        bins, perm, offs = out
        need = hip.bin_dispatch_workspace(rows, n_classes)
        work = work_buffer(need, dev)
        hip.call("es_bin_dispatch", hip.ptr(x), 1 if x.dtype == torch.float64 else 0, max(int(x.stride(0)), 1), rows,
                 hip.ptr(edges), B, hip.ptr(expert), E, hip.ptr(bins), hip.ptr(perm), hip.ptr(offs), hip.ptr(work),
                 int(work.numel()), hip.stream_ptr())
    return bins, perm, offs


def bin_edges(by, n_bins) -> torch.Tensor:
    """The n_bins - 1 edges of equally populated bins of by [N]: its quantiles at k / n_bins, k = 1 .. n_bins - 1
    (np.quantile, bit for bit), fp64 on the device, from one one-sample segment_quantiles call per
    hip.QUANTILE_MAX_Q edges.  The edges never leave the device."""
    by = _column(by)
    B = int(n_bins)
    if not 1 <= B <= hip.BINS_MAX:
        raise ValueError(f"n_bins = {B} outside 1 .. {hip.BINS_MAX}")
    col = by.double().reshape(-1, 1)
    parts = []
    for k0 in range(1, B, hip.QUANTILE_MAX_Q):
        probs = [k / B for k in range(k0, min(k0 + hip.QUANTILE_MAX_Q, B))]
        q, _ = segment_quantiles(col, None, probs)
        parts.append(q[0, 0, 0, :len(probs)])
    if not parts:
        return torch.empty(0, dtype=torch.float64, device=by.device)
    return torch.cat(parts).contiguous()


# ------------------------------------------------------------------------------------------ host half
def scalar_keys(names, n_experts=0) -> list:
    """The scalar keys of `profile` for the observables `names`, in the order summary_from_tables writes them;
    n_experts = 0: without an expert vector."""
    keys = ["cond_ws"] + [f"cond_{s}_{o}" for o in names for s in STATS]
    for e in range(int(n_experts)):
        keys += [f"cond_ws_{e}"] + [f"cond_ws_{o}_{e}" for o in names]
    return keys


def weighted_mean(count, values) -> np.ndarray:
    """sum_b n_b x_b / sum_b n_b over the bins b with n_b > 0, per column of values [B, cols]: the products are added
    in bin order from 0.0, the counts as integers, one division.  NaN where no bin has a row."""
    count = np.asarray(count, dtype=np.int64)
    values = np.asarray(values, dtype=np.float64)
    num, den = np.zeros(values.shape[1], dtype=np.float64), 0
    for b in range(values.shape[0]):
        if count[b] > 0:
            num = num + np.float64(count[b]) * values[b]
            den += int(count[b])
    return num / np.float64(den) if den else np.full(values.shape[1], np.nan)


def _index(probs, p):
    for k, v in enumerate(probs):
        if float(v) == p:
            return k
    raise ValueError(f"probs {tuple(probs)} must hold {p}: the scalars need the 16 % / 50 % / 84 % quantiles")


def _mean_in_order(x) -> float:
    t = 0.0
    for v in x:
        t = t + float(v)
    return t / len(x)


def summary_from_tables(count, q_real, q_gen, ws, ks, scale, probs=PROBS, names=None, n_experts=0) -> dict:
    """The scalars of `profile` from the host copies of its tables (numpy, float64): count [S, n_bins], q_real /
    q_gen [S, n_bins, cols, Q], ws / ks [S, n_bins, cols], scale [cols]; row 0 of S the joint bins, row 1 + e expert
    e's.  With n_b the rows of joint bin b, weighted_mean over the non-empty bins and s_o = scale[o]:

      cond_ws_<o>     mean of the per-bin Wasserstein-1 distance W1_b: the binned estimate of E_c W1(P(o|c), Q(o|c))
      cond_bias_<o>   mean of |median_gen - median_real| / s_o
      cond_width_<o>  mean of |w_gen - w_real| / s_o, w = (q84 - q16) / 2
      cond_ks_<o>     mean of the per-bin Kolmogorov-Smirnov statistic
      cond_ws         the mean over o (in order) of cond_ws_<o> / s_o: one number for model selection
      cond_ws_<o>_<e>, cond_ws_<e>   the same over expert e's bins (n_experts > 0); NaN where it has no row."""
    count = np.asarray(count, dtype=np.int64)
    q_real, q_gen = np.asarray(q_real, dtype=np.float64), np.asarray(q_gen, dtype=np.float64)
    ws, ks, scale = (np.asarray(a, dtype=np.float64) for a in (ws, ks, scale))
    cols = ws.shape[2]
    names = tuple(names) if names is not None else tuple(f"c{o}" for o in range(cols))
    if len(names) != cols:
        raise ValueError(f"{len(names)} names for {cols} columns")
    i16, i50, i84 = (_index(probs, p) for p in PROBS)
    n = count[0]
    bias = np.abs(q_gen[0, :, :, i50] - q_real[0, :, :, i50]) / scale
    w_real = (q_real[0, :, :, i84] - q_real[0, :, :, i16]) / 2.0
    w_gen = (q_gen[0, :, :, i84] - q_gen[0, :, :, i16]) / 2.0
    width = np.abs(w_gen - w_real) / scale
    empty = n == 0                                         # NaN quantiles there; weighted_mean skips the bin
    bias[empty], width[empty] = 0.0, 0.0
    cws = weighted_mean(n, ws[0])
    vals = {"ws": cws, "bias": weighted_mean(n, bias), "width": weighted_mean(n, width),
            "ks": weighted_mean(n, ks[0])}
    out = {"cond_ws": _mean_in_order(cws / scale)}
    for o, name in enumerate(names):
        for s in STATS:
            out[f"cond_{s}_{name}"] = float(vals[s][o])
    for e in range(int(n_experts)):
        w = weighted_mean(count[1 + e], ws[1 + e])
        out[f"cond_ws_{e}"] = _mean_in_order(w / scale)
        for o, name in enumerate(names):
            out[f"cond_ws_{name}_{e}"] = float(w[o])
    return out


# ------------------------------------------------------------------------------------------ profile
def profile_device(real, fake, by, n_bins=8, expert=None, n_experts=1, probs=PROBS) -> dict:
    """The device half of `profile`: {"edges" fp64 [n_bins - 1], "bin" int32 [N], "count" int32 [S, n_bins], "q_real"
    / "q_gen" fp64 [S, n_bins, cols, Q], "mean_real" / "mean_gen" / "std_real" / "std_gen" [S, n_bins, cols], "ws" /
    "ks" [S, n_bins, cols], "scale" [cols], "q_all" [cols, 2, Q], "seg" int32 [1 + S n_bins, 2], "idx"} with no host
    synchronisation; S = 1 (the joint bins) + n_experts with an expert vector."""
    _need_device()
    from .utils import wasserstein_1d_device
    real, fake = _table(real).double().contiguous(), _table(fake).double().contiguous()
    N, cols, dev = int(real.shape[0]), int(real.shape[1]), real.device
    if tuple(fake.shape) != (N, cols):
        raise ValueError(f"real and fake are aligned row by row: {tuple(real.shape)} against {tuple(fake.shape)}")
    by = _column(by)
    if by.shape[0] != N or by.device != dev:
        raise ValueError(f"by must be the [{N}] conditions of the rows on their device, got {tuple(by.shape)}")
    B, E = int(n_bins), int(n_experts)
    probs = tuple(float(p) for p in probs)
    i16, i84 = _index(probs, PROBS[0]), _index(probs, PROBS[2])
    _index(probs, PROBS[1])
    with torch.cuda.device(dev):
        edges = bin_edges(by, B)
        bins, perm, offs = bin_dispatch(by, edges, B)
        starts, idx = [offs], perm
        if expert is not None:
            _, perm_e, offs_e = bin_dispatch(by, edges, B, expert, E)
            # two perms over one table: the table stacked (distances._aligned), the second perm behind the first
            real, fake = torch.cat([real, real]), torch.cat([fake, fake])
            idx = torch.cat([perm, perm_e + N]).contiguous()
            starts.append(offs_e + N)
        S = 1 + (E if expert is not None else 0)
        seg = torch.empty(1 + S * B, 2, dtype=torch.int32, device=dev)
        seg[0, 0], seg[0, 1] = 0, N                                    # all rows first
        seg[1:1 + B, 0], seg[1:1 + B, 1] = offs[:-1], offs[1:]
        if expert is not None:
            seg[1 + B:, 0], seg[1 + B:, 1] = starts[1][:-1], starts[1][1:]
        q, cnt = segment_quantiles(real, fake, probs, idx, seg, N, idx, seg, N)
        _, mean_r, cov_r = segment_moments(real, idx, seg)
        _, mean_g, cov_g = segment_moments(fake, idx, seg)
        ws = wasserstein_1d_device(real, fake, seg, seg, idx, idx, N, N)
        rank = rank_stats(real, fake, idx, seg, N, idx, seg, N)
        pairs = (rank[..., 0] * rank[..., 1]).clamp_min(1).double()
        ks = rank[..., 3].double() / pairs
        w_all = (q[0, :, 0, i84] - q[0, :, 0, i16]) / 2.0
        scale = torch.where(w_all == 0, torch.ones_like(w_all), w_all)
        Q = len(probs)

        def bins_of(t, *tail):
            return t[1:].reshape(S, B, *tail)

        std_r = torch.diagonal(cov_r, dim1=1, dim2=2).clamp_min(0).sqrt()
        std_g = torch.diagonal(cov_g, dim1=1, dim2=2).clamp_min(0).sqrt()
    return {"edges": edges, "bin": bins, "count": bins_of(cnt[:, 0]), "q_real": bins_of(q[:, :, 0, :], cols, Q),
            "q_gen": bins_of(q[:, :, 1, :], cols, Q), "mean_real": bins_of(mean_r, cols),
            "mean_gen": bins_of(mean_g, cols), "std_real": bins_of(std_r, cols), "std_gen": bins_of(std_g, cols),
            "ws": bins_of(ws, cols), "ks": bins_of(ks, cols), "scale": scale, "q_all": q[0], "seg": seg, "idx": idx}


HOST_TABLES = ("count", "q_real", "q_gen", "ws", "ks", "scale")


def profile(real, fake, by, n_bins=8, expert=None, n_experts=1, probs=PROBS, names=None, details=False) -> dict:
    """The conditional profile of the generated rows `fake` against the real rows `real` ([N, cols] observable tables
    on the device, ALIGNED row by row: row i of both belongs to the condition by[i]; by [N], fp32 or fp64).

    The n_bins bins are equally populated in `by`: their edges are by's quantiles at k / n_bins (`bin_edges`), a
    row's bin the number of edges strictly below its value (pandas' (a, b] intervals).  Segments: all rows, then the
    n_bins joint bins, then with expert [N] the n_experts x n_bins (expert, bin) classes on the same edges, from two
    es_bin_dispatch calls; one index serves both sides because the rows are aligned.  Over those segments one
    es_segment_quantiles (probs must hold 0.16, 0.5 and 0.84), one es_segment_moments per side, one
    es_wasserstein_1d and one es_rank_stats call, then torch fp64 arithmetic on the device and ONE small
    device-to-host copy.  The scalars are summary_from_tables': cond_ws, cond_ws_<o> / cond_bias_<o> /
    cond_width_<o> / cond_ks_<o> per observable name o (names; default c0, c1, ..), and with an expert vector
    cond_ws_<e> / cond_ws_<o>_<e>, NaN where the expert has no row.  s_o, the unit of bias and width, is the real
    side's (q84 - q16) / 2 over all rows (1 where that is 0).

    details=True adds the curves themselves, the numbers of a response / resolution plot, as device tensors (see
    profile_device): edges, count, q_real, q_gen, mean_*, std_*, ws, ks, scale, bin.  An empty bin has count 0, NaN
    quantiles and moments, and 0 in ws and ks; a bin of one row has NaN in std_*."""
    raw = profile_device(real, fake, by, n_bins, expert, n_experts, probs)
    flat = torch.cat([raw[k].double().reshape(-1) for k in HOST_TABLES]).cpu().numpy()     # the one D2H copy
    host, at = {}, 0
    for k in HOST_TABLES:
        n = raw[k].numel()
        host[k] = flat[at:at + n].reshape(tuple(raw[k].shape))
        at += n
    out = summary_from_tables(host["count"].astype(np.int64), host["q_real"], host["q_gen"], host["ws"], host["ks"],
                              host["scale"], probs, names, int(n_experts) if expert is not None else 0)
    if details:
        out.update(raw)
    return out
