"""What the wrappers of the analysis kernels share (train/fidelity.py, train/diagnostics.py, train/embedding.py,
train/utils.py's Wasserstein entries, utils/clustering.py, utils/data_preparation.py): how a matrix, a workspace
and the segments of an expert vector are handed to a kernel.  csrc/segment.h is the device side of the same rule:
segment s covers the rows idx[seg[s, 0] .. seg[s, 1]) (idx None: the rows themselves), the bounds clamped to the
rows and the indices to [0, rows).
"""
from __future__ import annotations

import torch

from . import hip

WORK_MIN = 16      # bytes: no entry is handed an empty or a NULL workspace


def ld(x) -> int:
    """Row stride of a [rows, cols] tensor in elements (a single row: at least cols)."""
    return int(x.stride(0)) if x.shape[0] > 1 else max(int(x.stride(0)), int(x.shape[1]))


def is_f64(x) -> int:
    """The x_f64 argument of the entries that take fp32 or fp64."""
    return 1 if x.dtype == torch.float64 else 0


def work_buffer(nbytes, device) -> torch.Tensor:
    """A fresh uint8 workspace of at least nbytes (and at least WORK_MIN) bytes."""
    return torch.empty(max(int(nbytes), WORK_MIN), dtype=torch.uint8, device=device)


def unit_stride_matrix(t) -> torch.Tensor:
    """t [rows, cols] as the kernels read it: unit column stride and a row stride of at least cols (a copy only
    where t is not laid out like that)."""
    if t.shape[0] > 1 and (t.stride(0) < t.shape[1] or (t.shape[1] > 1 and t.stride(1) != 1)):
        t = t.contiguous()
    return t


def check_segments(x, seg, idx, what="") -> int:
    """n_seg of seg [n_seg, 2] after checking that seg and idx (or None) are what a kernel may read for the rows of
    x: contiguous int32 tensors on x's device, idx with one entry per row.  `what` prefixes the names in the
    error."""
    if seg.dtype != torch.int32 or seg.device != x.device or seg.numel() % 2 or not seg.is_contiguous():
        raise ValueError(f"{what}seg must be a contiguous device int32 [n_seg, 2] tensor")
    if idx is not None and (idx.dtype != torch.int32 or idx.device != x.device or not idx.is_contiguous()
                            or idx.numel() != x.shape[0]):
        raise ValueError(f"{what}idx must be a contiguous device int32 [{x.shape[0]}] tensor")
    return seg.numel() // 2


def expert_segments(expert, n_experts: int, n_rows: int, device, joint: bool = False):
    """(perm int32 [N] or None, seg int32 [E (+ 1), 2], offs int32 [E + 1]) on the device from one
    es_router_dispatch: expert e's samples are the rows perm[offs[e] .. offs[e + 1]), in batch order, and its
    segment is (offs[e], offs[e + 1]).  joint=True puts the segment (0, N) of all rows in front, so expert e's is
    segment 1 + e.  expert None (n_experts must be 1): one segment over all rows and no perm.  N == 0 launches
    nothing."""
    E, N, j = int(n_experts), int(n_rows), 1 if joint else 0
    offs = torch.zeros(E + 1, dtype=torch.int32, device=device)
    if expert is None:
        if E != 1:
            raise ValueError(f"n_experts = {E} needs an expert vector")
        perm = None
        offs[1] = N
    else:
        if tuple(expert.shape) != (N,):
            raise ValueError(f"expert must be [{N}], got {tuple(expert.shape)}")
        expert = expert.to(device=device, dtype=torch.int32).contiguous()
        perm = torch.empty(N, dtype=torch.int32, device=device)
        if N > 0:
            with torch.cuda.device(device):
                hip.call("es_router_dispatch", hip.ptr(expert), N, E, hip.ptr(perm), hip.ptr(offs), hip.stream_ptr())
    seg = torch.empty(E + j, 2, dtype=torch.int32, device=device)
    if joint:
        seg[0, 0] = 0
        seg[0, 1] = N
    seg[j:, 0] = offs[:-1]
    seg[j:, 1] = offs[1:]
    return perm, seg, offs
