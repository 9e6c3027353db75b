"""The sliced Wasserstein distance (SWD) between two sets of whole calorimeter images on the device.

Every other distribution-level number of the evaluation looks at a handful of observables (the channel sums, the
shower shapes, their joint distribution in train/distances.py) or at ranks in a neighbour graph
(train/fidelity.py); a generator can match all of them and still put the shower in the wrong pixels.  The SWD
compares the image distributions in pixel space without a trained feature network: it is the mean, over random unit
directions theta, of the 1-D Wasserstein-1 distance between the projections <x, theta> of the real and of the
generated images; the largest of those distances is the max-sliced distance.

HIP kernels (csrc/sliced.hip, defined in include/expertsim_hip.h):

* ``es_sliced_directions``  n_proj unit directions of d pixels from es_randn's Philox stream, fp64;
* ``es_sliced_project``     the [N, D] x [D, P] projection in fp64 on the fp64 matrix pipe, one pinned summation
                            order per output element;

and, unchanged, ``es_wasserstein_1d`` (train.utils.wasserstein_1d_device) over the projected columns, with
``es_router_dispatch``'s joint-plus-per-expert segments, and ``es_segment_moments`` for the mean and the variance
over the directions.

The value depends on the pixel domain of the images (log1p or photons) and on n_proj (and, through the directions,
on the seed): compare runs at equal settings only.

There is no CPU fallback: without a HIP device every device function raises hip.HipError.  The host half
(`summary`) is pure numpy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import hip
from ..segments import expert_segments, ld, unit_stride_matrix

KEYS = ("swd", "swd_err", "swd_max")
# Philox stream id of the directions (MoEWrapper.SIM_NOISE_STREAM / SIM_GUMBEL_STREAM are 0x51D00001 / 2)
SLICED_STREAM = 0x51D00003
MAX_D = 4096            # ES_SLICED_MAX_D
MAX_PROJ = 1024         # ES_SLICED_MAX_PROJ
MAX_PROBLEMS = 65535    # es_wasserstein_1d: n_seg * channels
MAX_SEGMENTS = 32       # es_segment_moments: cols of the transposed [P, E + 1] table

_NO_DEVICE = "the sliced Wasserstein distance needs a HIP device (no CPU fallback)"


def check_problems(n_seg: int, n_proj: int):
    """ValueError unless one es_wasserstein_1d call takes the n_seg x n_proj problems and es_segment_moments the
    n_seg columns."""
    n_seg, n_proj = int(n_seg), int(n_proj)
    if n_seg * n_proj > MAX_PROBLEMS:
        raise ValueError(f"(E + 1) * n_proj = {n_seg} * {n_proj} = {n_seg * n_proj} exceeds the {MAX_PROBLEMS} problems "
                         f"of one es_wasserstein_1d call: lower n_proj")
    if not 1 <= n_proj <= MAX_PROJ:
        raise ValueError(f"n_proj = {n_proj} outside 1 .. {MAX_PROJ}")
    if n_seg > MAX_SEGMENTS:
        raise ValueError(f"E + 1 = {n_seg} segments exceed the {MAX_SEGMENTS} columns of es_segment_moments")


def _images(x) -> torch.Tensor:
    """[N, H, W] fp32 / bf16 on the device, strides as given."""
    if not torch.cuda.is_available():
        raise hip.HipError(_NO_DEVICE)
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    hip.require_device(t)
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise ValueError(f"one-channel images expected, got {tuple(t.shape)}")
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"images must be [N,H,W] or [N,1,H,W], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    return t


def _theta(theta) -> torch.Tensor:
    if not torch.cuda.is_available():
        raise hip.HipError(_NO_DEVICE)
    t = theta if isinstance(theta, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(theta))
    hip.require_device(t)
    if t.dim() != 2 or t.dtype != torch.float64 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"directions must be a fp64 [P, D] tensor, got {t.dtype} {tuple(t.shape)}")
    return unit_stride_matrix(t)


# ------------------------------------------------------------------------------------------ thin wrappers
def directions(n_proj, d, seed=0, device=None) -> torch.Tensor:
    """es_sliced_directions: [n_proj, d] fp64 unit rows on the device.  Row p is draws p * D2 .. p * D2 + d - 1 (D2 = d
    rounded up to even) of es_randn(seed, SLICED_STREAM), normalised in fp64; a function of (n_proj, d, seed) alone."""
    if not torch.cuda.is_available():
        raise hip.HipError(_NO_DEVICE)
    P, d = int(n_proj), int(d)
    if not 1 <= P <= MAX_PROJ or not 1 <= d <= MAX_D:
        raise ValueError(f"directions: n_proj = {P} outside 1 .. {MAX_PROJ} or d = {d} outside 1 .. {MAX_D}")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        theta = torch.empty(P, d, dtype=torch.float64, device=dev)
        hip.call("es_sliced_directions", hip.ptr(theta), d, P, d, int(seed) & 0xFFFFFFFFFFFFFFFF, SLICED_STREAM,
                 hip.stream_ptr())
    return theta


_new_directions = directions       # sliced_device / sliced take a parameter of that name


def project(images, theta, out=None) -> torch.Tensor:
    """es_sliced_project: [N, P] fp64 on the device, entry (b, p) = sum_d images[b].flatten()[d] * theta[p, d].
    images [N,H,W] or [N,1,H,W], fp32 or bf16, any strides; theta [P, H * W] fp64.  out: a fp64 tensor of at least
    N rows and P columns with unit column stride to write into (its first N rows and P columns are returned)."""
    x, theta = _images(images), _theta(theta)
    N, H, W = (int(s) for s in x.shape)
    P = int(theta.shape[0])
    if theta.device != x.device or int(theta.shape[1]) != H * W:
        raise ValueError(f"directions {tuple(theta.shape)} on {theta.device} for images {tuple(x.shape)} on {x.device}")
    if out is None:
        out = torch.empty(N, P, dtype=torch.float64, device=x.device)
    elif (out.dtype != torch.float64 or out.device != x.device or out.dim() != 2 or out.shape[0] < N
          or out.shape[1] < P or (out.shape[1] > 1 and out.stride(1) != 1) or (N > 1 and out.stride(0) < P)):
        raise ValueError(f"out must be a device fp64 [>= {N}, >= {P}] tensor with unit column stride")
    if N > 0:
        view = hip.make_view((N, 1, H, W), (x.stride(0), H * W, x.stride(1), x.stride(2)))
        with torch.cuda.device(x.device):
            hip.call("es_sliced_project", C.byref(view), hip.dt_of(x), C.c_void_p(x.data_ptr()), hip.ptr(theta),
                     ld(theta), P, hip.ptr(out), ld(out), hip.stream_ptr())
    return out[:N, :P]


# ------------------------------------------------------------------------------------------ host half
def summary(moments, maxima, counts, n_proj, per_expert=True) -> dict:
    """The closing arithmetic on the host copy of sliced_device's small tensors (pure numpy): moments [2, S] (mean
    and np.var(ddof=1) of a segment's distances over the directions), maxima [S], counts [S, 2] (real, generated rows
    of a segment).  Segment 0 gives "swd" (the mean), "swd_err" (sqrt(var / n_proj), the standard error over the
    directions; NaN for n_proj < 2) and "swd_max" (the max-sliced distance), segment 1 + e the same with `_<e>`
    appended.  A segment that is empty on either side gives NaN for all three (es_wasserstein_1d writes 0 there,
    which is no distance)."""
    mom = np.asarray(moments, dtype=np.float64).reshape(2, -1)
    mx = np.asarray(maxima, dtype=np.float64).reshape(-1)
    cnt = np.asarray(counts).reshape(-1, 2)
    S, P = mx.shape[0], int(n_proj)
    live = (cnt[:, 0] > 0) & (cnt[:, 1] > 0)
    with np.errstate(invalid="ignore"):
        err = np.sqrt(mom[1] / P) if P >= 2 else np.full(S, np.nan)
    vals = {"swd": np.where(live, mom[0], np.nan), "swd_err": np.where(live, err, np.nan),
            "swd_max": np.where(live, mx, np.nan)}
    out = {name: float(vals[name][0]) for name in KEYS}
    if per_expert:
        for e in range(S - 1):
            for name in KEYS:
                out[f"{name}_{e}"] = float(vals[name][1 + e])
    return out


# ------------------------------------------------------------------------------------------ the distance
def sliced_device(real, fake, expert=None, n_experts=1, n_proj=256, seed=0, directions=None) -> dict:
    """The device half of `sliced`, no host synchronisation: {"w" fp64 [S, P] (the 1-D distance of every segment
    along every direction), "moments" fp64 [2, S] (mean and variance over the directions), "maxima" fp64 [S],
    "counts" int32 [S, 2] (real, generated rows), "theta" [P, D], "proj_real" [N_r, P], "proj_fake" [N_f, P], "seg",
    "perm"}.  Without an expert vector S = 1 and the two sides may differ in length; with one (real, fake and expert
    aligned, N rows each) S = E + 1: the joint segment and one per expert."""
    real, fake = _images(real), _images(fake)
    if real.device != fake.device or tuple(real.shape[1:]) != tuple(fake.shape[1:]):
        raise ValueError(f"real {tuple(real.shape)} on {real.device} against generated {tuple(fake.shape)} on "
                         f"{fake.device}")
    Nr, Nf, D, dev = int(real.shape[0]), int(fake.shape[0]), int(real.shape[1] * real.shape[2]), real.device
    if Nr < 1 or Nf < 1:
        raise ValueError(f"{Nr} real and {Nf} generated images: both sides need at least one")
    E = int(n_experts)
    P = int(n_proj) if directions is None else int(directions.shape[0])
    check_problems(E + 1 if expert is not None else 1, P)                 # before any launch
    with torch.cuda.device(dev):
        theta = _new_directions(P, D, seed, dev) if directions is None else _theta(directions)
        proj_r, proj_f = project(real, theta), project(fake, theta)
        from .utils import wasserstein_1d_device
        if expert is None:
            if E != 1:
                raise ValueError(f"n_experts = {E} needs an expert vector")
            perm = None
            r_seg = torch.tensor([[0, Nr]], dtype=torch.int32, device=dev)
            f_seg = r_seg if Nf == Nr else torch.tensor([[0, Nf]], dtype=torch.int32, device=dev)
        else:
            if Nf != Nr or tuple(expert.shape) != (Nr,):
                raise ValueError(f"with an expert vector real, fake and expert are aligned: {Nr}, {Nf}, "
                                 f"{tuple(expert.shape)}")
            perm, r_seg, _ = expert_segments(expert, E, Nr, dev, joint=True)
            f_seg = r_seg
        w = wasserstein_1d_device(proj_r, proj_f, r_seg, f_seg, perm, perm, u_cap=Nr, v_cap=Nf)     # [S, P]
        from .distances import segment_moments
        _, mean, cov = segment_moments(w.t().contiguous())                 # one segment: the P directions
        moments = torch.stack([mean[0], torch.diagonal(cov[0])])
        maxima = torch.amax(w, dim=1)
        counts = torch.stack([r_seg[:, 1] - r_seg[:, 0], f_seg[:, 1] - f_seg[:, 0]], dim=1)
    return {"w": w, "moments": moments, "maxima": maxima, "counts": counts, "theta": theta, "proj_real": proj_r,
            "proj_fake": proj_f, "seg": r_seg, "perm": perm}


def sliced(real, fake, expert=None, n_experts=1, n_proj=256, seed=0, directions=None, details=False) -> dict:
    """The sliced Wasserstein distance of the generated images `fake` against the real images `real` ([N,H,W] or
    [N,1,H,W] on the device, fp32 or bf16, any strides, at most 4096 pixels).

    Both sides are projected once onto n_proj unit directions (`directions`(n_proj, H * W, seed), or the
    [P, H * W] fp64 tensor passed as directions); one es_wasserstein_1d call gives the 1-D distance of every
    segment along every direction, one es_segment_moments call their mean and variance over the directions, and
    ONE small device-to-host copy brings the result: "swd" (the mean), "swd_err" (its standard error over the
    directions, sqrt(var / n_proj)) and "swd_max" (the max-sliced distance).  expert [N] (then real and fake are
    aligned row by row): `<name>_<e>` per expert next to the joint values, (E + 1) * n_proj <= 65535 and
    E + 1 <= 32.  A segment that is empty on either side gives NaN.  details=True adds sliced_device's tensors
    ("w", "theta", "proj_real", "proj_fake", ...).

    The value depends on the pixel domain of the images (log1p or photons: a distance in the units of a pixel) and
    on n_proj, and through the directions on the seed: compare runs at equal settings only.  swd_err measures the
    spread over the directions, not the sampling error of the two image sets."""
    raw = sliced_device(real, fake, expert, n_experts, n_proj, seed, directions)
    S, P = (int(s) for s in raw["w"].shape)
    host = torch.cat([raw["moments"].reshape(-1), raw["maxima"], raw["counts"].double().reshape(-1)]).cpu().numpy()
    out = summary(host[:2 * S].reshape(2, S), host[2 * S:3 * S], host[3 * S:].reshape(S, 2), P,
                  per_expert=expert is not None)                           # after the one D2H copy
    if details:
        out.update(raw)
    return out
