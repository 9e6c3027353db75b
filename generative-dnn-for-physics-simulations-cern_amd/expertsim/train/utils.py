"""Evaluation helpers — reference: expertsim/train/utils.py:18-205.

Same names, arguments and return conventions as the reference:
  get_channel_masks(a [H,W])                        train/utils.py:18-59   (host, numpy: geometry only)
  sum_channels_parallel(data [N,H,W])               train/utils.py:62-78   -> zip of 5-tuples
  get_max_value_image_coordinates(img)              train/utils.py:81-82
  calculate_image_features(images [N,H,W])          train/utils.py:85-112  -> [5, N] float64
  calculate_joint_ws_across_experts(...)            train/utils.py:117-176
  get_predictions_from_generator_results(...)       train/utils.py:179-205
  get_predictions_from_experts_results(...)         train/utils.py:208-266   (routed, device-side dispatch)
  evaluate_router(router, y, expert_number, ...)    train/utils.py:299-310   (es_confusion_matrix metrics)

MI355X design: the generated images never leave the device.  Each generator batch is produced in
HBM (eval mode: BatchNorm running statistics, no dropout), and the fused HIP kernel
``es_channel_sums`` (csrc/eval.hip) applies expm1 and reduces every image to its five masked photon
sums in one pass, in fp64.  Only the [N,5] sums cross to the host, where the 1-D Wasserstein
distances are taken with scipy.stats.wasserstein_distance exactly as the reference does (a host
O(N log N) sort over a few thousand values per channel).  There is no CPU fallback for the sums:
``channel_sums`` raises when the HIP library or device is missing.

Device evaluation (MoEWrapper.evaluate_device, opt-in): ``wasserstein_1d_device`` /
``ws_across_experts_device`` take the same distances on the device (es_wasserstein_1d,
csrc/wasserstein.hip: scipy's arithmetic term for term) from the batch-ordered sums and the expert
vector; only the [n_calc, E + 1, 5] distances cross to the host, where ``ws_summary`` closes them as
calculate_joint_ws_across_experts does.

Shower-shape observables: ``image_features`` (es_image_features, csrc/features.hip) reduces every image
to the five values of calculate_image_features and its peak pixel in one pass on the device;
``calculate_image_features`` is the reference's API over it, MoEWrapper.simulate(features=True) fuses it
into the chunk program, and MoEWrapper.evaluate_device(features=True) takes the per-feature Wasserstein
distances with the same es_wasserstein_1d call, closed by ``ws_feature_summary``.
"""
from __future__ import annotations

import ctypes as C
from typing import List

import numpy as np
import torch

from .. import hip
from ..segments import WORK_MIN, check_segments, expert_segments


def get_channel_masks(input_array: np.ndarray):
    """Masks 1..5 of train/utils.py:18-59 for an [n, m] image: mask5 = the squares with (i+j) even;
    masks 1..4 split the (i+j)-odd squares into the bottom-left, bottom-right, top-left and
    top-right quadrants (split at n//2, m//2)."""
    n, m = np.asarray(input_array).shape
    i = np.arange(n)[:, None]
    j = np.arange(m)[None, :]
    odd = ((i + j) & 1).astype(np.float64)
    top = (i < n // 2)
    left = (j < m // 2)
    dt = np.asarray(input_array).dtype
    mask1 = (odd * (~top & left)).astype(dt)
    mask2 = (odd * (~top & ~left)).astype(dt)
    mask3 = (odd * (top & left)).astype(dt)
    mask4 = (odd * (top & ~left)).astype(dt)
    mask5 = (1.0 - odd).astype(dt)
    return mask1, mask2, mask3, mask4, mask5


def _as_device_images(data, device=None) -> torch.Tensor:
    t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
    if t.dim() == 4:
        if t.shape[1] != 1:
            raise ValueError(f"channel sums need one-channel images, got {tuple(t.shape)}")
        t = t[:, 0]
    if t.dim() != 3:
        raise ValueError(f"channel sums need images [N,H,W], got {tuple(t.shape)}")
    if t.dtype not in (torch.float32, torch.bfloat16):
        t = t.float()
    if not t.is_cuda:
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        t = t.to(dev, non_blocking=True)
    return t


def channel_sums(images, log_domain: bool = False, device=None) -> torch.Tensor:
    """[N,5] fp64 device tensor of the five masked sums of each image (HIP kernel es_channel_sums).

    images: [N,H,W] or [N,1,H,W], fp32 / bf16, any strides, device or host (host data is copied
    to the device first).  log_domain=True sums expm1(images) (the log1p-domain images of the
    dataset and generator, moe.py:646, train/utils.py:198), fused into the same pass."""
    x = _as_device_images(images, device)
    N, H, W = x.shape
    out = torch.empty(N, 5, dtype=torch.float64, device=x.device)
    if N == 0:
        return out
    view = hip.make_view((N, 1, H, W), (x.stride(0), H * W, x.stride(1), x.stride(2)))
    with torch.cuda.device(x.device):
        hip.call("es_channel_sums", C.byref(view), hip.dt_of(x), C.c_void_p(x.data_ptr()),
                 1 if log_domain else 0, hip.ptr(out), hip.stream_ptr())
    return out


def sum_channels_parallel(data):
    """Reference API (train/utils.py:62-78): zip of (ch1, ch2, ch3, ch4, ch5) per image."""
    s = channel_sums(data).cpu().numpy()
    return zip(s[:, 0], s[:, 1], s[:, 2], s[:, 3], s[:, 4])


def get_max_value_image_coordinates(img):
    """train/utils.py:81-82 (host helper used by the data pipeline)."""
    return np.unravel_index(np.argmax(img), img.shape)


FEATURE_NAMES = ("max_x", "max_y", "center_x", "center_y", "nonzero")


def image_features(images, log_domain: bool = False, device=None):
    """(feat [N,5] fp64, peak [N,2] int32) device tensors of the shower-shape observables of each image
    (HIP kernel es_image_features, csrc/features.hip; train/utils.py:81-112).

    feat columns, FEATURE_NAMES: the largest column sum, the largest row sum, the centre of the hit mask
    (pixels > 0) in x and y (w / 2, h / 2 for an image without a hit) and the number of hit pixels; peak:
    (row, col) of the first maximum in row-major order (get_max_value_image_coordinates).  images as
    channel_sums takes them; H, W <= 64; no NaN.  log_domain=True describes expm1(images), fused into
    the same pass with the float32 expm1 of channel_sums."""
    x = _as_device_images(images, device)
    N, H, W = x.shape
    feat = torch.empty(N, 5, dtype=torch.float64, device=x.device)
    peak = torch.empty(N, 2, dtype=torch.int32, device=x.device)
    if N == 0:
        return feat, peak
    view = hip.make_view((N, 1, H, W), (x.stride(0), H * W, x.stride(1), x.stride(2)))
    with torch.cuda.device(x.device):
        hip.call("es_image_features", C.byref(view), hip.dt_of(x), C.c_void_p(x.data_ptr()),
                 1 if log_domain else 0, hip.ptr(feat), hip.ptr(peak), hip.stream_ptr())
    return feat, peak


def calculate_image_features(images):
    """Reference API (train/utils.py:85-112): np.ndarray [5, N] float64 with the rows max_values_x,
    max_values_y, centers_x, centers_y, non_zero_pixels, computed by es_image_features."""
    feat, _ = image_features(images)
    return np.ascontiguousarray(feat.cpu().numpy().T)


def _generate_log_images(generator, noise: torch.Tensor, cond: torch.Tensor) -> torch.Tensor:
    """One eval-mode generator batch -> log1p-domain images [n,H,W] on the device."""
    generator.eval()                 # the reference leaves the generator in eval mode (utils.py:195)
    if hasattr(generator, "fwd"):    # expertsim HIP generator: skip the autograd bridge's copy
        img, _ = generator.fwd(noise.contiguous(), cond.contiguous(), train=False)
        t = img.torch_nchw()
    else:
        t = generator(noise, cond)
    t = t.reshape(t.shape[0], -1, t.shape[-2], t.shape[-1])
    return t[:, 0]


def _cond_on(y, device):
    y = y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))
    return y.to(device=device, dtype=torch.float32)


@torch.no_grad()
def generator_channel_sums(batch_size, num_samples, noise_dim, device, y_test, generator,
                           input_noise=None) -> torch.Tensor:
    """Device-resident core of get_predictions_from_generator_results + sum_channels_parallel:
    [num_samples, 5] fp64 sums of expm1(G(noise, cond)), batch by batch, images never copied out."""
    out = torch.empty(num_samples, 5, dtype=torch.float64, device=device)
    y = _cond_on(y_test, device)
    for start in range(0, num_samples, batch_size):
        end = min(start + batch_size, num_samples)
        if input_noise is not None:
            noise = _cond_on(input_noise[start:end], device)
        else:
            noise = torch.randn(end - start, noise_dim, device=device)
        imgs = _generate_log_images(generator, noise, y[start:end])
        out[start:end] = channel_sums(imgs, log_domain=True)
    return out


@torch.no_grad()
def get_predictions_from_generator_results(batch_size, num_samples, noise_dim, device, y_test, generator,
                                           shape_images=(56, 30), input_noise=None):
    """Reference API (train/utils.py:179-205): host arrays (expm1(images), images), float64."""
    res = np.zeros((num_samples, *shape_images))
    raw = np.zeros((num_samples, *shape_images))
    y = _cond_on(y_test, device)
    for start in range(0, num_samples, batch_size):
        end = min(start + batch_size, num_samples)
        if input_noise is not None:
            noise = _cond_on(input_noise[start:end], device)
        else:
            noise = torch.randn(end - start, noise_dim, device=device)
        r = _generate_log_images(generator, noise, y[start:end]).float().cpu().numpy()
        res[start:end] = np.expm1(r).reshape(-1, *shape_images)
        raw[start:end] = r.reshape(-1, *shape_images)
    return res, raw


@torch.no_grad()
def get_predictions_from_experts_results(num_samples, noise_dim, device, y_test, router_network, experts,
                                         shape_images=(56, 30), input_noise=None, input_expo=None,
                                         batch_size=1024):
    """Reference API (train/utils.py:208-266): the routed photon-domain prediction, host float64
    [num_samples, *shape_images] -- each condition goes to the expert the router picks (argmax of its
    Gumbel-softmax gates, as the reference's ``router_network(y)``), that expert's generator runs in
    eval mode on fresh noise, and expm1 of its image lands at the condition's position.

    Built on the pieces of MoEWrapper.simulate: es_router_dispatch (no ``np.where`` round trip), per
    expert es_gather_rows_at of [noise | cond] with the expert's device count, generator.infer on
    dynamic rows and es_sim_finish (relu, expm1, scatter).  Generalised from the reference's five
    hard-coded experts to ``len(experts)``.  The reference's fifth expert reuses expert 2's indices
    (``indx_4 = np.where(predicted_expert == 2)``, utils.py:222,228), so its expert 4 overwrites expert
    2's predictions and conditions routed to expert 4 stay zero; that is not copied: expert e gets
    the conditions routed to e.
    input_noise [N, noise_dim] / input_expo [N, E] (Exp(1) draws of the Gumbel term; ones give the
    argmax of the logits) inject the random draws (tests); default: device Philox draws."""
    from ..models.moe import _gather_rows
    from ..rng import default_rng
    y = _cond_on(y_test, device)[:num_samples].contiguous()
    E = len(experts)
    H, W = shape_images
    out = torch.empty(num_samples, H, W, dtype=torch.float32, device=y.device)
    for start in range(0, num_samples, batch_size):
        end = min(start + batch_size, num_samples)
        n = end - start
        yc = y[start:end].contiguous()
        if input_noise is not None:
            noise = _cond_on(input_noise[start:end], y.device)
        else:
            noise = torch.randn(n, noise_dim, device=y.device)
        x0 = torch.cat([noise, yc], dim=1).contiguous()
        if input_expo is not None:
            expo = _cond_on(input_expo[start:end], y.device).contiguous()
        else:
            expo = default_rng().exponential(torch.empty(n, E, dtype=torch.float32, device=y.device))
        _, _, idx, counts, _ = router_network.fwd(yc, expo, 1.0)
        perm = torch.empty(n, dtype=torch.int32, device=y.device)
        offs = torch.empty(E + 1, dtype=torch.int32, device=y.device)
        hip.call("es_router_dispatch", hip.ptr(idx), n, E, hip.ptr(perm), hip.ptr(offs), hip.stream_ptr())
        dst = out[start:end]
        for e, gen in enumerate(experts):
            live = counts[e:e + 1]
            rows = _gather_rows(x0, (perm, offs[e:e + 1]), n, x0.shape[1], live)
            h6 = gen.infer(rows, rows=live)
            v = hip.make_view(h6.dims, h6.strides, False)
            hip.call("es_sim_finish", C.byref(v), h6.ptr, hip.ptr(live), hip.ptr(perm), hip.ptr(offs[e:e + 1]), 1,
                     hip.ptr(dst), None, hip.stream_ptr())
    return out.double().cpu().numpy().reshape(num_samples, *shape_images)


@torch.no_grad()
def evaluate_router(router_network, y_test, expert_number_test, accuracy_metric=None, precision_metric=None,
                    recall_metric=None, f1_metric=None):
    """Reference API (train/utils.py:299-310): (accuracy, precision, recall, f1) of the router's arg-max over
    the conditions y_test against the class column expert_number_test, as host floats.

    The router is put in eval mode and called as ``router_network(y_test)``; a router that returns
    ``(gates, logits)`` (this project's and the reference's RouterNetwork) is read through its logits, the
    arg-max free of the Gumbel draw.  A metric callable that is given is called as the reference calls it,
    ``metric(predicted_labels, expert_number_test).cpu().item()``.  One that is None is computed from
    es_confusion_matrix (train.diagnostics.agreement_metrics): accuracy, and macro-averaged precision, recall
    and F1 over the classes that occur, with zero for an undefined term.  HIP device only."""
    from .diagnostics import agreement_metrics, confusion_matrix
    router_network.eval()
    first = next(iter(router_network.parameters()), None) if hasattr(router_network, "parameters") else None
    y = _cond_on(y_test, first.device) if first is not None else y_test
    predicted_expert = router_network(y)
    if isinstance(predicted_expert, (tuple, list)):
        predicted_expert = predicted_expert[1]
    _, predicted_labels = torch.max(predicted_expert, 1)
    target = torch.as_tensor(expert_number_test).to(predicted_labels.device)
    if target.is_floating_point():
        target = target.round().long()
    given = (accuracy_metric, precision_metric, recall_metric, f1_metric)
    own = None
    if any(m is None for m in given):
        n_pred = int(predicted_expert.shape[1])
        n_cls = max(n_pred, int(target.max()) + 1) if target.numel() else n_pred
        counts, _ = confusion_matrix(predicted_labels, target, n_cls, n_cls)
        own = agreement_metrics(counts.cpu().numpy())
    names = ("accuracy", "precision", "recall", "f1")
    return tuple(own[k] if m is None else m(predicted_labels, target).cpu().item() for k, m in zip(names, given))


# ------------------------------------------------------------------------------ device Wasserstein
_WS_WORK = {}      # device -> workspace of es_wasserstein_1d's global-memory path (grown, never shrunk)
_WS_SEG = {}       # (device, rows) -> the default one-segment bounds [[0, rows]]


def _ws_workspace(nbytes: int, device) -> torch.Tensor:
    w = _WS_WORK.get(device)
    if w is None or w.numel() < nbytes:
        w = _WS_WORK[device] = torch.empty(max(nbytes, WORK_MIN), dtype=torch.uint8, device=device)
    return w


def _ws_side(name, t, seg, idx, cap):
    hip.require_device(t)
    if t.dim() != 2 or t.dtype != torch.float64 or t.shape[0] == 0 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"wasserstein_1d_device: {name} must be a non-empty fp64 [rows, C] tensor with unit "
                         f"column stride, got {t.dtype} {tuple(t.shape)} strides {t.stride()}")
    rows = int(t.shape[0])
    if seg is None:
        key = (t.device, rows)
        seg = _WS_SEG.get(key)
        if seg is None:
            seg = _WS_SEG[key] = torch.tensor([[0, rows]], dtype=torch.int32, device=t.device)
    check_segments(t, seg, idx, f"wasserstein_1d_device: {name}_")
    return rows, seg, idx, rows if cap is None else int(cap)


def wasserstein_1d_device(u, v, u_seg=None, v_seg=None, u_idx=None, v_idx=None, u_cap=None,
                          v_cap=None) -> torch.Tensor:
    """[n_seg, C] fp64 device tensor of 1-D Wasserstein-1 distances (HIP kernel es_wasserstein_1d,
    scipy.stats.wasserstein_distance term for term): entry (s, c) compares column c of the u rows of
    segment s with column c of the v rows of segment s.

    u [rows_u, C], v [rows_v, C]: device fp64, any row stride.  u_seg / v_seg: device int32 [n_seg, 2]
    bounds (default: one segment over all rows) of positions in u_idx / v_idx (device int32 [rows],
    default: the rows themselves).  u_cap / v_cap: host upper bounds of a segment's length (default: the
    rows).  Everything is read on the device: no host synchronisation; the workspace of problems past
    hip.WS_LDS_MAX values is cached per device (one buffer: such calls on different streams of a device
    must not overlap)."""
    ur, u_seg, u_idx, u_cap = _ws_side("u", u, u_seg, u_idx, u_cap)
    vr, v_seg, v_idx, v_cap = _ws_side("v", v, v_seg, v_idx, v_cap)
    ch = int(u.shape[1])
    n_seg = u_seg.numel() // 2
    if v.device != u.device or int(v.shape[1]) != ch or v_seg.numel() // 2 != n_seg:
        raise ValueError(f"wasserstein_1d_device: u {tuple(u.shape)} with {n_seg} segments against "
                         f"v {tuple(v.shape)} with {v_seg.numel() // 2}")
    out = torch.empty(n_seg, ch, dtype=torch.float64, device=u.device)
    with torch.cuda.device(u.device):
        need = int(hip.lib().es_wasserstein_1d_workspace(n_seg, ch, u_cap, v_cap))
        work = _ws_workspace(need, u.device) if need else None
        hip.call("es_wasserstein_1d", hip.ptr(u), u.stride(0), ur, hip.ptr(u_idx), hip.ptr(u_seg),
                 hip.ptr(v), v.stride(0), vr, hip.ptr(v_idx), hip.ptr(v_seg), n_seg, ch, u_cap, v_cap,
                 hip.ptr(out), hip.ptr(work), need, hip.stream_ptr())
    return out


def ws_across_experts_device(ch_org, ch_gen, expert, n_experts) -> torch.Tensor:
    """The distances of calculate_joint_ws_across_experts on the device: ch_org [N, 5] (real sums) and
    ch_gen [R, N, 5] (R repetitions of generated sums) fp64, both in batch order, expert [N] int32.
    Returns [R, E + 1, 5]: row 0 the joint distance, row 1 + e expert e's (0 for an expert without
    rows).  One es_router_dispatch gives perm / offs; the segments are (0, N) and (offs[e], offs[e + 1])
    with perm as the row index on both sides (no gather copy), and the R repetitions are rows r * N ..
    of one [R * N, 5] v side, so all R * (E + 1) * 5 problems go out in one es_wasserstein_1d call."""
    hip.require_device(ch_org)
    dev, E = ch_org.device, int(n_experts)
    N, R = int(ch_org.shape[0]), int(ch_gen.shape[0])
    if ch_org.dim() != 2 or tuple(ch_gen.shape) != (R, N, ch_org.shape[1]) or tuple(expert.shape) != (N,):
        raise ValueError(f"ws_across_experts_device: ch_org {tuple(ch_org.shape)}, ch_gen {tuple(ch_gen.shape)}, "
                         f"expert {tuple(expert.shape)}")
    if R * N > np.iinfo(np.int32).max:
        raise ValueError(f"ws_across_experts_device: {R} x {N} rows exceed int32")
    perm, seg, _ = expert_segments(expert, E, N, dev, joint=True)
    shift = torch.arange(R, dtype=torch.int32, device=dev) * N
    u_seg = seg.repeat(R, 1)
    v_seg = (seg[None] + shift[:, None, None]).reshape(R * (E + 1), 2).contiguous()
    v_idx = (perm[None] + shift[:, None]).reshape(R * N).contiguous()
    gen = ch_gen.to(torch.float64).contiguous().view(R * N, -1)
    ws = wasserstein_1d_device(ch_org.to(torch.float64), gen, u_seg, v_seg, perm, v_idx, u_cap=N, v_cap=N)
    return ws.view(R, E + 1, -1)


def ws_summary(ws):
    """Closing arithmetic of calculate_joint_ws_across_experts (train/utils.py:117-176) on the host copy
    of ws_across_experts_device's [R, E + 1, 5] result (a pure numpy function): channel means per
    repetition, then mean / std over the repetitions.  Returns (ws_mean, ws_std, ws_mean_exp [E],
    ws_std_exp [E])."""
    ws = np.asarray(ws, dtype=np.float64)
    if ws.ndim != 3 or ws.shape[1] < 2:
        raise ValueError(f"ws_summary: expected [R, E + 1, C], got {ws.shape}")
    ws_runs = ws[:, 0].mean(axis=1)
    ws_exp_runs = ws[:, 1:].mean(axis=2)
    return ws_runs.mean(), ws_runs.std(), ws_exp_runs.mean(axis=0), ws_exp_runs.std(axis=0)


def ws_feature_summary(ws):
    """Closing arithmetic of the shower-shape metrics on the host copy of ws_across_experts_device's
    [R, E + 1, 5] result over the FEATURE_NAMES columns (a pure numpy function): per feature the mean and
    std over the repetitions of the joint row, and per expert the mean over the repetitions.  Unlike
    ws_summary nothing is averaged across the columns: a sum of photons, a pixel coordinate and a pixel
    count differ in scale by orders of magnitude.  Returns (ws_feat [C], ws_feat_std [C],
    ws_feat_exp [E, C])."""
    ws = np.asarray(ws, dtype=np.float64)
    if ws.ndim != 3 or ws.shape[1] < 2:
        raise ValueError(f"ws_feature_summary: expected [R, E + 1, C], got {ws.shape}")
    return ws[:, 0].mean(axis=0), ws[:, 0].std(axis=0), ws[:, 1:].mean(axis=0)


def calculate_joint_ws_across_experts(n_calc, x_tests: List, y_tests: List, generators: List, ch_org,
                                      ch_org_expert, noise_dim, device, batch_size=64, n_experts=3,
                                      shape_images=(56, 30)):
    """Reference API and arithmetic (train/utils.py:117-176): for each of n_calc repetitions,
    generate every expert's samples, take the 5-channel WS distance of the joint and of each
    expert's distribution against the real sums, average over channels, then mean/std over the
    repetitions.  Returns (ws_mean, ws_std, ws_mean_exp [E], ws_std_exp [E])."""
    from scipy.stats import wasserstein_distance
    if len(x_tests) != len(y_tests) or len(x_tests) != len(generators):
        raise ValueError("Length of data is not the same")
    ch_org = np.asarray(ch_org)
    ws = np.zeros((n_calc, 5))
    ws_exp = np.zeros((n_calc, n_experts, 5))
    for j in range(n_calc):
        per = []
        for g_idx, gen in enumerate(generators):
            num = int(np.asarray(x_tests[g_idx]).shape[0]) if not isinstance(x_tests[g_idx], torch.Tensor) \
                else int(x_tests[g_idx].shape[0])
            if num == 0:
                per.append(None)
                continue
            per.append(generator_channel_sums(batch_size, num, noise_dim, device, y_tests[g_idx], gen))
        live = [p for p in per if p is not None]
        ch_gen_all = torch.cat(live).cpu().numpy() if live else np.zeros((0, 5))
        ch_gen_exp = [p.cpu().numpy() if p is not None else np.array([]) for p in per]
        for i in range(5):
            ws[j][i] = wasserstein_distance(ch_org[:, i], ch_gen_all[:, i])
            for e in range(len(generators)):
                org_e = np.asarray(ch_org_expert[e])
                if ch_gen_exp[e].shape[0] == 0 or org_e.shape[0] == 0:
                    continue
                ws_exp[j][e][i] = wasserstein_distance(org_e[:, i], ch_gen_exp[e][:, i])
    ws_runs = ws.mean(axis=1)
    ws_exp_runs = ws_exp.mean(axis=2)
    return ws_runs.mean(), ws_runs.std(), ws_exp_runs.mean(axis=0), ws_exp_runs.std(axis=0)
