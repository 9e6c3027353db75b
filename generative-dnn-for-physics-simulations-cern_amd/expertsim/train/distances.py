"""Distances between the joint distributions of the shower observables on the device: a Frechet distance between
fitted Gaussians and a polynomial-kernel MMD, after Kansal et al. 2023 ("Evaluating generative models in high
energy physics", the `fpd` and `kpd` of the jetnet package).

Every other distribution-level number of the evaluation is a one-dimensional marginal (five channel-sum and five
shower-shape Wasserstein distances) or a rank statistic of a neighbour graph (train/fidelity.py); none sees the
correlations between the observables, which is where a mixture of experts that fits every marginal can still be
wrong.  HIP kernels (csrc/distance.hip, defined in include/expertsim_hip.h):

* ``es_segment_moments``  count, mean and np.cov-style covariance of every segment, fp64;
* ``es_frechet``          |dmu|^2 + tr A + tr B - 2 tr (A B)^1/2 per pair of moments, two fp64 Jacobi
                          eigendecompositions per problem;
* ``es_mmd_poly``         the three all-pairs sums of k(u, v) = (gamma <u, v> + coef0)^degree per segment, fp64,
                          matrix-free, the diagonal excluded by index.

The statistics are defined here and claim descent from the paper, not equality with jetnet: `fpd` extrapolates
the Frechet distance of growing PREFIXES of the rows to infinite sample size, `kpd` is the median unbiased MMD^2
over CONSECUTIVE blocks; jetnet draws random batches for both.  Segments are es_router_dispatch's (joint + per
expert) as in train/fidelity.py, but because prefixes and blocks depend on the order of the rows the joint segment
keeps the order given and the experts' rows are gathered behind it (a copy of the small observable table).

There is no CPU fallback: without a HIP device every device function raises hip.HipError.  The host halves
(`fpd_from_table`, `kpd_from_table`, `summary_dict`) are pure numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ..segments import check_segments, expert_segments, is_f64, ld, unit_stride_matrix, work_buffer

CHANNEL_NAMES = ("ch1", "ch2", "ch3", "ch4", "ch5")
FPD_KEYS = ("fpd", "fpd_err", "fd_full")
KPD_KEYS = ("kpd", "kpd_err", "mmd_full")
KEYS = FPD_KEYS + KPD_KEYS


def _observable_names():
    from .utils import FEATURE_NAMES
    return tuple(f"sum_{c}" for c in CHANNEL_NAMES) + tuple(FEATURE_NAMES)


OBSERVABLE_NAMES = _observable_names()


def _table(x, f32=False) -> torch.Tensor:
    """[rows, cols] on the device with unit column stride; fp64 is kept unless f32, everything else becomes fp32."""
    if not torch.cuda.is_available():
        raise hip.HipError("the distribution distances need a HIP device (no CPU fallback)")
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    hip.require_device(t)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"x must be [rows, cols] with at least one of each, got {tuple(t.shape)}")
    if f32 or t.dtype != torch.float64:
        t = t if t.dtype == torch.float32 else t.float()
    return unit_stride_matrix(t)


def _segments(x, idx, seg):
    """(idx, seg [n_seg, 2], n_seg) as device int32 tensors; the default is one segment of all rows."""
    dev, rows = x.device, int(x.shape[0])
    if seg is None:
        seg = torch.tensor([[0, rows]], dtype=torch.int32, device=dev)
    seg = torch.as_tensor(seg).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
    if idx is not None:
        idx = torch.as_tensor(idx).to(device=dev, dtype=torch.int32).contiguous()
        if idx.dim() != 1 or idx.shape[0] < rows:
            raise ValueError(f"idx must have the {rows} entries of x's rows, got {tuple(idx.shape)}")
        idx = idx[:rows]
    return idx, seg, check_segments(x, seg, idx)


# ------------------------------------------------------------------------------------------ thin wrappers
def segment_moments(x, idx=None, seg=None, out=None):
    """es_segment_moments: (count int32 [n_seg], mean fp64 [n_seg, cols], cov fp64 [n_seg, cols, cols]) on the
    device for x [rows, cols <= 32], fp32 or fp64.  cov is np.cov(rowvar=False); a segment of fewer than two rows
    has NaN in cov, an empty one in mean too.  out: the three tensors to write into (their first n_seg entries)."""
    x = _table(x)
    idx, seg, n_seg = _segments(x, idx, seg)
    rows, cols = int(x.shape[0]), int(x.shape[1])
    with torch.cuda.device(x.device):
        if out is None:
            out = (torch.empty(n_seg, dtype=torch.int32, device=x.device),
                   torch.empty(n_seg, cols, dtype=torch.float64, device=x.device),
                   torch.empty(n_seg, cols, cols, dtype=torch.float64, device=x.device))
        count, mean, cov = out
        need = hip.segment_moments_workspace(n_seg, cols)
        work = work_buffer(need, x.device)
        hip.call("es_segment_moments", hip.ptr(x), is_f64(x), ld(x), rows, cols, hip.ptr(idx), hip.ptr(seg), n_seg,
                 hip.ptr(count), hip.ptr(mean), hip.ptr(cov), hip.ptr(work), int(work.numel()) if need else 0,
                 hip.stream_ptr())
    return count, mean, cov


def frechet(mean_a, cov_a, mean_b, cov_b, out=None) -> torch.Tensor:
    """es_frechet: fp64 [n, 4] = (d2, |dmu|^2, tr A + tr B, tr (A B)^1/2) on the device for the n problems
    (mean_a [n, cols], cov_a [n, cols, cols], mean_b, cov_b) as segment_moments returns them; a problem with a NaN
    in its moments gives four NaN."""
    if not torch.cuda.is_available():
        raise hip.HipError("the distribution distances need a HIP device (no CPU fallback)")
    ts = []
    for t in (mean_a, cov_a, mean_b, cov_b):
        t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
        hip.require_device(t)
        ts.append(t.to(torch.float64).contiguous())
    mean_a, cov_a, mean_b, cov_b = ts
    if mean_a.dim() == 1:
        mean_a, cov_a, mean_b, cov_b = mean_a[None], cov_a[None], mean_b[None], cov_b[None]
    n, cols = int(mean_a.shape[0]), int(mean_a.shape[1])
    if tuple(mean_b.shape) != (n, cols) or tuple(cov_a.shape) != (n, cols, cols) or tuple(cov_b.shape) != (n, cols, cols):
        raise ValueError(f"moments of {n} problems of {cols} columns expected, got {tuple(mean_a.shape)}, "
                         f"{tuple(cov_a.shape)}, {tuple(mean_b.shape)}, {tuple(cov_b.shape)}")
    with torch.cuda.device(mean_a.device):
        if out is None:
            out = torch.empty(n, 4, dtype=torch.float64, device=mean_a.device)
        hip.call("es_frechet", hip.ptr(mean_a), hip.ptr(cov_a), hip.ptr(mean_b), hip.ptr(cov_b), n, cols, hip.ptr(out),
                 hip.stream_ptr())
    return out


def mmd_poly_sums(real, fake, degree=4, gamma=None, coef0=1.0, r_idx=None, r_seg=None, r_cap=None, f_idx=None,
                  f_seg=None, f_cap=None, out=None):
    """es_mmd_poly: (sums fp64 [n_seg, 4] = (S_xx, S_yy, S_xy, 0), counts int32 [n_seg, 2] = (m, n)) on the device
    for the polynomial kernel k(u, v) = (gamma <u, v> + coef0)^degree over real / fake [rows, cols <= 64] (cast to
    fp32, the kernel's input type; the arithmetic is fp64).  gamma=None means 1 / cols.  S_xx and S_yy leave the
    diagonal out.  out: the two tensors to write into (their first n_seg entries)."""
    real, fake = _table(real, f32=True), _table(fake, f32=True)
    if real.device != fake.device:
        raise ValueError("real and fake are on different devices")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real has {real.shape[1]} columns, fake {fake.shape[1]}")
    r_idx, r_seg, n_seg = _segments(real, r_idx, r_seg)
    f_idx, f_seg, f_n_seg = _segments(fake, f_idx, f_seg)
    if n_seg != f_n_seg:
        raise ValueError(f"{n_seg} real segments, {f_n_seg} generated")
    cols, dev = int(real.shape[1]), real.device
    r_cap = int(real.shape[0]) if r_cap is None else int(r_cap)
    f_cap = int(fake.shape[0]) if f_cap is None else int(f_cap)
    gamma = 1.0 / cols if gamma is None else float(gamma)
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(n_seg, 4, dtype=torch.float64, device=dev),
                   torch.empty(n_seg, 2, dtype=torch.int32, device=dev))
        sums, counts = out
        need = hip.mmd_poly_workspace(n_seg, r_cap, f_cap)
        work = work_buffer(need, dev)
        hip.call("es_mmd_poly", hip.ptr(real), ld(real), int(real.shape[0]), hip.ptr(r_idx), hip.ptr(r_seg), r_cap,
                 hip.ptr(fake), ld(fake), int(fake.shape[0]), hip.ptr(f_idx), hip.ptr(f_seg), f_cap, cols, n_seg,
                 int(degree), gamma, float(coef0), hip.ptr(sums), hip.ptr(counts), hip.ptr(work),
                 int(work.numel()) if need else 0, hip.stream_ptr())
    return sums, counts


# ------------------------------------------------------------------------------------------ observables
def observables(images, log_domain=True, sums=None, features=None) -> torch.Tensor:
    """[N, 10] fp64 on the device, OBSERVABLE_NAMES: train.utils.channel_sums (five masked photon sums) next to
    train.utils.image_features' five columns (largest column / row sum, centre of the hit mask, hit count).
    sums / features: the [N, 5] tensors where a caller has them already (images may then be None)."""
    from .utils import channel_sums, image_features
    if sums is None:
        sums = channel_sums(images, log_domain=log_domain)
    if features is None:
        features, _ = image_features(images, log_domain=log_domain)
    return torch.cat([sums, features], dim=1)


def normalise(real, fake):
    """(real / scale, fake / scale, scale): both sides divided by the real side's per-column max |.| (1 where that
    is 0), Kansal et al.'s rule.  Plain torch on the device; fp64 in, fp64 out."""
    scale = real.abs().amax(dim=0)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))
    return real / scale, fake / scale, scale


# ------------------------------------------------------------------------------------------ host halves
def prefix_lengths(L, points):
    """n_j = floor(L (points + j) / (2 points - 1)), j = 0 .. points - 1: from about L / 2 up to L."""
    j = np.arange(int(points), dtype=np.int64)
    return (int(L) * (int(points) + j)) // (2 * int(points) - 1)


def fpd_from_table(table, cols) -> np.ndarray:
    """[S, 3] float64 (fpd, fpd_err, fd_full) from table [S, points, 3] = (FD_j, n_j real, n_j generated), the host
    copy of `fpd`'s device result.  Per segment the ordinary least-squares fit FD_j = a + c / n_j in float64:
    fpd = a, fpd_err = the standard error of a from the residuals (points - 2 degrees of freedom), fd_full = the
    last FD_j.  NaN where n_0 <= cols on either side (a rank-deficient covariance) or the n_j are all equal."""
    t = np.asarray(table, dtype=np.float64)
    S, P = t.shape[0], t.shape[1]
    out = np.full((S, 3), np.nan, dtype=np.float64)
    for s in range(S):
        fd, n_r, n_f = t[s, :, 0], t[s, :, 1], t[s, :, 2]
        if not (n_r[0] > cols and n_f[0] > cols) or P < 3:
            continue
        x = 1.0 / n_r
        xm = x.mean()
        sxx = float(((x - xm) ** 2).sum())
        if not sxx > 0.0:
            continue
        c = float(((x - xm) * (fd - fd.mean())).sum()) / sxx
        a = float(fd.mean() - c * xm)
        rss = float(((fd - (a + c * x)) ** 2).sum())
        err = np.sqrt(rss / (P - 2) * (1.0 / P + xm * xm / sxx))
        out[s] = (a, err, fd[-1])
    return out


def mmd2(sums, counts) -> np.ndarray:
    """The unbiased MMD^2 = S_xx / (m (m - 1)) + S_yy / (n (n - 1)) - 2 S_xy / (m n) of each row of sums [.., >= 3]
    with counts [.., 2] = (m, n), float64; NaN where m < 2 or n < 2."""
    s = np.asarray(sums, dtype=np.float64)
    m = np.asarray(counts)[..., 0].astype(np.float64)
    n = np.asarray(counts)[..., 1].astype(np.float64)
    ok = (m >= 2) & (n >= 2)
    ms, ns = np.where(ok, m, 2.0), np.where(ok, n, 2.0)
    v = s[..., 0] / (ms * (ms - 1.0)) + s[..., 1] / (ns * (ns - 1.0)) - 2.0 * s[..., 2] / (ms * ns)
    return np.where(ok, v, np.nan)


def kpd_from_table(table) -> np.ndarray:
    """[S, 3] float64 (kpd, kpd_err, mmd_full) from table [S, blocks + 1, 5] = (S_xx, S_yy, S_xy, m, n), the host
    copy of `kpd`'s device result, the whole segment last.  kpd = np.median of the blocks' MMD^2, kpd_err = half
    their interquartile range (np.percentile 75 and 25), mmd_full = the whole segment's MMD^2.  NaN where a block
    has fewer than two rows on either side."""
    t = np.asarray(table, dtype=np.float64)
    S = t.shape[0]
    out = np.full((S, 3), np.nan, dtype=np.float64)
    v = mmd2(t[..., :3], t[..., 3:5])
    for s in range(S):
        blocks = v[s, :-1]
        if blocks.size == 0 or not np.isfinite(blocks).all():
            continue
        q75, q25 = np.percentile(blocks, [75, 25])
        out[s] = (np.median(blocks), 0.5 * (q75 - q25), v[s, -1])
    return out


def summary_dict(fpd_values=None, kpd_values=None, per_expert=True) -> dict:
    """{"fpd", "fpd_err", "fd_full", "kpd", "kpd_err", "mmd_full"} from segment 0 of fpd_from_table's /
    kpd_from_table's result and `<name>_<e>` from segment 1 + e (the shape of fidelity.metrics_dict); either table
    may be None."""
    out = {}
    for names, vals in ((FPD_KEYS, fpd_values), (KPD_KEYS, kpd_values)):
        if vals is None:
            continue
        vals = np.asarray(vals, dtype=np.float64)
        for i, name in enumerate(names):
            out[name] = float(vals[0, i])
        if per_expert:
            for e in range(vals.shape[0] - 1):
                for i, name in enumerate(names):
                    out[f"{name}_{e}"] = float(vals[1 + e, i])
    return out


# ------------------------------------------------------------------------------------------ fpd / kpd
def _aligned(real, fake, expert, n_experts):
    """(real, fake, r_seg [S, 2], f_seg [S, 2], perm) for the prefixes and blocks, which depend on the ORDER of a
    segment's rows.  Without an expert vector: the tables as given and one segment over each.  With one (real and
    fake aligned, N rows each): one expert_segments(joint=True) call; the joint segment keeps the rows in the order
    given and every expert's rows follow behind them in batch order, gathered by the dispatch permutation (a copy
    of the [N, cols] tables, plain torch: in the permutation's own order the joint segment would be sorted by
    expert, exactly the ordering that biases a prefix), so expert e's segment is (N + offs[e], N + offs[e + 1])."""
    N, dev = int(real.shape[0]), real.device
    if expert is None:
        return (real, fake, torch.tensor([[0, N]], dtype=torch.int32, device=dev),
                torch.tensor([[0, int(fake.shape[0])]], dtype=torch.int32, device=dev), None)
    if fake.shape[0] != N or tuple(expert.shape) != (N,):
        raise ValueError(f"with an expert vector real, fake and expert are aligned: {N}, {fake.shape[0]}, "
                         f"{tuple(expert.shape)}")
    perm, seg, _ = expert_segments(expert, n_experts, N, dev, joint=True)
    seg = seg.clone()
    seg[1:] += N
    order = perm.long()
    return (torch.cat([real, real.index_select(0, order)]), torch.cat([fake, fake.index_select(0, order)]), seg, seg,
            perm)


def fpd_device(real, fake, expert=None, n_experts=1, points=10):
    """The device half of `fpd`: {"table" fp64 [S, points, 3] = (FD_j, n_j real, n_j generated), "frechet"
    [S, points, 4], "real" / "fake" (the tables the segments index: see _aligned), "sub_seg" int32 [S * points, 2],
    "f_sub_seg", "seg", "perm"} with no host synchronisation."""
    real, fake = _table(real), _table(fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real has {real.shape[1]} columns, fake {fake.shape[1]}")
    P = int(points)
    if P < 3:
        raise ValueError(f"points = {P}: the fit of two parameters needs at least 3")
    dev = real.device
    with torch.cuda.device(dev):
        real, fake, seg, f_seg, perm = _aligned(real, fake, expert, n_experts)
        S = int(seg.shape[0])
        mult = torch.arange(P, 2 * P, dtype=torch.int64, device=dev)

        def prefixes(sg):
            b, L = sg[:, 0].long(), (sg[:, 1] - sg[:, 0]).long()
            n = (L[:, None] * mult[None, :]) // (2 * P - 1)
            return torch.stack([b[:, None].expand(S, P), b[:, None] + n], dim=2).reshape(S * P, 2).to(torch.int32)

        r_sub, f_sub = prefixes(seg), prefixes(f_seg)
        cnt_r, mean_r, cov_r = segment_moments(real, None, r_sub)
        cnt_f, mean_f, cov_f = segment_moments(fake, None, f_sub)
        fr = frechet(mean_r, cov_r, mean_f, cov_f)
        table = torch.stack([fr[:, 0], cnt_r.double(), cnt_f.double()], dim=1).reshape(S, P, 3)
    return {"table": table, "frechet": fr.reshape(S, P, 4), "real": real, "fake": fake, "sub_seg": r_sub,
            "f_sub_seg": f_sub, "seg": seg, "perm": perm}


def fpd(real, fake, expert=None, n_experts=1, points=10, details=False) -> dict:
    """The Frechet physics distance of the generated rows `fake` against the real rows `real` ([rows, cols <= 32]
    observable tables on the device, fp64 or fp32; normalise() them first).

    The Frechet distance between Gaussians fitted to the two sides is biased upwards by about 1 / n, so it is
    taken on `points` prefixes [b, b + n_j) of each segment, n_j = floor(L (points + j) / (2 points - 1)) from about
    L / 2 up to L, and extrapolated to 1 / n -> 0 by a least-squares line: "fpd" is the intercept, "fpd_err" its
    standard error, "fd_full" the plain distance over the whole segment.  expert [N] (then real and fake are
    aligned row by row, N rows each): one es_router_dispatch gives the joint segment (the rows in the order given)
    and `<name>_<e>` per expert (its rows in batch order).
    One es_segment_moments call per side over all (E + 1) x points prefixes, one es_frechet call, one small
    device-to-host copy; the fit is on the host in float64.  A segment whose shortest prefix has at most `cols`
    rows on either side gives NaN (its covariance is rank deficient).  details=True adds fpd_device's tensors.

    The prefixes take the rows in the order given: a test set that is ORDERED (by energy, by class, by run) makes
    the shorter prefixes differ from the whole in distribution, not only in size, and biases the extrapolation;
    shuffle such a set first.  jetnet draws random batches instead."""
    raw = fpd_device(real, fake, expert, n_experts, points)
    table = raw["table"].cpu().numpy()                                     # the one D2H copy
    out = summary_dict(fpd_from_table(table, int(real.shape[1])), None, per_expert=expert is not None)
    if details:
        out.update(raw)
    return out


def kpd_device(real, fake, expert=None, n_experts=1, blocks=10, degree=4):
    """The device half of `kpd`: {"table" fp64 [S, blocks + 1, 5] = (S_xx, S_yy, S_xy, m, n) with the whole segment
    last, "real" / "fake" (the fp32 tables the segments index: see _aligned), "sub_seg" int32
    [S * (blocks + 1), 2], "f_sub_seg", "seg", "perm"} with no host synchronisation."""
    real, fake = _table(real, f32=True), _table(fake, f32=True)
    K = int(blocks)
    if K < 1:
        raise ValueError(f"blocks = {K}")
    dev = real.device
    r_cap, f_cap = int(real.shape[0]), int(fake.shape[0])                  # no segment is longer than a side
    with torch.cuda.device(dev):
        real, fake, seg, f_seg, perm = _aligned(real, fake, expert, n_experts)
        S = int(seg.shape[0])
        step =torch.arange(K + 1, dtype=torch.int64, device=dev)

        def parts(sg):
            b, L = sg[:, 0].long(), (sg[:, 1] - sg[:, 0]).long()
            m = L // K
            lo = b[:, None] + m[:, None] * step[None, :]
            hi = lo + m[:, None]
            lo[:, K] = b                                                   # the whole segment last
            hi[:, K] = b + L
            return torch.stack([lo, hi], dim=2).reshape(S * (K + 1), 2).to(torch.int32)

        r_sub, f_sub = parts(seg), parts(f_seg)
        sums, counts = mmd_poly_sums(real, fake, degree=degree, r_seg=r_sub, r_cap=r_cap, f_seg=f_sub, f_cap=f_cap)
        table = torch.cat([sums[:, :3], counts.double()], dim=1).reshape(S, K + 1, 5)
    return {"table": table, "real": real, "fake": fake, "sub_seg": r_sub, "f_sub_seg": f_sub, "seg": seg,
            "perm": perm}


def kpd(real, fake, expert=None, n_experts=1, blocks=10, degree=4, details=False) -> dict:
    """The kernel physics distance of the generated rows `fake` against the real rows `real` ([rows, cols <= 64]
    observable tables on the device; normalise() them first; cast to fp32 for the kernel, which computes in fp64).

    Per segment `blocks` disjoint blocks of m = floor(L / blocks) consecutive positions, block t of real against
    block t of generated, and the whole segment: one es_mmd_poly call over all (E + 1) x (blocks + 1) of them and
    one small copy; on the host MMD^2 = S_xx / (m (m - 1)) + S_yy / (n (n - 1)) - 2 S_xy / (m n) with the kernel
    k(u, v) = (<u, v> / cols + 1)^degree.  "kpd" is the median over the blocks, "kpd_err" half their interquartile
    range, "mmd_full" the whole segment's value; `<name>_<e>` per expert with an expert vector (real and fake
    aligned).  A segment with m < 2 gives NaN.  The blocks take the rows in the order given (see `fpd`).
    details=True adds kpd_device's tensors."""
    raw = kpd_device(real, fake, expert, n_experts, blocks, degree)
    table = raw["table"].cpu().numpy()                                     # the one D2H copy
    out = summary_dict(None, kpd_from_table(table), per_expert=expert is not None)
    if details:
        out.update(raw)
    return out


def distances(real, fake, expert=None, n_experts=1, points=10, blocks=10, degree=4, details=False) -> dict:
    """`fpd` and `kpd` of the same tables over the same segments with ONE device-to-host copy for both: the six
    keys of summary_dict and `<name>_<e>` per expert.  details=True adds the device tensors "fpd_table",
    "fpd_frechet", "kpd_table"."""
    f = fpd_device(real, fake, expert, n_experts, points)
    k = kpd_device(real, fake, expert, n_experts, blocks, degree)
    ft, kt = f["table"], k["table"]
    host = torch.cat([ft.reshape(-1), kt.reshape(-1)]).cpu().numpy()       # the one D2H copy
    out = summary_dict(fpd_from_table(host[:ft.numel()].reshape(tuple(ft.shape)), int(real.shape[1])),
                       kpd_from_table(host[ft.numel():].reshape(tuple(kt.shape))), per_expert=expert is not None)
    if details:
        out.update(fpd_table=ft, fpd_frechet=f["frechet"], kpd_table=kt)
    return out
