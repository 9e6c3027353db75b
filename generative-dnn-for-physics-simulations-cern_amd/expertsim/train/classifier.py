"""Classifier two-sample test on the device: how well can the best rule of a fixed family tell the generated
showers from the real ones, on rows the rule never saw?  The CaloChallenge reports it as "AUC / JSD of a classifier
on high-level features"; Kansal et al. 2023 compare `fpd` / `kpd` (train/distances.py) against it.

The family is fixed so that the result is a function of the data: ridge-penalised logistic regression on the
standardised observables and (degree 2) their pairwise products, a quadratic decision surface.  The objective is
strictly convex and has one optimum, so "the classifier" does not depend on an optimiser's path.  HIP kernels
(csrc/rank.hip, csrc/classifier.hip, defined in include/expertsim_hip.h):

* ``es_rank_stats``    Mann-Whitney rank sum (ROC AUC) and Kolmogorov-Smirnov statistic per (segment, column), exact
                       integers from the tagged sort es_wasserstein_1d uses;
* ``es_logit_fit``     safeguarded Newton steps in fp64 per segment, Cholesky in the kernel, no host synchronisation;
* ``es_logit_scores``  the scores of every member of every segment and the sums behind accuracy and log-loss.

There is no CPU fallback: without a HIP device every device function raises hip.HipError.  The host halves
(`split_segments_host`, `summary_from_table`) are pure numpy.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import hip
from ..segments import is_f64, ld, work_buffer
from .distances import _aligned, _segments, _table, segment_moments

KEYS = ("c2st_auc", "c2st_ks", "c2st_acc", "c2st_logloss", "c2st_iter", "c2st_converged")
MAX_BASE_COLS = 11          # degree 2: 11 + 66 = 77 <= hip.LOGIT_MAX_COLS


def _need_device():
    if not torch.cuda.is_available():
        raise hip.HipError("the classifier two-sample test needs a HIP device (no CPU fallback)")


def _sides(real, fake, r_idx, r_seg, r_cap, f_idx, f_seg, f_cap):
    if real.device != fake.device:
        raise ValueError("real and fake are on different devices")
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real has {real.shape[1]} columns, fake {fake.shape[1]}")
    r_idx, r_seg, n_seg = _segments(real, r_idx, r_seg)
    f_idx, f_seg, f_n_seg = _segments(fake, f_idx, f_seg)
    if n_seg != f_n_seg:
        raise ValueError(f"{n_seg} real segments, {f_n_seg} generated")
    r_cap = int(real.shape[0]) if r_cap is None else int(r_cap)
    f_cap = int(fake.shape[0]) if f_cap is None else int(f_cap)
    return r_idx, r_seg, r_cap, f_idx, f_seg, f_cap, n_seg


def _same_type(real, fake):
    """Both tables fp64, or both fp32 (the kernels take one type for the two)."""
    real, fake = _table(real), _table(fake)
    if real.dtype != fake.dtype:
        real, fake = _table(real.double()), _table(fake.double())
    return real, fake


# ------------------------------------------------------------------------------------------ thin wrappers
def rank_stats(u, v, u_idx=None, u_seg=None, u_cap=None, v_idx=None, v_seg=None, v_cap=None, out=None) -> torch.Tensor:
    """es_rank_stats: int64 [n_seg, channels, 4] = (nu, nv, U2, KS) on the device for the columns of u / v
    [rows, channels] (cast to fp64).  U2 / (2 nu nv) is the ROC AUC of u against v with ties counted half (U2 / 2 the
    Mann-Whitney U of u), KS / (nu nv) the two-sample Kolmogorov-Smirnov statistic.  Segments, idx and caps as
    train.utils.wasserstein_1d_device; a segment empty on either side gives (nu, nv, 0, 0).  Values must be finite.
    out: the tensor to write into (its first n_seg entries)."""
    _need_device()
    u, v = _table(u).double(), _table(v).double()
    u_idx, u_seg, u_cap, v_idx, v_seg, v_cap, n_seg = _sides(u, v, u_idx, u_seg, u_cap, v_idx, v_seg, v_cap)
    ch, dev = int(u.shape[1]), u.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(n_seg, ch, 4, dtype=torch.int64, device=dev)
        need = hip.rank_stats_workspace(n_seg, ch, u_cap, v_cap)
        work = work_buffer(need, dev)
        hip.call("es_rank_stats", hip.ptr(u), ld(u), int(u.shape[0]), hip.ptr(u_idx), hip.ptr(u_seg), hip.ptr(v), ld(v),
                 int(v.shape[0]), hip.ptr(v_idx), hip.ptr(v_seg), n_seg, ch, u_cap, v_cap, hip.ptr(out), hip.ptr(work),
                 int(work.numel()) if need else 0, hip.stream_ptr())
    return out


def logit_fit(real, fake, l2=1.0, max_iter=50, gtol=1e-9, r_idx=None, r_seg=None, r_cap=None, f_idx=None, f_seg=None,
              f_cap=None, out=None):
    """es_logit_fit: (theta fp64 [n_seg, cols + 1] intercept first, stat fp64 [n_seg, 4] = (F, |g|_inf, iterations,
    status)) on the device: per segment the ridge-penalised logistic regression of real (label 1) against fake
    (label 0) [rows, cols <= 80], fp32 or fp64, by safeguarded Newton steps from theta = 0.  l2 is scikit-learn's
    1 / C; the intercept is unpenalised.  status 1: |g|_inf <= gtol; 0: max_iter (<= 100) reached; -1: a side is
    empty (theta NaN).  No host synchronisation.  out: the two tensors to write into."""
    _need_device()
    real, fake = _same_type(real, fake)
    r_idx, r_seg, r_cap, f_idx, f_seg, f_cap, n_seg = _sides(real, fake, r_idx, r_seg, r_cap, f_idx, f_seg, f_cap)
    cols, dev = int(real.shape[1]), real.device
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(n_seg, cols + 1, dtype=torch.float64, device=dev),
                   torch.empty(n_seg, 4, dtype=torch.float64, device=dev))
        theta, stat = out
        need = hip.logit_fit_workspace(n_seg, cols, r_cap, f_cap)
        work = work_buffer(need, dev)
        hip.call("es_logit_fit", hip.ptr(real), ld(real), int(real.shape[0]), hip.ptr(r_idx), hip.ptr(r_seg), r_cap,
                 hip.ptr(fake), ld(fake), int(fake.shape[0]), hip.ptr(f_idx), hip.ptr(f_seg), f_cap, is_f64(real), cols,
                 n_seg, float(l2), float(gtol), int(max_iter), hip.ptr(theta), hip.ptr(stat), hip.ptr(work),
                 int(work.numel()) if need else 0, hip.stream_ptr())
    return theta, stat


def logit_scores(real, fake, theta, r_idx=None, r_seg=None, r_cap=None, f_idx=None, f_seg=None, f_cap=None, out=None):
    """es_logit_scores: {"r_scores" fp64 [n_seg, r_cap], "f_scores" [n_seg, f_cap], "r_seg" / "f_seg" int32
    [n_seg, 2], "sums" fp64 [n_seg, 4]} on the device for theta [n_seg, cols + 1] as logit_fit returns it.  The score
    of real member i of segment s is r_scores[s, i]; r_seg / f_seg bound every segment's scores inside the flattened
    tables, so `rank_stats(r_scores.reshape(-1, 1), f_scores.reshape(-1, 1), u_seg=r_seg, v_seg=f_seg, u_cap=r_cap,
    v_cap=f_cap)` ranks them with no length on the host (entries past a segment's length are not written).
    sums = (real members with t > 0, generated members with t <= 0, log-loss over the real members, over the
    generated).  out: the five tensors in that order."""
    _need_device()
    real, fake = _same_type(real, fake)
    r_idx, r_seg, r_cap, f_idx, f_seg, f_cap, n_seg = _sides(real, fake, r_idx, r_seg, r_cap, f_idx, f_seg, f_cap)
    cols, dev = int(real.shape[1]), real.device
    hip.require_device(theta)
    theta = theta.to(torch.float64).contiguous()
    if tuple(theta.shape) != (n_seg, cols + 1):
        raise ValueError(f"theta must be [{n_seg}, {cols + 1}], got {tuple(theta.shape)}")
    with torch.cuda.device(dev):
        if out is None:
            out = (torch.empty(n_seg, max(r_cap, 1), dtype=torch.float64, device=dev),
                   torch.empty(n_seg, max(f_cap, 1), dtype=torch.float64, device=dev),
                   torch.empty(n_seg, 2, dtype=torch.int32, device=dev),
                   torch.empty(n_seg, 2, dtype=torch.int32, device=dev),
                   torch.empty(n_seg, 4, dtype=torch.float64, device=dev))
        r_scores, f_scores, r_oseg, f_oseg, sums = out
        need = hip.logit_scores_workspace(n_seg, r_cap, f_cap)
        work = work_buffer(need, dev)
        hip.call("es_logit_scores", hip.ptr(real), ld(real), int(real.shape[0]), hip.ptr(r_idx), hip.ptr(r_seg), r_cap,
                 hip.ptr(fake), ld(fake), int(fake.shape[0]), hip.ptr(f_idx), hip.ptr(f_seg), f_cap, is_f64(real), cols,
                 n_seg, hip.ptr(theta), hip.ptr(r_scores), hip.ptr(f_scores), hip.ptr(r_oseg), hip.ptr(f_oseg),
                 hip.ptr(sums), hip.ptr(work), int(work.numel()) if need else 0, hip.stream_ptr())
    return {"r_scores": r_scores, "f_scores": f_scores, "r_seg": r_oseg, "f_seg": f_oseg, "sums": sums}


# ------------------------------------------------------------------------------------------ host halves
def split_segments_host(seg) -> tuple:
    """(train [S, 2], held_out [S, 2]) int64 from seg [S, 2]: the first ceil(L / 2) positions of every segment train,
    the rest are held out (numpy; `c2st` does the same arithmetic on the device)."""
    seg = np.asarray(seg, dtype=np.int64).reshape(-1, 2)
    b, e = seg[:, 0], np.maximum(seg[:, 1], seg[:, 0])
    mid = b + (e - b + 1) // 2
    return np.stack([b, mid], axis=1), np.stack([mid, e], axis=1)


def feature_count(cols: int, degree: int) -> int:
    """Columns of the feature table: cols, plus cols (cols + 1) / 2 products for degree 2."""
    cols, degree = int(cols), int(degree)
    if degree not in (1, 2):
        raise ValueError(f"degree = {degree}: 1 (the columns) or 2 (and their pairwise products)")
    total = cols + (cols * (cols + 1) // 2 if degree == 2 else 0)
    if cols < 1 or total > hip.LOGIT_MAX_COLS:
        raise ValueError(f"{cols} columns at degree {degree} make {total} features: at most {hip.LOGIT_MAX_COLS} "
                         f"(degree 2: cols <= {MAX_BASE_COLS})")
    return total


def summary_from_table(table, per_expert=True) -> dict:
    """KEYS from segment 0 of table [S, 12] = (nu, nv, U2, KS, real t > 0, generated t <= 0, log-loss real, log-loss
    generated, F, |g|_inf, iterations, status), the host copy of `c2st`'s device result, and `<key>_<e>` from segment
    1 + e.  c2st_auc = U2 / (2 nu nv), c2st_ks = KS / (nu nv), c2st_acc = (hits_real / nu + hits_generated / nv) / 2,
    c2st_logloss = (both sums) / (nu + nv), c2st_iter, c2st_converged = 1.0 where status is 1.  A segment whose
    held-out half is empty on either side, or whose training half was (status -1), gives NaN in all six."""
    t = np.asarray(table, dtype=np.float64).reshape(-1, 12)
    out = {}
    for s in range(t.shape[0]):
        nu, nv, u2, ks, hr, hf, lr, lf, _, _, it, status = t[s]
        if nu > 0 and nv > 0 and status >= 0:
            vals = (u2 / (2.0 * nu * nv), ks / (nu * nv), 0.5 * (hr / nu + hf / nv), (lr + lf) / (nu + nv), it,
                    1.0 if status == 1 else 0.0)
        else:
            vals = (np.nan,) * 6
        if s == 0:
            out.update({k: float(v) for k, v in zip(KEYS, vals)})
        elif per_expert:
            out.update({f"{k}_{s - 1}": float(v) for k, v in zip(KEYS, vals)})
    return out


# ------------------------------------------------------------------------------------------ c2st
def standardise(real, fake):
    """(real_z, fake_z, shift, scale) fp64: one shift and scale for both tables and all segments, the pooled mean and
    1 / (population standard deviation) of the two tables' rows together, from one es_segment_moments call per side
    and torch arithmetic on the device; the scale is 0 where the deviation is 0, so a constant column drops out."""
    real, fake = _table(real), _table(fake)
    cr, mr, vr = segment_moments(real)
    cf, mf, vf = segment_moments(fake)
    nr, nf = cr[0].double(), cf[0].double()
    n = nr + nf
    mu = (nr * mr[0] + nf * mf[0]) / n
    # np.cov divides by n - 1: a side of one row has NaN there and no spread of its own
    ssr = torch.where(nr > 1, torch.diagonal(vr[0]) * (nr - 1), torch.zeros_like(mu))
    ssf = torch.where(nf > 1, torch.diagonal(vf[0]) * (nf - 1), torch.zeros_like(mu))
    var = (ssr + nr * (mr[0] - mu) ** 2 + ssf + nf * (mf[0] - mu) ** 2) / n
    std = var.clamp_min(0).sqrt()
    scale = torch.where(std > 0, 1.0 / std, torch.zeros_like(std))
    return (real.double() - mu) * scale, (fake.double() - mu) * scale, mu, scale


def expand(z, degree=2) -> torch.Tensor:
    """The feature table of z [rows, cols] fp64: the columns, then for degree 2 the products z_i z_j, i <= j, in
    row-major order of (i, j) (torch.triu_indices)."""
    cols = int(z.shape[1])
    feature_count(cols, degree)
    if int(degree) == 1:
        return z.contiguous()
    iu = torch.triu_indices(cols, cols, device=z.device)
    return torch.cat([z, z[:, iu[0]] * z[:, iu[1]]], dim=1).contiguous()


def c2st_device(real, fake, expert=None, n_experts=1, degree=2, l2=1.0, max_iter=50, gtol=1e-9) -> dict:
    """The device half of `c2st`: {"table" fp64 [S, 12] (see summary_from_table), "theta" [S, features + 1], "stat"
    [S, 4], "rank" int64 [S, 1, 4], "sums" [S, 4], "r_scores", "f_scores", "score_r_seg", "score_f_seg", "real" /
    "fake" (the feature tables the segments index: see distances._aligned), "train_seg", "f_train_seg", "test_seg",
    "f_test_seg", "seg", "perm", "shift", "scale"} with no host synchronisation."""
    _need_device()
    real, fake = _table(real), _table(fake)
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f"real has {real.shape[1]} columns, fake {fake.shape[1]}")
    feature_count(int(real.shape[1]), degree)
    dev = real.device
    n_r, n_f = int(real.shape[0]), int(fake.shape[0])                      # no segment is longer than a side
    with torch.cuda.device(dev):
        zr, zf, shift, scale = standardise(real, fake)
        xr, xf, seg, f_seg, perm = _aligned(expand(zr, degree), expand(zf, degree), expert, n_experts)

        def halves(sg):
            b, e = sg[:, 0].long(), torch.maximum(sg[:, 1], sg[:, 0]).long()
            mid = b + (e - b + 1) // 2
            return (torch.stack([b, mid], dim=1).to(torch.int32).contiguous(),
                    torch.stack([mid, e], dim=1).to(torch.int32).contiguous())

        (r_train, r_test), (f_train, f_test) = halves(seg), halves(f_seg)
        tr_caps = dict(r_cap=max((n_r + 1) // 2, 1), f_cap=max((n_f + 1) // 2, 1))
        te_caps = dict(r_cap=max(n_r // 2, 1), f_cap=max(n_f // 2, 1))
        theta, stat = logit_fit(xr, xf, l2=l2, max_iter=max_iter, gtol=gtol, r_seg=r_train, f_seg=f_train, **tr_caps)
        sc = logit_scores(xr, xf, theta, r_seg=r_test, f_seg=f_test, **te_caps)
        rank = rank_stats(sc["r_scores"].reshape(-1, 1), sc["f_scores"].reshape(-1, 1), u_seg=sc["r_seg"],
                          v_seg=sc["f_seg"], u_cap=te_caps["r_cap"], v_cap=te_caps["f_cap"])
        table = torch.cat([rank[:, 0, :].double(), sc["sums"], stat], dim=1)
    return {"table": table, "theta": theta, "stat": stat, "rank": rank, "sums": sc["sums"], "r_scores": sc["r_scores"],
            "f_scores": sc["f_scores"], "score_r_seg": sc["r_seg"], "score_f_seg": sc["f_seg"], "real": xr, "fake": xf,
            "train_seg": r_train, "f_train_seg": f_train, "test_seg": r_test, "f_test_seg": f_test, "seg": seg,
            "perm": perm, "shift": shift, "scale": scale}


def c2st(real, fake, expert=None, n_experts=1, degree=2, l2=1.0, max_iter=50, gtol=1e-9, details=False) -> dict:
    """The classifier two-sample test of the generated rows `fake` against the real rows `real` ([rows, cols]
    observable tables on the device, fp64 or fp32; NOT normalised: the test standardises them itself).

    Both tables are shifted and scaled by their pooled mean and population standard deviation (a constant column
    drops out).  degree=2 appends the cols (cols + 1) / 2 pairwise products of the standardised columns (cols <= 11,
    ValueError otherwise), degree=1 uses the columns alone.  Per segment the first ceil(L / 2) positions of each
    side train a ridge-penalised logistic regression (l2 = scikit-learn's 1 / C, the intercept unpenalised, Newton
    steps to |g|_inf <= gtol or max_iter), real rows labelled 1, and the remaining positions are scored:

      c2st_auc        ROC AUC of the held-out scores (0.5: indistinguishable), exact from the Mann-Whitney rank sum
      c2st_ks         two-sample Kolmogorov-Smirnov statistic of the held-out scores
      c2st_acc        held-out accuracy at t = 0, the two sides weighted equally
      c2st_logloss    held-out mean log-loss; ln 2 - c2st_logloss is the estimate of the Jensen-Shannon divergence
                      that the CaloChallenge quotes as the classifier's "JSD"
      c2st_iter       Newton moves taken
      c2st_converged  1.0 where |g|_inf <= gtol was reached

    expert [N] (then real and fake are aligned row by row, N rows each): one es_router_dispatch gives the joint
    segment (the rows in the order given) and `<key>_<e>` per expert (its rows in batch order, gathered behind the
    joint rows as for `fpd`).  One es_logit_fit over all E + 1 training problems, one es_logit_scores and one
    es_rank_stats over the held-out halves, one small device-to-host copy.  Where a half is empty on either side
    the six values are NaN.  details=True adds c2st_device's tensors.

    The halves take the rows in the order given: a test set that is ORDERED (by energy, by class, by run) makes the
    training half differ from the held-out half in distribution, and the held-out score then measures that shift
    too; shuffle such a set first (see `distances.fpd`)."""
    raw = c2st_device(real, fake, expert, n_experts, degree, l2, max_iter, gtol)
    table = raw["table"].cpu().numpy()                                     # the one D2H copy
    out = summary_from_table(table, per_expert=expert is not None)
    if details:
        out.update(raw)
    return out
