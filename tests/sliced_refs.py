"""numpy / scipy restatement of the sliced Wasserstein distance (csrc/sliced.hip, expertsim/train/sliced.py), the
seeded inputs its tests share and the derived bounds.  u = 2^-53 throughout.

* project_ref accumulates in np.longdouble, so its own rounding stays out of the bounds.
* w_table takes the 1-D distances of the projected columns from scipy.stats.wasserstein_distance.
* Bounds (derived, not measured):
    projection   |out - ref| <= (D + 1) u sum_d |x_d| |theta_d|         a dot product of D terms in any order
                                                                         (Higham, Accuracy and Stability, ch. 3)
    direction    |theta - ref| <= (D / 2 + 3) u |ref|                    the sum of squares ((D - 1) u, halved by
                                                                         the square root), the root, the division
    distance     |w - ref| <= 2 m 2^-52 ref                              tests/test_wasserstein_gpu.py, m values
    end to end   the distance bound + the largest projection bound of either side along that direction: W1 moves
                 by at most the mean absolute perturbation of the samples
    summary      swd: the mean of the entries' bounds + (P + 1) u mean |w|; swd_max: the largest entry bound (a
                 maximum is 1-Lipschitz); swd_err = std / sqrt(P): centring is a projection, so the standard
                 deviation moves by at most |delta|_2 / sqrt(P - 1) <= max bound sqrt(P / (P - 1)), hence
                 max bound / sqrt(P - 1), + (P + 8) u swd_err for the two-pass moments' own rounding.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from golden_utils import GOLDEN_DIR

U = 2.0 ** -53
GOLDEN = os.path.join(GOLDEN_DIR, "sliced_numpy.npz")
RECORD_SHAPES = [(6, 5), (44, 44)]
RECORD_N = 257
RECORD_P = 64
RECORD_E = 3


@functools.lru_cache(maxsize=None)
def images(h, w, n, seed=0, shift=0.0):
    """Seeded float32 images [n,h,w] in the style of tests/feature_refs.py (read-only): expm1(relu(normal + shift))
    with an all-zero image among them when n allows."""
    rng = np.random.default_rng(7000 * h + 70 * w + n + 100003 * seed)
    x = np.expm1(np.maximum(rng.standard_normal((n, h, w)) + shift, 0.0)).astype(np.float32)
    if n >= 5:
        x[1] = 0.0
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def normal_theta(p, d, seed=0):
    """Seeded fp64 directions [p, d] for the projection tests (read-only): normal draws, normalised in fp64."""
    rng = np.random.default_rng(31 * p + d + 1009 * seed)
    t = rng.standard_normal((p, d))
    t /= np.sqrt((t * t).sum(axis=1, keepdims=True))
    t.setflags(write=False)
    return t


def record_theta16(h, w):
    """The record's direction matrix as it is stored: float16 [RECORD_P, h * w], normal draws normalised and rounded
    to float16 (a quarter of the bytes; unit to within 2^-11 relative, and exact when widened to fp64)."""
    rng = np.random.default_rng(52000 + 100 * h + w)
    t = rng.standard_normal((RECORD_P, h * w))
    t /= np.sqrt((t * t).sum(axis=1, keepdims=True))
    return t.astype(np.float16)


@functools.lru_cache(maxsize=None)
def record_inputs(h, w):
    """(real [N,h,w] f32, fake [N,h,w] f32, expert [N] int32) of a record case (read-only): E = 3, expert 1 empty,
    expert 2 holding the single row 100."""
    real, fake = images(h, w, RECORD_N, seed=1), images(h, w, RECORD_N, seed=2, shift=0.25)
    expert = np.zeros(RECORD_N, dtype=np.int32)
    expert[100] = 2
    expert.setflags(write=False)
    return real, fake, expert


def members(expert, n_experts):
    """Row indices of the joint segment and of every expert's, in batch order."""
    return [np.arange(len(expert))] + [np.where(expert == e)[0] for e in range(n_experts)]


# ------------------------------------------------------------------------------------------ restatement
def project_ref(x, theta):
    """(ref [n, P] np.longdouble, absum [n, P] float64 = sum_d |x_d| |theta_d|) for x [n,h,w] float32 (or fp64 values
    of a widened bf16) and theta [P, D] float64."""
    n = x.shape[0]
    a = np.asarray(x).reshape(n, -1).astype(np.longdouble)
    t = np.asarray(theta, dtype=np.float64)
    ref = a @ t.T.astype(np.longdouble)
    absum = np.abs(a).astype(np.float64) @ np.abs(t).T
    return ref, absum


def project_bound(d, absum):
    return (d + 1) * U * absum


def directions_ref(draws, d):
    """draws [P, >= d] float32 (es_randn's) -> the first d of each row normalised in np.longdouble."""
    v = np.asarray(draws)[:, :d].astype(np.longdouble)
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True))


def direction_bound(d, ref):
    return (d / 2 + 3) * U * np.abs(np.asarray(ref, dtype=np.float64))


def w_table(proj_r, proj_f, mem_r, mem_f=None):
    """scipy's [n_seg, P] table of 1-D distances between the columns of proj_r[mem_r[s]] and proj_f[mem_f[s]]; 0 where
    a segment is empty on either side (as es_wasserstein_1d writes it)."""
    from scipy.stats import wasserstein_distance
    mem_f = mem_r if mem_f is None else mem_f
    pr, pf = np.asarray(proj_r, dtype=np.float64), np.asarray(proj_f, dtype=np.float64)
    out = np.zeros((len(mem_r), pr.shape[1]))
    for s, (ir, jf) in enumerate(zip(mem_r, mem_f)):
        if len(ir) == 0 or len(jf) == 0:
            continue
        for p in range(pr.shape[1]):
            out[s, p] = wasserstein_distance(pr[ir, p], pf[jf, p])
    return out


def ws_bound(m, ref):
    return 2 * m * 2.0 ** -52 * np.asarray(ref)


def summary_ref(w, counts):
    """[3, n_seg] = (swd, swd_err, swd_max) of a [n_seg, P] table; NaN where counts [n_seg, 2] has a zero (and for
    swd_err when P < 2)."""
    w = np.asarray(w, dtype=np.float64)
    P = w.shape[1]
    out = np.full((3, w.shape[0]), np.nan)
    for s in range(w.shape[0]):
        if counts[s][0] == 0 or counts[s][1] == 0:
            continue
        out[0, s] = w[s].mean()
        out[1, s] = np.sqrt(w[s].var(ddof=1) / P) if P >= 2 else np.nan
        out[2, s] = w[s].max()
    return out


def summary_bounds(w_ref, entry_bound):
    """[3, n_seg] bounds of (swd, swd_err, swd_max) from the per-entry bounds [n_seg, P] of the table (module
    docstring)."""
    w = np.asarray(w_ref, dtype=np.float64)
    P = w.shape[1]
    b = np.asarray(entry_bound, dtype=np.float64)
    err = np.sqrt(w.var(axis=1, ddof=1) / P) if P >= 2 else np.zeros(w.shape[0])
    return np.stack([b.mean(axis=1) + (P + 1) * U * np.abs(w).mean(axis=1),
                     b.max(axis=1) / np.sqrt(max(P - 1, 1)) + (P + 8) * U * err,
                     b.max(axis=1)])


def record_case(h, w):
    """The restatement of a record case: (theta [P, D] f64, table [E + 1, P], summary [3, E + 1], counts [E + 1, 2],
    proj_bound [P]: the largest projection bound of either side along each direction)."""
    real, fake, expert = record_inputs(h, w)
    theta = record_theta16(h, w).astype(np.float64)
    (pr, ar), (pf, af) = project_ref(real, theta), project_ref(fake, theta)
    mem = members(expert, RECORD_E)
    table = w_table(pr.astype(np.float64), pf.astype(np.float64), mem)
    counts = np.array([[len(m), len(m)] for m in mem])
    bound = np.maximum(project_bound(h * w, ar).max(axis=0), project_bound(h * w, af).max(axis=0))
    return theta, table, summary_ref(table, counts), counts, bound


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(GOLDEN)
    out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out
