"""fp64 numpy restatement of es_segment_histogram and es_segment_kde (csrc/diagnostics.hip) as
include/expertsim_hip.h defines them, the golden of the KDE tests and the bounds they share.

Binning (bin_index), against the edges e[0 .. bins] in fp64:
  right = 0  np.histogram(x, bins=e): b = searchsorted(e, x, 'right') - 1, so e[b] <= x < e[b+1]; x == e[bins]
             goes to the last bin.  All edges equal: every value in the last bin.
  right = 1  pd.cut(x, bins=e, include_lowest=True): b = searchsorted(e, x, 'left') - 1, so e[b] < x <= e[b+1];
             x == e[0] goes to bin 0.  All edges equal: every value in bin 0.
  A value below e[0] or above e[bins] is in no bin (-1) and counted as outside.

linspace_ref(lo, hi, num): div = num - 1, delta = hi - lo, step = delta / div, value k = k * step + lo (product
rounded, then added; (k / div) * delta + lo when step == 0), the last value hi itself, num == 1 gives [lo].

moments_ref: S, m = S / n, Q = sum of the rounded (d - m)^2 in es_group_diversity's order (prepare_refs: one
chain up to SPLIT_MIN members, else CHUNKS chunks of ceil(n / CHUNKS), chunk sums in chunk order from +0.0).

kde_ref, in the kernel's stated order: valid = n >= max(min_samples, 2), Q > 0 and not sqrt(Q / n) < std_eps;
sd = sqrt(Q / (n - 1)); bw = sd * n ** -0.2; r = 1 / bw; per grid point T = the members in chunks of KDE_CHUNK,
each chunk summed sequentially from +0.0 over exp(-0.5 * (z * z)), z = (g - d) * r, the chunk sums added in
chunk order from +0.0; density = T / ((n * bw) * SQRT_2PI).  numpy's exp and pow are the host library's, not
the device's, so this restates the ORDER; the truth for the values is the golden (np.longdouble).

Bounds (the issue's): bw within 17 * 2^-53 relative of the golden's h (16 ulp for the device library's pow by
the OpenCL bound, one for the product); density per grid point within (n + 40 A_j + 9) 2^-53 relative, A_j the
weighted mean exponent sum(a t) / sum(t), a = z^2 / 2, t = exp(-a): at most 5 roundings in the exponent plus
twice the 17-ulp bandwidth difference scale a term's relative error by a (40 A), 3 ulp for exp, n for the
positive sum, 4 for the normalisation, 0.5 for the golden's rounding (9 with the 3 and the slack).
"""
from __future__ import annotations

import functools
import os

import numpy as np

import prepare_refs as PR
from golden_utils import GOLDEN_DIR

U = 2.0 ** -53
KDE_CHUNK = 256            # ES_DIAG_KDE_CHUNK
SQRT_2PI = 2.5066282746310002
BW_BOUND = 17.0 * U
GOLDEN_CASES = ("n5", "n64", "n65", "n1000_clusters", "n4097")


def widen(x):
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    return x.astype(np.float64)


def linspace_ref(lo, hi, num):
    lo, hi = np.float64(lo), np.float64(hi)
    div = num - 1
    if div == 0:
        return np.array([lo])
    k = np.arange(num, dtype=np.float64)
    delta = hi - lo
    step = delta / np.float64(div)
    if step != 0.0:
        out = k * step
        out = out + lo
    else:
        out = k / np.float64(div)
        out = out * delta
        out = out + lo
    out[-1] = hi
    return out


def kde_grid_ref(lo, hi, points):
    lo, hi = np.float64(lo), np.float64(hi)
    if lo == hi:
        lo, hi = lo - 1e-6, hi + 1e-6
    return linspace_ref(lo, hi, points)


def bin_index(x, e, right):
    """Bin of every value of x against the edges e (-1: outside)."""
    x, e = widen(x), np.asarray(e, dtype=np.float64)
    bins = len(e) - 1
    if right:
        b = np.searchsorted(e, x, side="left") - 1
        b[(b < 0) & (x == e[0])] = 0
    else:
        b = np.searchsorted(e, x, side="right") - 1
        b[(b == bins) & (x == e[-1])] = bins - 1
    b[(b < 0) | (b >= bins)] = -1
    return b


def histogram_ref(x, e, right):
    """(counts [bins] int64, outside)."""
    b = bin_index(x, e, right)
    return np.bincount(b[b >= 0], minlength=len(e) - 1), int((b < 0).sum())


def segment_histogram_ref(x, members, bins, right, edges=None):
    """x [N, C]; members: per segment the row indices in member order -> (counts [S, C, bins] int32,
    edges [C, bins + 1], outside [S, C] int32).  edges None: linspace_ref of every column's range over all N."""
    x = widen(x)
    C = x.shape[1]
    if edges is None:
        edges = np.stack([linspace_ref(x[:, c].min(), x[:, c].max(), bins + 1) for c in range(C)])
    counts = np.zeros((len(members), C, bins), dtype=np.int32)
    outside = np.zeros((len(members), C), dtype=np.int32)
    for s, rows in enumerate(members):
        for c in range(C):
            counts[s, c], outside[s, c] = histogram_ref(x[np.asarray(rows, dtype=np.int64), c], edges[c], right)
    return counts, edges, outside


def moments_ref(d):
    """(S, m, Q) of the members d [n] (n >= 1) in the kernel's fixed order."""
    d = widen(d).reshape(-1, 1)
    n = np.float64(d.shape[0])
    S = PR._member_sum(d)[0]
    m = S / n
    return S, m, PR._member_sum(d, m)[0]


def kde_ref(d, grid, min_samples=5, std_eps=1e-12):
    """{valid, sd, bw, density [points]} of the members d [n] on grid, in the kernel's order."""
    d, grid = widen(d).reshape(-1), np.asarray(grid, dtype=np.float64)
    n = d.shape[0]
    bad = dict(valid=0, sd=0.0, bw=0.0, density=np.full(grid.shape, np.nan))
    if n < max(int(min_samples), 2):
        return bad
    dn = np.float64(n)
    _, _, Q = moments_ref(d)
    if Q == 0.0 or np.sqrt(Q / dn) < std_eps:
        return bad
    sd = np.sqrt(Q / (dn - 1.0))
    bw = sd * dn ** -0.2
    r = 1.0 / bw
    total = np.zeros(grid.shape, dtype=np.float64)
    for first in range(0, n, KDE_CHUNK):
        acc = np.zeros(grid.shape, dtype=np.float64)
        for v in d[first:first + KDE_CHUNK]:
            z = (grid - v) * r
            a = z * z
            acc = acc + np.exp(-0.5 * a)
        total = total + acc
    return dict(valid=1, sd=sd, bw=bw, density=total / ((dn * bw) * SQRT_2PI))


def kde_bound(n, A):
    """Relative bound on the density per grid point: (n + 40 A_j + 9) 2^-53."""
    return (np.float64(n) + 40.0 * np.asarray(A, dtype=np.float64) + 9.0) * U


def check_density(got, case):
    """Worst error / bound of a device density row against a golden case; asserts the issue's rule."""
    got = np.asarray(got, dtype=np.float64)
    want, A, n = case["density"], case["A"], len(case["d"])
    tiny = want < 2.0 ** -1000
    assert (got[tiny] < 2.0 ** -999).all()
    assert np.isfinite(got).all() and (got >= 0.0).all()
    rel = np.abs(got[~tiny] - want[~tiny]) / want[~tiny]
    ratio = rel / kde_bound(n, A[~tiny])
    assert (ratio <= 1.0).all(), (float(ratio.max()), int(ratio.argmax()))
    return float(ratio.max()) if ratio.size else 0.0


@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/diag_kde.npz (tools/make_diag_golden.py): {case: {d, grid, sd, h, density, A}}, read-only."""
    z = np.load(os.path.join(GOLDEN_DIR, "diag_kde.npz"))
    out = {}
    for name in GOLDEN_CASES:
        out[name] = {k: z[f"{name}_{k}"] for k in ("d", "grid", "sd", "h", "density", "A")}
        for a in out[name].values():
            a.setflags(write=False)
    return out
