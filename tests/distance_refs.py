"""Numpy restatement of the distribution-distance kernels (include/expertsim_hip.h: es_segment_moments, es_frechet,
es_mmd_poly) and of the inputs of their record, shared by tests/test_distances_*.py and
tools/make_distance_golden.py.  scipy and scikit-learn are imported only by the functions the tool calls.

Bounds (derived, not measured; u = 2^-53):
* a mean of n terms summed in any order and divided once: (n + 1) u sum|x| / n;
* a covariance entry, centred on a rounded mean, n products summed in any order and divided once:
  (n + 4) 2 u sum|x_i - mu_i||x_j - mu_j| / (n - 1) (the doubling covers the rounded mean);
* a kernel sum of T terms in any order, each term a dot product of `cols` terms, one scale-and-shift and
  degree - 1 multiplications: (T - 1 + cols + degree + 2) u sum|k| (Higham, Accuracy and Stability, ch. 3-4).
The kernel sums here are accumulated in extended precision (np.longdouble) so that the restatement's own rounding
does not eat into the bound.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distances_scipy.npz")
U = 2.0 ** -53


def load_golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------ moments
def moments(x):
    """(n, mean [cols], cov [cols, cols]) of the rows x [n, cols] in fp64: np.mean and np.cov(rowvar=False); NaN in
    cov for n < 2 and in mean for n == 0, as es_segment_moments writes them."""
    x = np.asarray(x, dtype=np.float64)
    n, cols = x.shape
    mean = x.mean(axis=0) if n > 0 else np.full(cols, np.nan)
    cov = np.cov(x, rowvar=False).reshape(cols, cols) if n > 1 else np.full((cols, cols), np.nan)
    return n, mean, cov


def moment_bounds(x):
    """(mean bound [cols], cov bound [cols, cols]) of the module docstring for the rows x [n >= 2, cols]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    d = np.abs(x - x.mean(axis=0))
    return (n + 1) * U * np.abs(x).sum(axis=0) / n, (n + 4) * 2 * U * (d.T @ d) / (n - 1)


# ------------------------------------------------------------------------------------------ Frechet
def frechet_unit(mean_a, cov_a, mean_b, cov_b):
    """U = 2^-52 cols (tr A + tr B + |dmu|^2), the unit of every Frechet tolerance."""
    dm = np.asarray(mean_a) - np.asarray(mean_b)
    return 2.0 ** -52 * len(dm) * (np.trace(cov_a) + np.trace(cov_b) + float(dm @ dm))


def frechet_eigh(mean_a, cov_a, mean_b, cov_b):
    """[4] = (d2, |dmu|^2, tr A + tr B, tr (A B)^1/2) in the symmetric form es_frechet computes: A^1/2 from
    np.linalg.eigh with the eigenvalues clipped at 0, then the clipped spectrum of A^1/2 B A^1/2."""
    a, b = np.asarray(cov_a, dtype=np.float64), np.asarray(cov_b, dtype=np.float64)
    dm = np.asarray(mean_a, dtype=np.float64) - np.asarray(mean_b, dtype=np.float64)
    if np.isnan(a).any() or np.isnan(b).any() or np.isnan(dm).any():
        return np.full(4, np.nan)
    w, v = np.linalg.eigh(a)
    h = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = h @ b @ h
    mu = np.linalg.eigvalsh(0.5 * (m + m.T))
    root = float(np.sqrt(np.clip(mu, 0.0, None)).sum())
    dmu2, trs = float(dm @ dm), float(np.trace(a) + np.trace(b))
    return np.array([dmu2 + trs - 2.0 * root, dmu2, trs, root])


def frechet_sqrtm(mean_a, cov_a, mean_b, cov_b):
    """The same four numbers with scipy.linalg.sqrtm(A @ B), the usual FID formulation."""
    from scipy.linalg import sqrtm
    a, b = np.asarray(cov_a, dtype=np.float64), np.asarray(cov_b, dtype=np.float64)
    dm = np.asarray(mean_a, dtype=np.float64) - np.asarray(mean_b, dtype=np.float64)
    root = float(np.real(np.trace(np.atleast_2d(sqrtm(a @ b)))))
    dmu2, trs = float(dm @ dm), float(np.trace(a) + np.trace(b))
    return np.array([dmu2 + trs - 2.0 * root, dmu2, trs, root])


def gauss_rows(rs, n, cols, spread=10.0):
    """n rows of a correlated Gaussian: iid normals times a random matrix with singular values 1 .. spread (a
    covariance with condition number about spread^2 times the sampling spread), plus an offset."""
    q1, _ = np.linalg.qr(rs.randn(cols, cols))
    q2, _ = np.linalg.qr(rs.randn(cols, cols))
    mix = (q1 * np.logspace(0.0, np.log10(spread), cols)) @ q2
    return rs.randn(n, cols) @ mix + rs.randn(cols)


def observable_rows(rs, n, cols):
    """n rows of non-negative, correlated, observable-like columns divided by their column maxima (the data
    `normalise` hands to the kernels): a shared energy scale times per-column gamma factors."""
    energy = rs.gamma(4.0, 1.0, size=(n, 1))
    x = energy * rs.gamma(6.0, 1.0, size=(n, cols)) * (0.5 + rs.rand(cols))
    return x / np.abs(x).max(axis=0)


FRECHET_CASES = (("gauss", 1), ("gauss", 2), ("gauss", 10), ("gauss", 32), ("obs", 1), ("obs", 2), ("obs", 10),
                 ("obs", 32))
FRECHET_ROWS = 300


def frechet_case(kind, cols):
    """(rows_a, rows_b) of a Frechet case, fp64 [FRECHET_ROWS, cols] each."""
    rs = np.random.RandomState(1000 + 37 * cols + (0 if kind == "gauss" else 1))
    if kind == "gauss":
        a = gauss_rows(rs, FRECHET_ROWS, cols)
        return a, 1.1 * gauss_rows(rs, FRECHET_ROWS, cols) + 0.3
    a = observable_rows(rs, FRECHET_ROWS, cols)
    return a, 0.9 * observable_rows(rs, FRECHET_ROWS, cols) + 0.02


# ------------------------------------------------------------------------------------------ polynomial-kernel sums
def poly_sums(x, y, degree=4, gamma=None, coef0=1.0):
    """(sums [3], abs sums [3]) = (S_xx, S_yy, S_xy) of es_mmd_poly and the sums of |k| over the same pairs, for the
    fp32 rows x [m, cols], y [n, cols].  Kernel values in extended precision; the diagonal of xx / yy is left out
    by index."""
    x, y = np.asarray(x, dtype=np.float32), np.asarray(y, dtype=np.float32)
    cols = x.shape[1]
    g = np.longdouble(1.0 / cols if gamma is None else gamma)
    sums, absum = np.zeros(3), np.zeros(3)
    for i, (a, b, sym) in enumerate(((x, x, True), (y, y, True), (x, y, False))):
        if len(a) == 0 or len(b) == 0:
            continue
        k = (g * (a.astype(np.longdouble) @ b.astype(np.longdouble).T) + np.longdouble(coef0)) ** int(degree)
        if sym:
            k = k[~np.eye(len(a), dtype=bool)]
        sums[i], absum[i] = float(k.sum()), float(np.abs(k).sum())
    return sums, absum


def poly_terms(m, n):
    """The number of terms of (S_xx, S_yy, S_xy)."""
    return np.array([m * (m - 1), n * (n - 1), m * n], dtype=np.float64)


def poly_bound(m, n, cols, degree, absum):
    """[3]: (T - 1 + cols + degree + 2) u sum|k| per sum (0 terms: 0)."""
    t = poly_terms(m, n)
    return np.where(t > 0, (t - 1 + cols + degree + 2) * U * np.asarray(absum), 0.0)


def sklearn_sums(x, y, degree=4, gamma=None, coef0=1.0):
    """[3] = (S_xx, S_yy, S_xy) from sklearn.metrics.pairwise.polynomial_kernel on the fp64-widened rows."""
    from sklearn.metrics.pairwise import polynomial_kernel
    x, y = np.asarray(x, dtype=np.float32).astype(np.float64), np.asarray(y, dtype=np.float32).astype(np.float64)
    g = 1.0 / x.shape[1] if gamma is None else gamma
    out = np.zeros(3)
    for i, (a, b, sym) in enumerate(((x, x, True), (y, y, True), (x, y, False))):
        if len(a) == 0 or len(b) == 0:
            continue
        k = polynomial_kernel(a, b, degree=degree, gamma=g, coef0=coef0)
        out[i] = k[~np.eye(len(a), dtype=bool)].sum() if sym else k.sum()
    return out


def mmd2(sums, m, n):
    """The unbiased MMD^2 from (S_xx, S_yy, S_xy)."""
    return sums[0] / (m * (m - 1)) + sums[1] / (n * (n - 1)) - 2.0 * sums[2] / (m * n)


# the record's kernel cases: (cols, m, n, degree); rows as mmd_case makes them
MMD_CASES = ((1, 63, 65, 4), (3, 64, 257, 2), (10, 257, 64, 4), (16, 65, 63, 1), (10, 2, 1, 4))


def mmd_case(cols, m, n, degree):
    """(x [m, cols], y [n, cols]) fp32: normalised observable-like rows, the generated side slightly shifted."""
    rs = np.random.RandomState(2000 + 101 * cols + 7 * m + n + degree)
    return (observable_rows(rs, max(m, 2), cols)[:m].astype(np.float32),
            (0.95 * observable_rows(rs, max(n, 2), cols)[:n] + 0.03).astype(np.float32))


# ------------------------------------------------------------------------------------------ fpd / kpd over experts
EXPERT_ROWS, EXPERT_COLS, EXPERT_E = 400, 10, 3


def expert_case():
    """(real, fake fp64 [400, 10], expert int32 [400]) for the end-to-end tests: expert 0 holds all rows but 7,
    expert 1 is empty and expert 2 holds 7 rows (<= cols: a rank-deficient covariance)."""
    rs = np.random.RandomState(3000)
    real = observable_rows(rs, EXPERT_ROWS, EXPERT_COLS)
    fake = 0.9 * observable_rows(rs, EXPERT_ROWS, EXPERT_COLS) + 0.02
    expert = np.zeros(EXPERT_ROWS, dtype=np.int32)
    expert[rs.permutation(EXPERT_ROWS)[:7]] = 2
    return real, fake, expert


def prefix_lengths(L, points):
    """n_j = floor(L (points + j) / (2 points - 1)), j = 0 .. points - 1."""
    return np.array([L * (points + j) // (2 * points - 1) for j in range(points)], dtype=np.int64)


def fpd_table(real, fake, points=10):
    """[points, 3] = (FD_j, n_j, n_j) of one aligned segment (rows in order), the eigh form on np.cov moments."""
    out = np.zeros((points, 3))
    for j, nj in enumerate(prefix_lengths(len(real), points)):
        _, ma, ca = moments(real[:nj])
        _, mb, cb = moments(fake[:nj])
        out[j] = (frechet_eigh(ma, ca, mb, cb)[0], nj, nj)
    return out


def kpd_table(real, fake, blocks=10, degree=4):
    """[blocks + 1, 5] = (S_xx, S_yy, S_xy, m, n) of one aligned segment, the whole segment last."""
    L = len(real)
    m = L // blocks
    parts = [(t * m, (t + 1) * m) for t in range(blocks)] + [(0, L)]
    out = np.zeros((blocks + 1, 5))
    for t, (lo, hi) in enumerate(parts):
        s, _ = poly_sums(real[lo:hi], fake[lo:hi], degree)
        out[t] = (*s, hi - lo, hi - lo)
    return out
