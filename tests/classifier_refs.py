"""Numpy restatement of the classifier two-sample test (include/expertsim_hip.h: es_rank_stats, es_logit_fit,
es_logit_scores; expertsim/train/classifier.py: c2st) and of the inputs of its record, shared by
tests/test_classifier_*.py and tests/golden/make_classifier_goldens.py.  scipy and scikit-learn are imported only by
that tool.

Bounds (derived, not measured; u = 2^-53; z~ = (1, z), n rows, `cols` columns, A_i = sum_c |theta_c z~_ic|):
* a score t_i = b + sum_c w_c z_ic, one chain of `cols` fused multiply-adds: (cols + 2) u A_i (Higham, Accuracy and
  Stability, ch. 3; the + 2 covers a non-fused evaluation and the final rounding);
* the gradient entry g_c = (1/n) sum_i r_i z~_ic + (l2/n) w_c, r_i = p_i - y_i: |r_i| <= 1, so the n products, their
  sum in any order and the division cost (n + 2) u max|z~|; r_i itself carries 8 u (exp to 2 ulp, one addition, one
  division, one product, doubled) and the error of t_i through dp/dt = p (1 - p): (cols + 2) u amp with
  amp = max(1, max_i p_i (1 - p_i) A_i) (amp = 1 unless scores are both large and the product of cancellation); the
  ridge term 3 u (l2/n) max|w|.  Together (n + cols + c) u amp max|z~| + 3 u (l2/n) max|w| with c = 12;
* the objective F = (1/n) sum_i loss_i + (l2/(2n)) |w|^2, |dloss/dt| <= 1: (n + 8) u mean(loss) +
  (cols + 2) u mean(A) + (cols + 4) u (l2/(2n)) |w|^2;
* a log-loss sum over m rows: (m + 8) u sum(loss) + (cols + 2) u sum(A).
Two independent evaluations (the device's and numpy's) differ by at most twice a bound.

Distance to the record.  With D = theta_dev - theta_rec and r = max_i |z~_i|_2 |D|_2, p (1 - p) changes by at most a
factor exp(|dt|) <= exp(r) along the segment between the two points, so the Hessian there is at least exp(-r) times
the record's and, F being convex,  lambda_min(H(theta_rec)) exp(-r) |D|_2 <= |g(theta_dev) - g(theta_rec)|_2
<= |g(theta_dev)|_2 + |g(theta_rec)|_2.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classifier_sklearn.npz")
U = 2.0 ** -53
GRAD_C = 12
L2 = 1.0
GTOL = 1e-9               # the gtol of the end-to-end cases


def load_golden():
    return np.load(GOLDEN)


# ------------------------------------------------------------------------------------------ rank statistics
RANK_KINDS = ("cont", "three", "equal", "zeros")
# (nu, nv): the lengths of the Wasserstein / moments tests, the totals 8191 / 8192 / 8193 around the LDS limit and one
# near 20000 (a global compare-exchange stride)
RANK_SIZES = ((1, 1), (2, 1), (63, 65), (64, 64), (257, 1000), (4096, 4095), (4096, 4096), (4097, 4096),
              (10000, 10001))


def rank_case(kind, nu, nv):
    """(u [nu], v [nv]) float64 of record case (kind, nu, nv)."""
    rs = np.random.RandomState(1000 + 17 * RANK_KINDS.index(kind) + nu + 3 * nv)
    if kind == "cont":
        return rs.randn(nu) + 0.3, rs.randn(nv)
    if kind == "three":                                        # tie runs far longer than a tile
        vals = np.array([-1.5, 0.25, 2.0])
        return vals[rs.randint(0, 3, nu)], vals[rs.randint(0, 3, nv)]
    if kind == "equal":
        return np.full(nu, 0.75), np.full(nv, 0.75)
    zeros = np.array([-0.0, 0.0, 1.0, -1.0])                    # -0.0 == +0.0: one run
    return zeros[rs.randint(0, 4, nu)], zeros[rs.randint(0, 4, nv)]


def rank_stats(u, v):
    """(nu, nv, U2, KS) as Python ints, es_rank_stats's definition in int64 numpy."""
    u, v = np.sort(np.asarray(u, dtype=np.float64) + 0.0), np.sort(np.asarray(v, dtype=np.float64) + 0.0)
    nu, nv = len(u), len(v)
    if nu == 0 or nv == 0:
        return nu, nv, 0, 0
    less = np.searchsorted(v, u, side="left").astype(np.int64)          # v_j < u_i
    leq = np.searchsorted(v, u, side="right").astype(np.int64)          # v_j <= u_i
    u2 = int((less + leq).sum())
    a = np.unique(np.concatenate([u, v]))
    cu = np.searchsorted(u, a, side="right").astype(np.int64)
    cv = np.searchsorted(v, a, side="right").astype(np.int64)
    return nu, nv, u2, int(np.abs(cu * nv - cv * nu).max())


# ------------------------------------------------------------------------------------------ logistic regression
def softplus(t):
    return np.maximum(t, 0.0) + np.log1p(np.exp(-np.abs(t)))


def design(real, fake):
    """(Z~ [n, cols + 1] float64 with the ones first, y [n]) of the real rows (label 1) then the generated ones."""
    z = np.concatenate([np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)])
    y = np.concatenate([np.ones(len(real)), np.zeros(len(fake))])
    return np.concatenate([np.ones((len(z), 1)), z], axis=1), y


def pq(t):
    e = np.exp(-np.abs(t))
    inv = 1.0 / (1.0 + e)
    return np.where(t >= 0, inv, e * inv), np.where(t >= 0, e * inv, inv)


def objective(theta, Z, y, l2=L2):
    """(F, g [P], H [P, P]) of the header's objective at theta, float64."""
    n = len(y)
    t = Z @ theta
    p, q = pq(t)
    loss = softplus(np.where(y > 0, -t, t))
    pen = np.concatenate([[0.0], theta[1:]])
    F = loss.sum() / n + 0.5 * l2 / n * float(pen @ pen)
    g = Z.T @ np.where(y > 0, -q, p) / n + l2 / n * pen
    H = (Z * (p * q)[:, None]).T @ Z / n + l2 / n * np.diag(np.concatenate([[0.0], np.ones(len(theta) - 1)]))
    return F, g, H


def fit(Z, y, l2=L2, gtol=1e-9, max_iter=50):
    """(theta, F, |g|_inf, moves, status): Newton steps from 0 with the header's safeguard, numpy float64."""
    theta = np.zeros(Z.shape[1])
    F, g, H = objective(theta, Z, y, l2)
    for it in range(max_iter + 1):
        if np.abs(g).max() <= gtol:
            return theta, F, np.abs(g).max(), it, 1
        if it == max_iter:
            break
        d = -np.linalg.solve(H, g)
        for j in range(8):
            Fn, gn, Hn = objective(theta + d / 2 ** j, Z, y, l2)
            if Fn <= F * (1 + (len(y) + 64) * 2 * U) if j == 0 else Fn < F:
                theta, F, g, H = theta + d / 2 ** j, Fn, gn, Hn
                break
        else:
            break
    return theta, F, np.abs(g).max(), it, 0


def amplitude(theta, Z):
    return np.abs(Z * theta[None, :]).sum(axis=1)


def score_bound(theta, Z):
    """[n]: the bound of one evaluation of every row's score."""
    return (Z.shape[1] + 1) * U * amplitude(theta, Z)


def grad_bound(theta, Z, l2=L2):
    """The bound of one evaluation of a gradient entry (module docstring)."""
    n, P = Z.shape
    A = amplitude(theta, Z)
    p, q = pq(Z @ theta)
    amp = max(1.0, float((p * q * A).max()))
    return (n + (P - 1) + GRAD_C) * U * amp * np.abs(Z).max() + 3 * U * l2 / n * np.abs(theta[1:]).max(initial=0.0)


def objective_bound(theta, Z, y, l2=L2):
    n, P = Z.shape
    t = Z @ theta
    loss = softplus(np.where(y > 0, -t, t))
    return ((n + 8) * U * loss.mean() + (P + 1) * U * amplitude(theta, Z).mean()
            + (P + 3) * U * 0.5 * l2 / n * float(theta[1:] @ theta[1:]))


def logloss_bound(theta, Z, loss):
    return (len(loss) + 8) * U * loss.sum() + (Z.shape[1] + 1) * U * amplitude(theta, Z).sum()


def distance_bound(theta_dev, theta_rec, Z, y, l2=L2):
    """(|D|_2, its bound, r) of the module docstring's inequality."""
    D = np.linalg.norm(theta_dev - theta_rec)
    r = np.linalg.norm(Z, axis=1).max() * D
    _, g_dev, _ = objective(theta_dev, Z, y, l2)
    _, g_rec, H = objective(theta_rec, Z, y, l2)
    lam = np.linalg.eigvalsh(H).min()
    return D, (np.linalg.norm(g_dev) + np.linalg.norm(g_rec)) * np.exp(r) / lam, r


def prior_score_slack(theta_rec, Z, y, Zheld, gtol=GTOL, l2=L2):
    """The most a held-out score of ANY fit that stopped with |g|_inf <= gtol can differ from the record's, from the
    reference alone: such a fit has |g|_2 <= sqrt(P) (gtol + 2 grad_bound), so by the inequality above
    |D|_2 <= (sqrt(P) (gtol + 2 grad_bound) + |g(theta_rec)|_2) exp(r) / lambda_min(H(theta_rec)) (r from that bound,
    one fixed-point step from exp(0): r stays below 1e-4 here and exp(r) < 1.0002 covers it), and a score moves by
    at most |D|_2 |z~|_2 plus the two evaluations' dot-product bounds."""
    _, g_rec, H = objective(theta_rec, Z, y, l2)
    P = Z.shape[1]
    lam = np.linalg.eigvalsh(H).min()
    D = (np.sqrt(P) * (gtol + 2 * grad_bound(theta_rec, Z, l2)) + np.linalg.norm(g_rec)) * 1.0002 / lam
    assert np.linalg.norm(Z, axis=1).max() * D < 1e-4
    return float((D * np.linalg.norm(Zheld, axis=1) + 2.0002 * score_bound(theta_rec, Zheld)).max())


def block_rows():
    return 256                                                  # ES_LOGIT_BLOCK_ROWS; the GPU test checks the library's


# name: (m, k, cols, dtype, separation in standard deviations along the first column, or None for a small shift)
FIT_CASES = {
    "c1": (257, 130, 1, "f8", None), "c3": (65, 63, 3, "f8", None), "c3_f4": (64, 64, 3, "f4", None),
    "c10": (300, 300, 10, "f8", None), "c10_f4": (2, 63, 10, "f4", None), "c77": (256, 256, 77, "f8", None),
    "c77_f4": (129, 127, 77, "f4", None), "c80": (260, 255, 80, "f8", None), "c80_f4": (200, 57, 80, "f4", None),
    "one_row": (1, 64, 3, "f8", None), "two_rows": (2, 2, 3, "f8", None),
    "blk_m1": (128, 127, 10, "f8", None), "blk_0": (128, 128, 10, "f8", None), "blk_p1": (129, 128, 10, "f8", None),
    "blk2_m1": (255, 256, 3, "f8", None), "blk2_p1": (256, 257, 3, "f8", None),
    "sep": (100, 100, 5, "f8", 12.0), "z_c1_f4": (130, 257, 1, "f4", None),
}


def fit_case(name):
    """(real [m, cols], fake [k, cols]) of record case `name`, in its dtype."""
    m, k, cols, dt, sep = FIT_CASES[name]
    rs = np.random.RandomState(2000 + sorted(FIT_CASES).index(name))
    real, fake = rs.randn(m, cols), rs.randn(k, cols)
    if sep is None:
        real += 0.4 * rs.randn(cols)[None, :]
        real *= 1.0 + 0.2 * rs.rand(cols)[None, :]
    else:
        real[:, 0] += sep
    dt = np.float32 if dt == "f4" else np.float64
    return real.astype(dt), fake.astype(dt)


# ------------------------------------------------------------------------------------------ c2st
def standardise(real, fake):
    """(real_z, fake_z): the pooled mean and population standard deviation of both tables; scale 0 where it is 0."""
    x = np.concatenate([real, fake]).astype(np.float64)
    mu, sd = x.mean(axis=0), x.std(axis=0)
    scale = np.where(sd > 0, 1.0 / np.where(sd > 0, sd, 1.0), 0.0)
    return (np.asarray(real, dtype=np.float64) - mu) * scale, (np.asarray(fake, dtype=np.float64) - mu) * scale


def expand(z, degree):
    if degree == 1:
        return z
    i, j = np.triu_indices(z.shape[1])
    return np.concatenate([z, z[:, i] * z[:, j]], axis=1)


def halves(L):
    """(train, held out) lengths of a segment of L positions."""
    return (L + 1) // 2, L // 2


def segments(expert, n_experts, N):
    """The row lists of c2st's segments: the joint one in the order given, then every expert's in batch order."""
    segs = [np.arange(N)]
    if expert is not None:
        segs += [np.flatnonzero(np.asarray(expert) == e) for e in range(n_experts)]
    return segs


# name: (N, cols, E, degree)
C2ST_CASES = {"e1_d1": (600, 4, 1, 1), "e1_d2": (600, 4, 1, 2), "e3_d1": (601, 3, 3, 1), "e3_d2": (601, 3, 3, 2)}


def c2st_case(name):
    """(real [N, cols], fake [N, cols], expert [N] or None, E, degree): Gaussian tables with a mean shift."""
    N, cols, E, degree = C2ST_CASES[name]
    rs = np.random.RandomState(3000 + sorted(C2ST_CASES).index(name))
    real = rs.randn(N, cols) * (1.0 + rs.rand(cols)) + 5.0 * rs.randn(cols)
    fake = real[rs.permutation(N)] * 1.1 + 0.5 + 0.3 * rs.randn(N, cols)
    expert = rs.randint(0, E, N).astype(np.int32) if E > 1 else None
    return real, fake, expert, E, degree


def c2st_features(name):
    real, fake, expert, E, degree = c2st_case(name)
    zr, zf = standardise(real, fake)
    return expand(zr, degree), expand(zf, degree), expert, E


def held_out(xr, xf, rows, theta):
    """What c2st reports for one segment from its feature rows (in segment order) and a theta: a dict of the four
    integers, the two hit counts, the two log-loss sums, the held-out scores and the least real-generated gap."""
    ntr, nte = halves(len(rows))
    tr, fr = xr[rows[ntr:]], xf[rows[ntr:]]
    Zr, Zf = design(tr, fr[:0])[0], design(fr, tr[:0])[0]
    sr, sf = Zr @ theta, Zf @ theta
    nu, nv, u2, ks = rank_stats(sr, sf)
    gap = np.abs(sr[:, None] - sf[None, :]).min() if nte else np.inf
    return {"rank": (nu, nv, u2, ks), "hits": (int((sr > 0).sum()), int((sf <= 0).sum())),
            "loss": (softplus(-sr).sum(), softplus(sf).sum()), "r_scores": sr, "f_scores": sf, "gap": gap,
            "Zr": Zr, "Zf": Zf}


def train_design(xr, xf, rows):
    ntr, _ = halves(len(rows))
    return design(xr[rows[:ntr]], xf[rows[:ntr]])
