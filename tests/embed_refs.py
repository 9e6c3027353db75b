"""fp64 numpy restatement of es_pca_project, es_tsne_affinities, es_tsne_gradient and es_tsne_run
(csrc/embedding.hip) as include/expertsim_hip.h defines them, and the error bounds of tests/test_embedding_gpu.py.

Written from the header, not from the kernels: dense P, dense pair sums in numpy's own order.  Only the quantities
the header DEFINES in fp32 (d_ij, dmin) and the fixed-order fp64 moments of the PCA are reproduced bit for bit.

Bounds (U = 2^-53, u = 2^-24).

PCA residual.  One Jacobi rotation replaces two rows and two columns by c a -/+ s b with |c|, |s| <= 1 known to
4 U: each new entry carries at most 4 U (|a| + |b|), at most 8 U lambda_1 in norm per touched row.  The cols / 2
disjoint rotations of a round touch every row once, a sweep is cols - 1 such rounds, so a sweep perturbs the matrix
by at most 8 (cols - 1) U lambda_1; the sweeps converge quadratically and the kernel stops at the first one without
a rotation: 8 sweeps carry weight (cols <= 64).  The entries left behind by the skip rule (|a_pq| <= 2^-56
sqrt(a_pp a_qq)) add cols 2^-56 lambda_1, and evaluating the residual in fp64 cols U lambda_1.  Together
|cov v - lambda v| <= (64 + 2) cols U lambda_1 < PCA_C cols 2^-52 lambda_1 with PCA_C = 40.  Components against
the restatement: Davis-Kahan, sin(angle) <= residual / gap, times 4 for the two-sided gap and both computations.

Affinity entropy.  S and W are sums of rows - 1 non-negative terms whose exponent -beta dd is known to
|beta dd| U; a term above 2^-64 of the largest has |beta dd| < 45, the others change nothing at the 1e-5 level.
Each sum is within (rows + 45 + 8) U relative whatever the order, the log and the quotient add 4 U, and
H = log S + beta W / S moves by at most that times (1 + beta W / S) <= 1 + log(rows) + |log perplexity|:
H_SLACK(rows) = 64 (rows + 64) U (1 + log rows), far below the 1e-5 of the search.

Pair pass (gradient, Z, KL): see grad_bounds().
"""
import os

import numpy as np

U = 2.0 ** -53
u32 = 2.0 ** -24
EPS = np.finfo(np.float64).eps
SPLIT_MIN, CHUNKS = 256, 16        # ES_PREP_SPLIT_MIN, ES_PREP_CHUNKS
TILE = 32                          # ES_TSNE_TILE
MAX_SPLITS = 16                    # ES_TSNE_MAX_SPLITS
PCA_C = 40.0
LOG2E = 1.4426950408889634


def golden():
    here = os.path.dirname(os.path.abspath(__file__))
    return np.load(os.path.join(here, "golden", "tsne_sklearn.npz"))


# ------------------------------------------------------------------------------------------ PCA
def _chunked(terms):
    """Sum of terms [rows, ...] over rows in es_group_diversity's order (fp64)."""
    n = terms.shape[0]
    L = n if n <= SPLIT_MIN else -(-n // CHUNKS)
    total = np.zeros(terms.shape[1:])
    for k in range(CHUNKS):
        part = np.zeros(terms.shape[1:])
        for r in range(min(k * L, n), min((k + 1) * L, n)):
            part = part + terms[r]
        total = total + part
    return total


def moments_ref(x):
    """(mean [C], cov [C, C]) of the header, bit for bit."""
    x = np.asarray(x).astype(np.float64)
    n = x.shape[0]
    mean = _chunked(x) / np.float64(n)
    d = x - mean
    cov = _chunked(d[:, :, None] * d[:, None, :]) / (np.float64(n) - 1.0)
    return mean, cov


def sign_rule(components):
    """svd_flip(u_based_decision=False): the entry of largest magnitude of each row positive, first index wins."""
    c = np.array(components, dtype=np.float64)
    for m in range(c.shape[0]):
        if c[m, np.argmax(np.abs(c[m]))] < 0:
            c[m] = -c[m]
    return c


def pca_ref(x, k):
    mean, cov = moments_ref(x)
    lam, vec = np.linalg.eigh(cov)
    order = np.argsort(-lam, kind="stable")[:k]
    comp = sign_rule(vec[:, order].T)
    trace = float(np.sum(np.diag(cov)))
    scores = (np.asarray(x, dtype=np.float64) - mean) @ comp.T
    return {"mean": mean, "cov": cov, "components": comp, "explained_variance": lam[order],
            "explained_variance_ratio": lam[order] / trace if trace > 0 else np.zeros(k), "scores": scores,
            "eigenvalues": np.sort(lam)[::-1]}


def pca_residual_bound(cols, lam1):
    return PCA_C * cols * 2.0 ** -52 * lam1


# ------------------------------------------------------------------------------------------ affinities
def dist32(x):
    """d_ij of the header, float32 numpy ops: bit for bit."""
    x = np.asarray(x, dtype=np.float32)
    acc = np.zeros((x.shape[0], x.shape[0]), dtype=np.float32)
    for c in range(x.shape[1]):
        t = x[:, None, c] - x[None, :, c]
        acc = acc + t * t
    return acc


def row_min(d):
    m = np.array(d, dtype=np.float32)
    np.fill_diagonal(m, np.inf)
    return m.min(axis=1)


def entropy(beta, dd):
    """(H, log S) of one row at beta; dd = d_ij - dmin_i over j != i (fp64)."""
    e = np.exp(-beta * dd)
    S = e.sum()
    return float(np.log(S) + beta * ((dd * e).sum() / S)), float(np.log(S))


def h_slack(rows):
    return 64.0 * (rows + 64) * U * (1.0 + np.log(rows))


def affinities_ref(x, perplexity):
    """beta, log_s (fp64), dmin (fp32), steps (int32), converged (bool) per row, and d (fp32 [N, N])."""
    d = dist32(x)
    n = d.shape[0]
    dmin = row_min(d)
    target = np.log(perplexity)
    beta_out, ls_out, steps, conv = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    for i in range(n):
        dd = np.delete(d[i].astype(np.float64) - np.float64(dmin[i]), i)
        beta, lo, hi = 1.0, -np.inf, np.inf
        for it in range(100):
            H, lS = entropy(beta, dd)
            beta_out[i], ls_out[i], steps[i] = beta, lS, it + 1
            diff = H - target
            if abs(diff) <= 1e-5:
                conv[i] = True
                break
            if diff > 0:
                lo = beta
                beta = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
            else:
                hi = beta
                beta = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
    return {"beta": beta_out, "log_s": ls_out, "dmin": dmin, "steps": steps, "converged": conv, "d": d}


def conditional_P(beta, log_s, dmin, d):
    """p_{j|i} [N, N] fp64 (zero diagonal) from the per-row scalars and the fp32 d."""
    dd = d.astype(np.float64) - dmin.astype(np.float64)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):      # the diagonal (dd < 0) is zeroed below
        P = np.exp(-beta[:, None] * dd - log_s[:, None])
    np.fill_diagonal(P, 0.0)
    return P


def joint_P(beta, log_s, dmin, d):
    C = conditional_P(beta, log_s, dmin, d)
    return (C + C.T) / (2.0 * d.shape[0])


# ------------------------------------------------------------------------------------------ gradient, KL
def gradient_ref(P, y, a):
    """(g [N, 2], Z, KL) of the header, to the letter (the clamps included), fp64."""
    y = np.asarray(y).astype(np.float64)
    dy = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (dy ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    q = np.maximum(w / Z, EPS)
    g = 4.0 * (((a * P - q) * w)[:, :, None] * dy).sum(1)
    off = ~np.eye(len(y), dtype=bool)
    KL = float((P[off] * np.log(np.maximum(P[off], EPS) / q[off])).sum())
    return g, float(Z), KL


def grad_bounds(P, y, a, beta, log_s, dmin, d):
    """Bounds of |g_dev - g_ref| [N, 2], |Z_dev - Z_ref| and |KL_dev - KL_ref| for the fp32 pair pass.

    One pair term, in units of u = 2^-24 (first order; GUARD covers the second):
      exponent  arg = -b dd - l with b = fl32(beta log2 e) (1), dd = d - dmin (1), the fused multiply-add (1) on
                |b dd| and l = fl32(..) (1) plus the same fma rounding on |l|: |delta arg| <= 3 u E,
                E = |b dd| + |l|; exp2 turns it into 3 ln2 E <= 2.1 E relative and adds 1 (v_exp_f32), the sum of
                the two conditionals 1 more: delta p <= (2 + 2.1 E) u p, E the larger of the pair's two exponents.
      w         dy0, dy1 (1 each, twice through the squares -> at most 2 on 1 + |dy|^2), the two fmas (2),
                v_rcp_f32 (1): 5, taken as 6.
      A term    p w dy: delta p + 6 (w) + 1 (p w) + 1 (dy)          k_A = 10 + 2.1 E
      R term    w w dy: 12 + 1 + 1                                  k_R = 14
      Zr term   w                                                   k_Z = 6
      K term    p (log p~ - log w), L = log p~ - log w: delta p acts on the factor (|L|) and through log p (1);
                logf within 2 ulp on |log p~| and |log w|; the difference 1 on |L|; the product 1 on |L|:
                (2 + 2.1 E)(|L| + 1) + 2 (|log p~| + |log w|) + 2 |L|, all times p.
    The fp32 chain along a tile adds T - 1 < T = ES_TSNE_TILE roundings on the running sum, at most the sum of the
    absolute terms each.  So per row  (k + T + 2.1 A_i) u sum_j |term_ij|, with A_i the |term|-weighted mean of E
    -- evaluated below pair by pair, which is the same number.  The fp64 tail (tile, split and row sums: at most
    N / T + 16 + N / 1024 + 10 additions) adds (N / T + 64) U on the same absolute sums.
    g = 4 (a A - R / Z):  delta g <= 4 (a dA + dR / Z + |R| dZ / Z^2).  Where the clamp of q binds the split form
    differs by 4 sum_j max(0, eps - w / Z) w |dy| (header).  exp2 flushes below 2^-126: absolute 2^-120 N a.
    KL = sum K + log Z sum P:  dK + |log Z| dP + P dZ / Z, plus N^2 eps 2^-20 for pairs whose p straddles the clamp.
    """
    n = len(y)
    T = float(TILE)
    GUARD = 1.0 + 1e-3
    tail = (n / T + 64.0) * U
    y = np.asarray(y).astype(np.float64)
    dy = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (dy ** 2).sum(-1))
    np.fill_diagonal(w, 0.0)
    Z = w.sum()
    dd = d.astype(np.float64) - dmin.astype(np.float64)[:, None]
    Ei = np.abs(beta[:, None] * LOG2E * dd) + np.abs(log_s * LOG2E + np.log2(2.0 * n))[:, None]
    E = np.maximum(Ei, Ei.T)
    ady = np.abs(dy)
    tA = (P * w)[:, :, None] * ady
    tR = (w * w)[:, :, None] * ady
    dA = (((10.0 + T + 2.1 * E) * u32 + tail)[:, :, None] * tA).sum(1)
    dR = ((14.0 + T) * u32 + tail) * tR.sum(1)
    dZ = ((6.0 + T) * u32 + tail) * Z
    R = ((w * w)[:, :, None] * dy).sum(1)
    clamp = 4.0 * ((np.maximum(0.0, EPS - w / Z) * w)[:, :, None] * ady).sum(1)
    g_bound = GUARD * 4.0 * (a * dA + dR / Z + np.abs(R) * dZ / Z ** 2) + clamp + 2.0 ** -120 * n * a
    off = ~np.eye(n, dtype=bool)
    p, wo, Eo = P[off], w[off], E[off]
    lp = np.log(np.maximum(p, EPS))
    lw = np.log(wo)
    L = lp - lw
    dK = (p * (((2.0 + 2.1 * Eo) * (np.abs(L) + 1.0) + 2.0 * (np.abs(lp) + np.abs(lw)) + 2.0 * np.abs(L)
                + T * np.abs(L)) * u32 + tail * np.abs(L))).sum()
    dP = (p * ((2.0 + 2.1 * Eo + T) * u32 + tail)).sum()
    kl_bound = GUARD * (dK + abs(np.log(Z)) * dP + p.sum() * dZ / Z) + n * n * EPS * 2.0 ** -20 + 2.0 ** -100
    return g_bound, GUARD * dZ, kl_bound


def gradient_rows_ref(idx, x, y, a, beta, log_s, dmin):
    """gradient_ref and the g / Z bounds of grad_bounds for the rows idx only, in [len(idx), N] arrays (a large N
    without the dense N x N x 2 arrays): (g [m, 2], Z, g_bound [m, 2], Z_bound).  Same terms as grad_bounds."""
    x = np.asarray(x, dtype=np.float32)
    n, T, GUARD = len(x), float(TILE), 1.0 + 1e-3
    tail = (n / T + 64.0) * U
    y = np.asarray(y).astype(np.float64)
    Z = 0.0
    for r0 in range(0, n, 512):                               # Z over all ordered pairs, in row blocks
        dyb = y[r0:r0 + 512, None, :] - y[None, :, :]
        wb = 1.0 / (1.0 + (dyb ** 2).sum(-1))
        wb[np.arange(len(wb)), np.arange(r0, r0 + len(wb))] = 0.0
        Z += wb.sum()
    d = np.zeros((len(idx), n), dtype=np.float32)             # d_ij of the header for the rows idx (== d_ji)
    for c in range(x.shape[1]):
        t = x[idx, None, c] - x[None, :, c]
        d = d + t * t
    d64, dm = d.astype(np.float64), dmin.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        Cij = np.exp(-beta[idx, None] * (d64 - dm[idx, None]) - log_s[idx, None])      # p_{j|i}
        Cji = np.exp(-beta[None, :] * (d64 - dm[None, :]) - log_s[None, :])            # p_{i|j}
    P = (Cij + Cji) / (2.0 * n)
    self_ = np.asarray(idx)[:, None] == np.arange(n)[None, :]
    P[self_] = 0.0
    dy = y[idx, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (dy ** 2).sum(-1))
    w[self_] = 0.0
    q = np.maximum(w / Z, EPS)
    g = 4.0 * (((a * P - q) * w)[:, :, None] * dy).sum(1)
    l2 = np.abs(log_s * LOG2E + np.log2(2.0 * n))
    E = np.maximum(np.abs(beta[idx, None] * LOG2E * (d64 - dm[idx, None])) + l2[idx, None],
                   np.abs(beta[None, :] * LOG2E * (d64 - dm[None, :])) + l2[None, :])
    ady = np.abs(dy)
    dA = ((((10.0 + T + 2.1 * E) * u32 + tail) * P * w)[:, :, None] * ady).sum(1)
    dR = ((14.0 + T) * u32 + tail) * ((w * w)[:, :, None] * ady).sum(1)
    dZ = ((6.0 + T) * u32 + tail) * Z
    R = ((w * w)[:, :, None] * dy).sum(1)
    clamp = 4.0 * ((np.maximum(0.0, EPS - w / Z) * w)[:, :, None] * ady).sum(1)
    g_bound = GUARD * 4.0 * (a * dA + dR / Z + np.abs(R) * dZ / Z ** 2) + clamp + 2.0 ** -120 * n * a
    return g, float(Z), g_bound, GUARD * dZ


# ------------------------------------------------------------------------------------------ update, schedule
def auto_learning_rate(rows, exaggeration=12.0):
    return max(rows / exaggeration / 4.0, 50.0)


def run_ref(P, y0, n_iter, iter0=0, upd=None, gains=None, exaggeration=12.0, exaggeration_iters=250, momentum0=0.5,
            momentum1=0.8, learning_rate=None, min_gain=0.01, check_every=50, round_grad=False):
    """es_tsne_run of the header on the dense P: (y fp32, upd, gains, log {row: (KL, |g|)}).  round_grad rounds
    every gradient to fp32 first (the yardstick of the trajectory test)."""
    y = np.array(y0, dtype=np.float32)
    n = len(y)
    upd = np.zeros((n, 2)) if upd is None else np.array(upd, dtype=np.float64)
    gains = np.ones((n, 2)) if gains is None else np.array(gains, dtype=np.float64)
    lr = auto_learning_rate(n, exaggeration) if learning_rate is None else float(learning_rate)
    log = {}
    last = iter0 + n_iter - 1
    for t in range(iter0, last + 1):
        early = t < exaggeration_iters
        a, mu = (exaggeration, momentum0) if early else (1.0, momentum1)
        g, _, KL = gradient_ref(P, y, a)
        if round_grad:
            g = g.astype(np.float32).astype(np.float64)
        if (t + 1) % check_every == 0 or t == last:
            log[t // check_every] = (KL, float(np.sqrt((g * g).sum())))
        inc = upd * g < 0.0
        gains = np.where(inc, gains + 0.2, gains * 0.8)
        gains = np.maximum(gains, min_gain)
        upd = mu * upd - lr * (g * gains)
        y = (y.astype(np.float64) + upd).astype(np.float32)
    return y, upd, gains, log


def knn_purity(y, labels, k=10):
    """Mean fraction of a point's k nearest neighbours (itself excluded) that carry its label."""
    y = np.asarray(y, dtype=np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())
