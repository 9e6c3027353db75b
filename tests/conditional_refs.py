"""numpy restatements behind tests/test_conditional_*.py: the quantile rule and the bin rule of
csrc/quantile_rule.h, the stable grouping of es_bin_dispatch and the `profile` of expertsim/train/conditional.py, the
seeded fixture of the record tests/golden/conditional_numpy.npz, and the error bounds of the comparisons.  The
per-bin distances come from scipy.stats.wasserstein_distance and ks_2samp.

Bounds (u = 2^-53, B bins, n_b rows a side in bin b, all derived here, none fitted to a result):

* quantiles, bins, perm, offs, counts: EQUAL.  The device sorts the same doubles and applies the rule of
  `quantile` operation for operation; the bin of a value and the stable order are integers.
* per-bin W1: |got - ref| <= 2 (nu + nv) 2^-52 ref, as tests/test_wasserstein_gpu.py derives it (the same
  non-negative terms summed in two orders).
* a count-weighted mean sum_b n_b x_b / sum_b n_b of B non-negative terms: B products, B - 1 additions and one
  division, every one rounded once and no cancellation: (B + 2) u relative, on either side of a comparison.
  - cond_ws_<o>: e_W = max_b 4 n_b 2^-52 from the terms, so  rel <= e_W + 2 (B + 2) u.
  - cond_ks_<o>: the device's KS / (nu nv) is one rounded quotient of exact integers; scipy's statistic is the
    difference of two rounded quotients that are at most 1, i.e. within 2 u ABSOLUTE of the exact value, and the
    device's quotient within u of it:  abs <= 3 u + 2 (B + 2) u value.
  - cond_bias_<o>: |median_gen - median_real| / s_o on EXACT quantiles: one subtraction (u relative), s_o = (q84 -
    q16) / 2 one subtraction (halving is exact), one division: 3 u per term on either side:
    rel <= (6 + 2 (B + 2)) u.
  - cond_width_<o>: w = (q84 - q16) / 2 is rounded once, so w_gen - w_real cancels: its error is u (w_gen + w_real)
    ABSOLUTE plus u relative, then s_o and the division:
    abs <= 2 [sum_b n_b u (w_gen,b + w_real,b) / s_o / sum_b n_b] + (6 + 2 (B + 2)) u value.
  - cond_ws: the mean over `cols` values cond_ws_<o> / s_o: s_o (u), the division (u), cols - 1 additions and one
    division:  rel <= e_W + 2 (B + 2) u + 2 (cols + 2) u.
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conditional_numpy.npz")
U = 2.0 ** -53
PROBS = (0.16, 0.5, 0.84)
STATS = ("ws", "bias", "width", "ks")

# the fixture: N rows, n_bins bins, three columns
N, BINS, SEED = 600, 4, 20240611
NAMES = ("lin", "abs", "int")


def load_golden():
    return np.load(GOLDEN)


def golden_tables(rec, case) -> dict:
    """The record's tables of `case` ("redraw", "shuffled", "experts") in the shape `profile` returns them."""
    t = {k[len(case) + 1:]: rec[k] for k in rec.files if k.startswith(case + "_")}
    t["scalars"] = {str(k): float(v) for k, v in zip(t.pop("keys"), t.pop("values"))}
    t["width_sum"] = dict(zip(NAMES, t["width_sum"]))
    return t


# ------------------------------------------------------------------------------------------ the two rules
def canon(x):
    """-0.0 as +0.0 (the device fetches it so); every other double unchanged."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x == 0.0, 0.0, x)


def quantile(x, p) -> float:
    """numpy's default rule written out on the sorted doubles, every operation rounded on its own (numpy float64
    scalars never fuse).  NaN for an empty x."""
    x = np.sort(canon(x).ravel())
    n = x.size
    if n == 0:
        return float("nan")
    h = np.float64(p) * np.float64(n - 1)
    lo = int(np.floor(h))
    g = h - np.float64(lo)
    hi = min(lo + 1, n - 1)
    a, b = x[lo], x[hi]
    d = b - a
    return float(b - d * (np.float64(1.0) - g)) if g >= 0.5 else float(a + d * g)


def quantiles(x, probs) -> np.ndarray:
    return np.array([quantile(x, p) for p in probs], dtype=np.float64)


def bin_of(edges, x) -> np.ndarray:
    """The number of edges strictly below each x, by counting (np.searchsorted(edges, x, side="left"))."""
    edges = np.asarray(edges, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    return (edges[None, :] < x[:, None]).sum(axis=1).astype(np.int32)


def classes(bins, n_bins, expert=None, n_experts=1) -> np.ndarray:
    if expert is None:
        return np.asarray(bins, dtype=np.int64)
    return np.clip(np.asarray(expert, dtype=np.int64), 0, n_experts - 1) * n_bins + np.asarray(bins, dtype=np.int64)


def grouping(cls, n_classes):
    """(perm, offs): the rows grouped by class, each group in ascending row order; offs[n_classes] = rows."""
    perm = np.argsort(cls, kind="stable").astype(np.int32)
    offs = np.concatenate([[0], np.cumsum(np.bincount(cls, minlength=n_classes))]).astype(np.int32)
    return perm, offs


def bin_edges(by, n_bins) -> np.ndarray:
    by = np.asarray(by, dtype=np.float64)
    return np.array([quantile(by, k / n_bins) for k in range(1, n_bins)], dtype=np.float64)


# ------------------------------------------------------------------------------------------ profile
def weighted_mean(n, x) -> float:
    num, den = 0.0, 0
    for nb, xb in zip(n, x):
        if nb > 0:
            num += float(nb) * float(xb)
            den += int(nb)
    return num / den if den else float("nan")


def profile(real, fake, by, n_bins, expert=None, n_experts=1, probs=PROBS, names=None) -> dict:
    """The tables and the scalars of expertsim.train.conditional.profile with numpy and scipy: {"edges", "bin",
    "count" [S, B], "q_real" / "q_gen" [S, B, cols, Q], "mean_*" / "std_*" [S, B, cols], "ws" / "ks" [S, B, cols],
    "scale" [cols], "scalars": {key: value}}."""
    from scipy.stats import ks_2samp, wasserstein_distance
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    by = np.asarray(by, dtype=np.float64)
    rows, cols = real.shape
    names = tuple(names) if names is not None else tuple(f"c{o}" for o in range(cols))
    edges = bin_edges(by, n_bins)
    b = bin_of(edges, by)
    S = 1 + (n_experts if expert is not None else 0)
    e = np.clip(np.asarray(expert, dtype=np.int64), 0, n_experts - 1) if expert is not None else None
    Q = len(probs)
    t = {"edges": edges, "bin": b, "count": np.zeros((S, n_bins), dtype=np.int64),
         "q_real": np.full((S, n_bins, cols, Q), np.nan), "q_gen": np.full((S, n_bins, cols, Q), np.nan),
         "mean_real": np.full((S, n_bins, cols), np.nan), "mean_gen": np.full((S, n_bins, cols), np.nan),
         "std_real": np.full((S, n_bins, cols), np.nan), "std_gen": np.full((S, n_bins, cols), np.nan),
         "ws": np.zeros((S, n_bins, cols)), "ks": np.zeros((S, n_bins, cols))}
    for s in range(S):
        for k in range(n_bins):
            m = (b == k) if s == 0 else ((b == k) & (e == s - 1))
            n = int(m.sum())
            t["count"][s, k] = n
            if n == 0:
                continue
            r, f = real[m], fake[m]
            t["mean_real"][s, k], t["mean_gen"][s, k] = r.mean(axis=0), f.mean(axis=0)
            if n > 1:
                t["std_real"][s, k], t["std_gen"][s, k] = r.std(axis=0, ddof=1), f.std(axis=0, ddof=1)
            for c in range(cols):
                t["q_real"][s, k, c], t["q_gen"][s, k, c] = quantiles(r[:, c], probs), quantiles(f[:, c], probs)
                t["ws"][s, k, c] = wasserstein_distance(r[:, c], f[:, c])
                t["ks"][s, k, c] = ks_2samp(r[:, c], f[:, c]).statistic
    i16, i50, i84 = (list(probs).index(p) for p in PROBS)
    q_all = np.array([quantiles(real[:, c], probs) for c in range(cols)])
    w_all = (q_all[:, i84] - q_all[:, i16]) / 2.0
    t["scale"] = np.where(w_all == 0, 1.0, w_all)
    sc, wsum = {}, {}
    n0 = t["count"][0]
    for c, o in enumerate(names):
        s_o = t["scale"][c]
        bias = [abs(t["q_gen"][0, k, c, i50] - t["q_real"][0, k, c, i50]) / s_o if n0[k] else 0.0
                for k in range(n_bins)]
        w_r = [(t["q_real"][0, k, c, i84] - t["q_real"][0, k, c, i16]) / 2.0 if n0[k] else 0.0 for k in range(n_bins)]
        w_g = [(t["q_gen"][0, k, c, i84] - t["q_gen"][0, k, c, i16]) / 2.0 if n0[k] else 0.0 for k in range(n_bins)]
        width = [abs(g - r) / s_o for g, r in zip(w_g, w_r)]
        sc[f"cond_ws_{o}"] = weighted_mean(n0, t["ws"][0, :, c])
        sc[f"cond_bias_{o}"] = weighted_mean(n0, bias)
        sc[f"cond_width_{o}"] = weighted_mean(n0, width)
        sc[f"cond_ks_{o}"] = weighted_mean(n0, t["ks"][0, :, c])
        wsum[o] = weighted_mean(n0, [(g + r) / s_o for g, r in zip(w_g, w_r)])      # for the width bound
    sc["cond_ws"] = sum(sc[f"cond_ws_{o}"] / t["scale"][c] for c, o in enumerate(names)) / cols
    for x in range(S - 1):
        for c, o in enumerate(names):
            sc[f"cond_ws_{o}_{x}"] = weighted_mean(t["count"][1 + x], t["ws"][1 + x, :, c])
        sc[f"cond_ws_{x}"] = sum(sc[f"cond_ws_{o}_{x}"] / t["scale"][c] for c, o in enumerate(names)) / cols
    t["scalars"] = sc
    t["width_sum"] = wsum
    return t


def bound(kind, ref, tables, name=None) -> float:
    """The absolute bound on |got - ref| of a scalar of `kind` "total" (cond_ws, cond_ws_<e>), "ws", "ks", "bias" or
    "width" (see the module docstring); ref is the reference value, tables the reference tables of `profile`, name
    the observable (for "width")."""
    B, cols = tables["count"].shape[1], tables["ws"].shape[2]
    e_w = 4.0 * float(tables["count"].max()) * 2.0 ** -52
    mean_u = 2 * (B + 2) * U
    if not np.isfinite(ref):
        return 0.0
    if kind == "total":
        return (e_w + mean_u + 2 * (cols + 2) * U) * abs(ref)
    if kind == "ws":
        return (e_w + mean_u) * abs(ref)
    if kind == "ks":
        return 3 * U + mean_u * abs(ref)
    if kind == "bias":
        return (6 * U + mean_u) * abs(ref)
    if kind == "width":
        return 2 * U * tables["width_sum"][name] + (6 * U + mean_u) * abs(ref)
    raise KeyError(kind)


def scalar_kinds(names, n_experts=0) -> dict:
    """{key: (kind, observable name or None)} of every scalar of `profile`."""
    out = {"cond_ws": ("total", None)}
    for o in names:
        out.update({f"cond_{s}_{o}": (s, o) for s in STATS})
    for e in range(n_experts):
        out[f"cond_ws_{e}"] = ("total", None)
        out.update({f"cond_ws_{o}_{e}": ("ws", o) for o in names})
    return out


def check_scalars(got, tables, names, n_experts=0, what=""):
    """Asserts every scalar of got against tables["scalars"] within its bound (NaN must meet NaN); returns the worst
    error / bound."""
    ref, worst = tables["scalars"], 0.0
    kinds = scalar_kinds(names, n_experts)
    assert set(kinds) == set(ref) and set(kinds) <= set(got), (what, sorted(set(kinds) ^ set(ref)))
    for key, (kind, o) in kinds.items():
        g, r = float(got[key]), float(ref[key])
        if np.isnan(r):
            assert np.isnan(g), (what, key, g)
            continue
        bd = bound(kind, r, tables, o)
        err = abs(g - r)
        print(f"{what} {key}: got {g!r} ref {r!r} err {err:.3e} bound {bd:.3e}")
        assert err <= bd, (what, key, g, r, err, bd)
        if err > 0:
            worst = max(worst, err / bd)
    return worst


# ------------------------------------------------------------------------------------------ the fixture
def fixture(seed=SEED, n=N):
    """(by [N], real [N, 3], redraw [N, 3], shuffled [N, 3], expert [N]): column 0 = 3 by + noise, column 1 = |by| +
    noise, column 2 integer-valued and independent of by.  `redraw` is an independent draw from the same conditional
    law, `shuffled` the real rows permuted across the conditions: its marginals are the real ones exactly.  expert
    takes the values 0 and 2 of three experts (expert 1 owns no row)."""
    rng = np.random.default_rng(seed)
    by = rng.normal(0.0, 1.0, n)

    def draw():
        return np.stack([3.0 * by + rng.normal(0.0, 0.5, n), np.abs(by) + rng.normal(0.0, 0.3, n),
                         rng.integers(0, 6, n).astype(np.float64)], axis=1)

    real, redraw = draw(), draw()
    shuffled = real[rng.permutation(n)]
    expert = np.where(rng.random(n) < 0.4, 0, 2).astype(np.int32)
    return by, real, redraw, shuffled, expert
