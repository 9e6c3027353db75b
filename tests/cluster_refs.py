"""Host restatements for the clustering tests: scikit-learn's Lloyd loop, the k-means++ of
include/expertsim_hip.h and the router-agreement numbers, in plain numpy.

`lloyd` restates ``sklearn.cluster._kmeans._kmeans_single_lloyd`` on fp64 input -- the mean-centring, the
tolerance, both stopping rules, ``_relocate_empty_clusters_dense`` and the closing E-step -- with the distance as
the sum of squared differences.  tests/test_cluster_cpu.py pins it to scikit-learn's own results in
tests/golden/kmeans_sklearn.npz (equal labels and n_iter); the GPU tests use it at shapes the golden does not
hold.  `plusplus` restates es_kmeans_plusplus to the letter except for the summation order inside a distance
and a potential, which the golden's asserted gaps make immaterial.
"""
from __future__ import annotations

import itertools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmeans_sklearn.npz")
CASES = ("proton", "proton_empty", "neutron")


def sq_dist(X, centres):
    """[rows, K] sums of squared differences, fp64."""
    X = np.asarray(X, dtype=np.float64)
    return np.stack([((X - c[None, :]) ** 2).sum(axis=1) for c in np.asarray(centres, dtype=np.float64)], axis=1)


def lloyd(X, init, tol=1e-4, max_iter=300, centre=True, trace=None):
    """(labels int64 [rows], centres fp64 [K, cols], inertia, n_iter).  trace (a dict) receives per-iteration
    lists: "gap" (the smallest relative gap between a row's nearest and second-nearest centre), "margin"
    (|shift - threshold| / threshold) and "relocated" (empty clusters refilled)."""
    X = np.asarray(X, dtype=np.float64)
    mean = X.mean(axis=0) if centre else np.zeros(X.shape[1])
    Xc = X - mean
    centres = np.asarray(init, dtype=np.float64) - mean
    K = centres.shape[0]
    threshold = np.mean(np.var(Xc, axis=0)) * tol
    labels_old = np.full(X.shape[0], -1, dtype=np.int64)
    strict = False
    if trace is not None:
        trace.update(gap=[], margin=[], relocated=[], threshold=threshold)
    for i in range(max_iter):
        d = sq_dist(Xc, centres)
        labels = d.argmin(axis=1)                       # the first of equal minima: the lowest centre
        if trace is not None and K > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            trace["gap"].append(float(((two[:, 1] - two[:, 0]) / np.maximum(two[:, 1], 1e-300)).min()))
        new = np.zeros_like(centres)
        np.add.at(new, labels, Xc)
        counts = np.bincount(labels, minlength=K).astype(np.float64)
        empty = np.flatnonzero(counts == 0)
        if empty.size:
            dist = d[np.arange(X.shape[0]), labels]
            far = np.lexsort((np.arange(X.shape[0]), -dist))[:empty.size]   # descending dist, the lower row first
            for k, r in zip(empty, far):
                new[labels[r]] -= Xc[r]
                counts[labels[r]] -= 1
                new[k] = Xc[r]
                counts[k] = 1
        has = counts > 0
        new[has] *= (1.0 / counts[has])[:, None]
        shift = float(((new - centres) ** 2).sum())
        centres = new
        if trace is not None:
            trace["margin"].append(abs(shift - threshold) / threshold if threshold > 0 else np.inf)
            trace["relocated"].append(int(empty.size))
        if np.array_equal(labels, labels_old):
            strict = True
            break
        if shift <= threshold:
            break
        labels_old = labels
    if not strict:
        labels = sq_dist(Xc, centres).argmin(axis=1)
    inertia = float(((Xc - centres[labels]) ** 2).sum())
    return labels, centres + mean, inertia, i + 1


def trials(K):
    return 2 + int(np.log(K))


def prefix_sums(v):
    """cum of es_kmeans_plusplus: 1024 segments of ceil(rows / 1024) rows, cum[i] = off_t + local_i."""
    v = np.asarray(v, dtype=np.float64)
    rows = v.shape[0]
    Ls = -(-rows // 1024)
    cum = np.empty(rows)
    off = 0.0
    for lo in range(0, rows, Ls):
        local = np.cumsum(v[lo:lo + Ls])               # sequential adds from the first element
        cum[lo:lo + Ls] = off + local
        off = off + local[-1]
    return cum


def plusplus(X, K, u, trace=None):
    """(index int64 [K], centres fp64 [K, cols]) of es_kmeans_plusplus on the draws u [K, trials].  trace
    receives "search_gap" (the smallest |cum - v| / total next to a chosen candidate) and "pot_gap" (the
    smallest relative gap between the best and the second-best potential)."""
    X = np.asarray(X, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    rows = X.shape[0]
    index = np.zeros(K, dtype=np.int64)
    index[0] = min(int(np.floor(u[0, 0] * rows)), rows - 1)
    closest = ((X - X[index[0]]) ** 2).sum(axis=1)
    gaps, pgaps = [], []
    for s in range(1, K):
        cum = prefix_sums(closest)
        total = cum[-1]
        v = u[s] * total
        cand = np.minimum(np.searchsorted(cum, v, side="left"), rows - 1)
        for c, vv in zip(cand, v):
            near = [abs(cum[c] - vv)] + ([abs(cum[c - 1] - vv)] if c > 0 else [])
            gaps.append(min(near) / total if total > 0 else np.inf)
        dmin = np.stack([np.minimum(closest, ((X - X[c]) ** 2).sum(axis=1)) for c in cand])
        pot = dmin.sum(axis=1)
        best = int(np.argmin(pot))                      # the first of equal minima
        others = np.delete(pot, best)
        distinct = others[np.delete(cand, best) != cand[best]]
        if distinct.size:
            pgaps.append(float((distinct.min() - pot[best]) / max(pot[best], 1e-300)))
        index[s] = cand[best]
        closest = dmin[best]
    if trace is not None:
        trace.update(search_gap=min(gaps) if gaps else np.inf, pot_gap=min(pgaps) if pgaps else np.inf)
    return index, X[index].copy()


# ---------------------------------------------------------------------------------------------- metrics
def confusion(pred, target, n_pred, n_true):
    """(counts int64 [n_true, n_pred], invalid) by np.add.at."""
    pred, target = np.asarray(pred, dtype=np.int64), np.asarray(target, dtype=np.int64)
    ok = (pred >= 0) & (pred < n_pred) & (target >= 0) & (target < n_true)
    cm = np.zeros((n_true, n_pred), dtype=np.int64)
    np.add.at(cm, (target[ok], pred[ok]), 1)
    return cm, int((~ok).sum())


def _comb2(n):
    return n * (n - 1) // 2


def metrics(cm):
    """The numbers of expertsim.train.diagnostics.agreement_metrics by other routes: class loops, the
    binomial form of the adjusted Rand index and a search over all relabellings."""
    cm = np.asarray(cm, dtype=np.int64)
    k = max(cm.shape)
    sq = np.zeros((k, k), dtype=np.int64)
    sq[:cm.shape[0], :cm.shape[1]] = cm
    total = int(sq.sum())
    prec, rec, f1 = [], [], []
    for c in range(k):
        tp, n_p, n_t = int(sq[c, c]), int(sq[:, c].sum()), int(sq[c, :].sum())
        if n_p + n_t == 0:
            continue
        p = tp / n_p if n_p else 0.0
        r = tp / n_t if n_t else 0.0
        prec.append(p)
        rec.append(r)
        f1.append(2 * p * r / (p + r) if p + r > 0 else 0.0)
    mean = lambda v: float(np.mean(v)) if v else 0.0
    s_ij = sum(_comb2(int(v)) for v in sq.ravel())
    s_a = sum(_comb2(int(v)) for v in sq.sum(axis=1))
    s_b = sum(_comb2(int(v)) for v in sq.sum(axis=0))
    n2 = _comb2(total)
    if s_a == s_ij and s_b == s_ij:
        ari = 1.0                                       # the same partition on both sides (sklearn's special case)
    else:
        expected = s_a * s_b / n2
        ari = (s_ij - expected) / (0.5 * (s_a + s_b) - expected)
    best = max(sum(int(sq[i, p[i]]) for i in range(k)) for p in itertools.permutations(range(k))) if k <= 7 else None
    return {"accuracy": float(np.trace(sq)) / total if total else 0.0, "precision": mean(prec), "recall": mean(rec),
            "f1": mean(f1), "adjusted_rand": float(ari),
            "matched_accuracy": (best / total if total else 0.0) if best is not None else None}


def load_golden():
    return np.load(GOLDEN)
