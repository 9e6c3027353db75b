"""Writes tests/golden/tsne_sklearn.npz: scikit-learn's exact t-SNE on a small clustered set, the yardstick of
tests/test_embedding_gpu.py's end-to-end test.  Run once on a CPU (minutes); never run from a test.

    python tools/make_tsne_golden.py [--out tests/golden/tsne_sklearn.npz]

Contents (data only):
  X            [1024, 9] fp32   four Gaussian clusters of 256 points, centres N(0, 36 I), unit spread, seed 20240
  labels       [1024]    int32  the cluster of each point
  y_pca        [1024, 2] fp32   TSNE(method='exact', init='pca', perplexity=30, max_iter=1000, random_state=42)
  kl_pca, n_iter_pca            its kl_divergence_ and n_iter_
  y_random     [5, 1024, 2]     the same with init='random', random_state = 0 .. 4
  kl_random    [5]
  purity_pca, purity_random [5] 10-nearest-neighbour label purity of each embedding
  sklearn_version
"""
import argparse
import os

import numpy as np

SEED = 20240
RANDOM_SEEDS = (0, 1, 2, 3, 4)


def make_data():
    rng = np.random.default_rng(SEED)
    centres = rng.normal(0.0, 6.0, (4, 9))
    labels = np.repeat(np.arange(4), 256)
    X = (centres[labels] + rng.normal(0.0, 1.0, (1024, 9))).astype(np.float32)
    return X, labels.astype(np.int32)


def knn_purity(y, labels, k=10):
    """Mean fraction of a point's k nearest neighbours (itself excluded) that carry its label."""
    y = np.asarray(y, dtype=np.float64)
    d = ((y[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1, kind="stable")[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


def main():
    import sklearn
    from sklearn.manifold import TSNE
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(here, "tests", "golden", "tsne_sklearn.npz"))
    args = ap.parse_args()
    X, labels = make_data()
    kw = dict(n_components=2, method="exact", perplexity=30, max_iter=1000)
    t = TSNE(init="pca", random_state=42, **kw)
    y_pca = t.fit_transform(X)
    out = {"X": X, "labels": labels, "y_pca": y_pca.astype(np.float32), "kl_pca": np.float64(t.kl_divergence_),
           "n_iter_pca": np.int32(t.n_iter_), "purity_pca": np.float64(knn_purity(y_pca, labels))}
    print("pca init: KL", t.kl_divergence_, "n_iter", t.n_iter_, "purity", out["purity_pca"], flush=True)
    ys, kls, pur = [], [], []
    for s in RANDOM_SEEDS:
        t = TSNE(init="random", random_state=s, **kw)
        y = t.fit_transform(X)
        ys.append(y.astype(np.float32))
        kls.append(t.kl_divergence_)
        pur.append(knn_purity(y, labels))
        print("random init", s, ": KL", kls[-1], "purity", pur[-1], flush=True)
    out.update(y_random=np.stack(ys), kl_random=np.asarray(kls, dtype=np.float64),
               purity_random=np.asarray(pur, dtype=np.float64), sklearn_version=np.asarray(sklearn.__version__))
    np.savez_compressed(args.out, **out)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
