"""Writes tests/golden/classifier_sklearn.npz, the record behind tests/test_classifier_*.py: what scikit-learn and
scipy give for the seeded cases of tests/classifier_refs.py.  Needs scikit-learn (1.7.2 was used) and scipy (1.15.3);
the tests need neither.

    python tests/golden/make_classifier_goldens.py

Per rank case:  ks_2samp(u, v).statistic, mannwhitneyu(u, v).statistic, roc_auc_score(labels, values).
Per fit case:   theta = (intercept, coef) of LogisticRegression(C=1/l2, solver="newton-cholesky", tol=1e-12) on the
                float64 widening of the case's rows, real rows labelled 1.
Per c2st case:  theta of the same classifier on the training half of every segment's features.
Inputs are regenerated from their seeds; the record holds the shapes so that a changed generator is noticed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import classifier_refs as R  # noqa: E402


def sk_theta(Z, y, l2=R.L2):
    from sklearn.linear_model import LogisticRegression
    clf = LogisticRegression(C=1.0 / l2, solver="newton-cholesky", tol=1e-12, max_iter=200)
    clf.fit(Z[:, 1:], y)
    return np.concatenate([clf.intercept_, clf.coef_[0]]).astype(np.float64)


def main():
    import scipy
    import sklearn
    from scipy.stats import ks_2samp, mannwhitneyu
    from sklearn.metrics import roc_auc_score
    rec = {"versions": np.array([sklearn.__version__, scipy.__version__])}
    for kind in R.RANK_KINDS:
        for nu, nv in R.RANK_SIZES:
            u, v = R.rank_case(kind, nu, nv)
            labels = np.concatenate([np.ones(nu), np.zeros(nv)])
            rec[f"rank_{kind}_{nu}_{nv}"] = np.array([ks_2samp(u, v).statistic, mannwhitneyu(u, v).statistic,
                                                      roc_auc_score(labels, np.concatenate([u, v]))])
    for name in R.FIT_CASES:
        real, fake = R.fit_case(name)
        Z, y = R.design(real, fake)
        rec[f"fit_{name}_shape"] = np.array([real.shape[0], fake.shape[0], real.shape[1]])
        rec[f"fit_{name}_theta"] = sk_theta(Z, y)
    for name in R.C2ST_CASES:
        xr, xf, expert, E = R.c2st_features(name)
        for s, rows in enumerate(R.segments(expert, E, len(xr))):
            Z, y = R.train_design(xr, xf, rows)
            rec[f"c2st_{name}_s{s}_theta"] = sk_theta(Z, y)
            rec[f"c2st_{name}_s{s}_rows"] = np.array([len(rows)])
    np.savez_compressed(os.path.join(HERE, "classifier_sklearn.npz"), **rec)
    print("wrote", len(rec), "arrays")


if __name__ == "__main__":
    main()
