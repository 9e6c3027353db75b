"""Writes tests/golden/conditional_numpy.npz, the record behind tests/test_conditional_*.py: what numpy
(np.quantile, np.searchsorted), pandas (pd.qcut) and scipy (wasserstein_distance, ks_2samp) give on the seeded
fixture of tests/conditional_refs.py (N = 600, four bins, three columns).  numpy 2.2.6, pandas 2.3.3 and scipy 1.15.3
were used; the CPU tests need only numpy.

    python tests/golden/make_conditional_goldens.py

The record holds, for the cases "redraw" (an independent draw from the same conditional law), "shuffled" (the real
rows permuted across the conditions) and "experts" (redraw with three experts of which one owns no row), the tables
and scalars of conditional_refs.profile, whose quantiles are asserted here to be np.quantile's and whose bins to be
np.searchsorted's and pd.qcut's (the (a, b] convention), bit for bit.  Conditions on the fixture that the tests rely
on are asserted here too: the four bins are non-empty, the shuffled table's marginal Wasserstein distance is exactly
0 in every column, and its cond_ws of column 0 is at least five times the redraw's.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conditional_refs as R  # noqa: E402

TABLES = ("edges", "bin", "count", "q_real", "q_gen", "mean_real", "mean_gen", "std_real", "std_gen", "ws", "ks",
          "scale")


def main():
    import pandas as pd
    from scipy.stats import wasserstein_distance
    by, real, redraw, shuffled, expert = R.fixture()
    edges = np.quantile(by, [k / R.BINS for k in range(1, R.BINS)])
    bins = np.searchsorted(edges, by, side="left")
    codes = pd.qcut(by, R.BINS, labels=False)
    assert (R.bin_edges(by, R.BINS) == edges).all() and (R.bin_of(edges, by) == bins).all() and (codes == bins).all()
    assert np.bincount(bins, minlength=R.BINS).min() > 0
    rec = {"versions": np.array([np.__version__, pd.__version__, __import__("scipy").__version__]),
           "np_edges": edges, "np_bin": bins.astype(np.int32), "qcut_codes": codes.astype(np.int32)}
    cases = {"redraw": (redraw, None, 1), "shuffled": (shuffled, None, 1), "experts": (redraw, expert, 3)}
    out = {}
    for name, (fake, ex, E) in cases.items():
        t = out[name] = R.profile(real, fake, by, R.BINS, ex, E, names=R.NAMES)
        for s in range(t["count"].shape[0]):
            for k in range(R.BINS):
                m = (bins == k) if s == 0 else ((bins == k) & (ex == s - 1))
                for c in range(3):
                    for side, x in (("q_real", real), ("q_gen", fake)):
                        want = np.quantile(x[m, c], R.PROBS) if m.any() else np.full(3, np.nan)
                        assert np.array_equal(t[side][s, k, c], want, equal_nan=True), (name, s, k, c, side)
        for key in TABLES:
            rec[f"{name}_{key}"] = t[key]
        rec[f"{name}_width_sum"] = np.array([t["width_sum"][o] for o in R.NAMES])
        rec[f"{name}_keys"] = np.array(sorted(t["scalars"]))
        rec[f"{name}_values"] = np.array([t["scalars"][k] for k in sorted(t["scalars"])])
    for c in range(3):
        assert wasserstein_distance(real[:, c], shuffled[:, c]) == 0.0
    ws_shuffled, ws_redraw = out["shuffled"]["scalars"]["cond_ws_lin"], out["redraw"]["scalars"]["cond_ws_lin"]
    print("cond_ws_lin shuffled", ws_shuffled, "redraw", ws_redraw)
    assert ws_shuffled >= 5 * ws_redraw
    assert out["experts"]["count"][2].sum() == 0 and np.isnan(out["experts"]["scalars"]["cond_ws_1"])
    np.savez_compressed(os.path.join(HERE, "conditional_numpy.npz"), **rec)
    print("wrote", len(rec), "arrays")


if __name__ == "__main__":
    main()
