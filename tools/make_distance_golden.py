"""Write tests/golden/distances_scipy.npz: the yardstick of the device Frechet and kernel distances (DESIGN.md
§7i), from numpy, scipy and scikit-learn only.  Runs on the host.

    python tools/make_distance_golden.py

Stored (inputs from tests/distance_refs.py):
* Frechet cases `fr_<kind>_<cols>` for kind = gauss (correlated Gaussian rows, condition number a few hundred)
  and obs (normalised non-negative observable-like rows), cols = 1, 2, 10, 32, 300 rows a side: the moments of
  both sides from np.mean / np.cov (the exact bits the device starts from), the four Frechet numbers two ways --
  scipy.linalg.sqrtm(A @ B) and the symmetric eigh form --, their disagreement D in units of
  U = 2^-52 cols (tr A + tr B + |dmu|^2), and the condition numbers of A and B.
* Kernel cases `mmd_<i>` (distance_refs.MMD_CASES, at most 16 columns): the fp32 rows of both sides and the three
  sums from sklearn.metrics.pairwise.polynomial_kernel.
* The expert case `ex_*`: 400 x 10 rows a side and a 3-expert vector with expert 1 empty and expert 2 of 7 rows;
  per segment (joint, expert 0, 1, 2) the host tables of fpd (FD_j, n_j) and kpd (sums, counts), the values
  np.polyfit / np.median / np.percentile give from them, and which segments are NaN.

The tool asserts what the tests rely on and fails otherwise: every Frechet case has condition numbers <= 1e3 and
D <= 4 U; the restatement's kernel sums agree with scikit-learn's within the rounding bound of
distance_refs.poly_bound; exactly the segments of experts 1 and 2 of the expert case are NaN.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "generative-dnn-for-physics-simulations-cern_amd"))
import distance_refs as R  # noqa: E402


def host_fpd(table, cols):
    """(fpd, fpd_err, fd_full) of a [points, 3] table by np.polyfit; NaN when n_0 <= cols."""
    fd, n = table[:, 0], table[:, 1]
    if not n[0] > cols:
        return np.full(3, np.nan)
    coef, cov = np.polyfit(1.0 / n, fd, 1, cov=True)
    return np.array([coef[1], np.sqrt(cov[1, 1]), fd[-1]])


def host_kpd(table):
    """(kpd, kpd_err, mmd_full) of a [blocks + 1, 5] table by np.median / np.percentile; NaN when m < 2."""
    if table[0, 3] < 2:
        return np.full(3, np.nan)
    v = np.array([R.mmd2(row[:3], row[3], row[4]) for row in table])
    q75, q25 = np.percentile(v[:-1], [75, 25])
    return np.array([np.median(v[:-1]), 0.5 * (q75 - q25), v[-1]])


def main():
    out = {}
    for kind, cols in R.FRECHET_CASES:
        a, b = R.frechet_case(kind, cols)
        (_, ma, ca), (_, mb, cb) = R.moments(a), R.moments(b)
        unit = R.frechet_unit(ma, ca, mb, cb)
        eigh, sqrtm = R.frechet_eigh(ma, ca, mb, cb), R.frechet_sqrtm(ma, ca, mb, cb)
        D = float(np.abs(eigh - sqrtm).max() / unit)
        ka, kb = float(np.linalg.cond(ca)), float(np.linalg.cond(cb))
        print(f"fr_{kind}_{cols}: d2 = {eigh[0]:.6g}  D = {D:.3g} U  cond A = {ka:.3g}  cond B = {kb:.3g}")
        assert ka <= 1e3 and kb <= 1e3, (kind, cols, ka, kb)
        assert D <= 4.0, (kind, cols, D)
        key = f"fr_{kind}_{cols}"
        out.update({f"{key}_mean_a": ma, f"{key}_cov_a": ca, f"{key}_mean_b": mb, f"{key}_cov_b": cb,
                    f"{key}_eigh": eigh, f"{key}_sqrtm": sqrtm, f"{key}_D": np.float64(D),
                    f"{key}_cond": np.array([ka, kb])})
    for i, (cols, m, n, degree) in enumerate(R.MMD_CASES):
        x, y = R.mmd_case(cols, m, n, degree)
        sk = R.sklearn_sums(x, y, degree)
        ref, absum = R.poly_sums(x, y, degree)
        bound = R.poly_bound(m, n, cols, degree, absum)
        assert (np.abs(sk - ref) <= bound).all(), (i, sk, ref, bound)
        print(f"mmd_{i}: cols={cols} m={m} n={n} degree={degree}  sums {sk}  |sklearn - restatement| / bound "
              f"{np.max(np.abs(sk - ref) / np.where(bound > 0, bound, 1.0)):.3g}")
        out.update({f"mmd_{i}_x": x, f"mmd_{i}_y": y, f"mmd_{i}_sums": sk})
    real, fake, expert = R.expert_case()
    out.update(ex_real=real, ex_fake=fake, ex_expert=expert)
    members = [np.arange(len(real))] + [np.where(expert == e)[0] for e in range(R.EXPERT_E)]
    fpd_nan, kpd_nan = [], []
    for s, ix in enumerate(members):
        ft, kt = R.fpd_table(real[ix], fake[ix]), R.kpd_table(real[ix].astype(np.float32), fake[ix].astype(np.float32))
        fv, kv = host_fpd(ft, R.EXPERT_COLS), host_kpd(kt)
        fpd_nan.append(bool(np.isnan(fv).all()))
        kpd_nan.append(bool(np.isnan(kv).all()))
        print(f"ex segment {s}: {len(ix)} rows  fpd {fv}  kpd {kv}")
        out.update({f"ex_s{s}_fpd_table": ft, f"ex_s{s}_kpd_table": kt, f"ex_s{s}_fpd": fv, f"ex_s{s}_kpd": kv})
    assert fpd_nan == [False, False, True, True] and kpd_nan == [False, False, True, True], (fpd_nan, kpd_nan)
    out.update(ex_fpd_nan=np.array(fpd_nan), ex_kpd_nan=np.array(kpd_nan))
    np.savez_compressed(R.GOLDEN, **out)
    size = os.path.getsize(R.GOLDEN)
    assert size < 512 * 1024, size
    print(f"wrote {R.GOLDEN}: {size} bytes")


if __name__ == "__main__":
    main()
