"""Write tests/golden/sliced_numpy.npz: the yardstick of the device sliced Wasserstein distance, from
numpy and scipy only.  Runs on the host.

    python tools/make_sliced_golden.py

Stored, per record case `c<h>x<w>` of tests/sliced_refs.py (6x5 and 44x44; 257 rows a side, 64 directions, E = 3 with
expert 1 empty and expert 2 holding one row); numbers only:
* `_theta16`  the numpy-made direction matrix [64, h * w] as float16 (normal draws, normalised, rounded to float16:
              exact when widened to fp64, unit to within 2^-11, a quarter of the bytes of fp64);
* `_w`        scipy.stats.wasserstein_distance's [4, 64] table over the np.longdouble projections rounded to fp64;
* `_summary`  [3, 4] = (swd, swd_err, swd_max) per segment, NaN for the empty expert;
* `_counts`   [4, 2] rows per segment and side.

The tool asserts what the tests rely on and fails otherwise: exactly segment 2 (expert 1) is NaN, the one-row expert
has a finite distance, and the shifted generated side is farther from the real side than an unshifted draw.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sliced_refs as R  # noqa: E402


def main():
    out = {}
    for h, w in R.RECORD_SHAPES:
        theta, table, summ, counts, _ = R.record_case(h, w)
        nan = np.isnan(summ).all(axis=0)
        assert nan.tolist() == [False, False, True, False], nan
        assert np.isnan(summ[:, ~nan]).sum() == 0
        real = R.images(h, w, R.RECORD_N, seed=1)
        plain = R.images(h, w, R.RECORD_N, seed=3)
        (pr, _), (pp, _) = R.project_ref(real, theta), R.project_ref(plain, theta)
        base = R.w_table(pr.astype(np.float64), pp.astype(np.float64), [np.arange(R.RECORD_N)]).mean()
        print(f"c{h}x{w}: swd {summ[0]}  swd_err {summ[1]}  swd_max {summ[2]}  unshifted swd {base:.4g}")
        assert summ[0, 0] > base + 3 * summ[1, 0], (summ[0, 0], base)
        key = f"c{h}x{w}"
        out.update({f"{key}_theta16": R.record_theta16(h, w), f"{key}_w": table, f"{key}_summary": summ,
                    f"{key}_counts": counts.astype(np.int32)})
    np.savez_compressed(R.GOLDEN, **out)
    size = os.path.getsize(R.GOLDEN)
    assert size < 400 * 1024, size
    print(f"wrote {R.GOLDEN}: {size} bytes")


if __name__ == "__main__":
    main()
