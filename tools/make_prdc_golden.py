"""Write tests/golden/prdc_sklearn.npz: the `prdc` formulation on scikit-learn (three pairwise_distances in fp64,
np.partition, the four reductions) on a half-collapsed synthetic generator, the yardstick of the device
precision / recall / density / coverage.  Needs scikit-learn; runs on the host.

    python tools/make_prdc_golden.py

Inputs (tests/prdc_refs.make_inputs): neutron 161 real x 149 generated x 1936 and proton 97 x 96 x 1680, the
synthetic batches of seeds 11 and 12, the first half of the generated side replaced by +-2 % multiplicative
perturbations of four of its own rows; a 3-expert vector per side with expert 0 empty and expert 1 of 12 real /
9 generated rows (not valid at k = 16).  Stored: the inputs, and for k = 1, 5, 16 and the segments joint, expert 0,
1, 2 scikit-learn's squared radii of both sides and the totals row (n_r, n_f, valid, precision_hits, recall_hits,
density_pairs, coverage_hits, 0).

The tool asserts what the tests rely on and fails otherwise (change the expert vector, not the factor): with
B = (cols + 3) 2^-52 4 max|x|^2, the rounding bound of scikit-learn's expansion form against the exact squared
distance, every strict comparison of every valid segment has |d2 - radius2| >= 1000 B in the difference form; the
difference form (tests/prdc_refs.segment) gives scikit-learn's integers and radii within B; no joint total is
0 and no precision or recall numerator is everything (the coverage numerator does saturate as k grows: every real
row is covered for the proton set at k = 5 and for both at k = 16).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import prdc_refs as R  # noqa: E402

FACTOR = 1000.0


def main():
    out = {}
    for arch in R.ARCHS:
        real, fake, e_r, e_f = R.make_inputs(arch)
        out.update({f"{arch}_real": real, f"{arch}_fake": fake, f"{arch}_expert_r": e_r, f"{arch}_expert_f": e_f})
        m_r, m_f = R.members(e_r, R.N_EXPERTS), R.members(e_f, R.N_EXPERTS)
        assert len(m_r[1]) == 0 and len(m_f[1]) == 0 and len(m_r[2]) == 12 and len(m_f[2]) == 9
        for k in R.KS:
            totals = np.zeros((len(m_r), 8), dtype=np.int64)
            for s, (ir, jf) in enumerate(zip(m_r, m_f)):
                a, b = real[ir], fake[jf]
                r2, f2, t = R.sklearn_prdc(a, b, k)
                ref = R.segment(a, b, k)
                assert np.array_equal(t, ref["totals"]), (arch, k, s, t, ref["totals"])
                if t[2]:
                    B = R.bound(a, b)
                    gap = R.min_gap(a, b, k)
                    assert gap >= FACTOR * B, f"{arch} k={k} segment {s}: gap {gap:.3g} < {FACTOR:g} B = {FACTOR * B:.3g}"
                    assert np.abs(r2 - ref["r_radius2"]).max() <= B and np.abs(f2 - ref["f_radius2"]).max() <= B
                    print(f"{arch} k={k} segment {s}: totals {t[:7].tolist()}  gap {gap / B:.3g} B")
                else:
                    print(f"{arch} k={k} segment {s}: not valid ({t[0]} x {t[1]})")
                totals[s] = t
                out[f"{arch}_k{k}_s{s}_r_radius2"] = r2
                out[f"{arch}_k{k}_s{s}_f_radius2"] = f2
            n_r, n_f = int(totals[0, 0]), int(totals[0, 1])
            assert 0 < totals[0, 3] < n_f and 0 < totals[0, 4] < n_r and totals[0, 5] > 0 and totals[0, 6] > 0
            out[f"{arch}_k{k}_totals"] = totals
    np.savez_compressed(R.GOLDEN, **out)
    size = os.path.getsize(R.GOLDEN)
    assert size < 512 * 1024, size
    print(f"wrote {R.GOLDEN}: {size} bytes")


if __name__ == "__main__":
    main()
