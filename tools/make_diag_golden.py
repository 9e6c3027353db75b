"""Writes tests/golden/diag_kde.npz: the truth of the es_segment_kde tests, computed on the host in
np.longdouble so that the GPU tests need neither longdouble nor scipy.

Per case (tests/diag_refs.py GOLDEN_CASES): the members d, the grid, the restated sd (fixed-order moments,
ddof = 1), h = sd * n ** -0.2, the density at that h evaluated in np.longdouble and rounded to fp64, and per
grid point the weighted mean exponent A_j = sum_i a_ij t_ij / sum_i t_ij, a = z^2 / 2, t = exp(-a), which
scales the tests' error bound.

    python tools/make_diag_golden.py          (CPU only; seeded, reproducible)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import diag_refs as DR  # noqa: E402

LD = np.longdouble


def truth(d, grid, h):
    """(density fp64 [points], A fp64 [points]) in np.longdouble at the bandwidth h."""
    n = len(d)
    z = (grid.astype(LD)[:, None] - d.astype(LD)[None, :]) / LD(h)
    a = z * z / LD(2)
    t = np.exp(-a)
    T = t.sum(axis=1)
    assert (T > 0).all(), "a grid point underflows even in longdouble"
    density = T / (LD(n) * LD(h) * np.sqrt(LD(2) * LD(np.pi)))
    return density.astype(np.float64), ((a * t).sum(axis=1) / T).astype(np.float64)


def make_case(name, rng):
    if name == "n1000_clusters":
        # two far-apart clusters and a caller-given grid of an odd length that runs far past the data, so
        # that the outer grid points' densities fall below 2^-1000
        d = np.concatenate([rng.normal(-40.0, 0.5, 400), rng.normal(55.0, 1.5, 600)])
        rng.shuffle(d)
        grid = None
        points = 37
    else:
        n = int(name[1:])
        d = rng.gamma(2.0, 1.5, n) if n != 64 else rng.normal(3.0, 2.0, n)
        grid = DR.linspace_ref(d.min(), d.max(), 100)
        points = 100
    n = len(d)
    _, _, Q = DR.moments_ref(d)
    sd = np.sqrt(Q / (np.float64(n) - 1.0))
    h = sd * np.float64(n) ** -0.2
    if grid is None:
        grid = DR.linspace_ref(d.min() - 45.0 * h, d.max() + 45.0 * h, points)
    density, A = truth(d, grid, h)
    return dict(d=d, grid=grid, sd=np.float64(sd), h=np.float64(h), density=density, A=A)


def main():
    assert np.finfo(LD).nmant >= 63, f"np.longdouble has {np.finfo(LD).nmant} mantissa bits: no better than fp64 here"
    rng = np.random.default_rng(20240611)
    out = {}
    for name in DR.GOLDEN_CASES:
        case = make_case(name, rng)
        for k, v in case.items():
            out[f"{name}_{k}"] = np.asarray(v, dtype=np.float64)
        tiny = int((case["density"] < 2.0 ** -1000).sum())
        print(f"{name}: n={len(case['d'])} points={len(case['grid'])} h={case['h']:.6g} max A={case['A'].max():.4g} "
              f"below 2^-1000: {tiny}")
    path = os.path.join(ROOT, "tests", "golden", "diag_kde.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {sum(v.size for v in out.values())} values")


if __name__ == "__main__":
    main()
