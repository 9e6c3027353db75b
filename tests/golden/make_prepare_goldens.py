"""Writes tests/golden/prepare_{neutron,proton}.npz: synthetic log1p-domain calorimeter images with
conditions that repeat, and the dataset-preparation columns as pandas / numpy give them from the
definitions (not from the device kernels or their restatement):

    group_number  DataFrame.groupby(COND_COLUMNS).ngroup()
    std           per (group, pixel) np.std of the pixel column (pandas passes ddof = 0), summed over the
                  pixels per group (group_sum), divided by the largest group sum
    photon_sum    np.sum(image)
    max_x, max_y  np.unravel_index(np.argmax(image), (H, W))

Run from the repository root:  python tests/golden/make_prepare_goldens.py

The images are log1p of small integer photon counts of sparse showers, so the fp64 arrays hold few
distinct values and savez_compressed keeps each file well under the size limit.  Group sizes: 1, 1, 2, 3
(identical images on a quarter grid, whose sums are exact), 63, 64, 65 and 257; the samples are shuffled.
"""
import os

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
COND_COLUMNS = ["Energy", "Vx", "Vy", "Vz", "Px", "Py", "Pz", "mass", "charge"]
SIZES = [1, 1, 2, 3, 63, 64, 65, 257]
IDENTICAL = 3          # index of the group of identical images
CASES = {"neutron": (44, 44, 20261), "proton": (56, 30, 20262)}


def showers(rng, n, h, w, centre, spread):
    """n sparse showers: Poisson counts under a Gaussian blob, log1p of the integer counts."""
    yy, xx = np.mgrid[0:h, 0:w]
    cy = centre[0] + rng.normal(0.0, 1.5, size=(n, 1, 1))
    cx = centre[1] + rng.normal(0.0, 1.5, size=(n, 1, 1))
    amp = rng.uniform(5.0, 60.0, size=(n, 1, 1))
    blob = amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * spread ** 2))
    return np.log1p(rng.poisson(blob).astype(np.float64))


def build(h, w, seed):
    rng = np.random.default_rng(seed)
    # one conditions row per group, columns drawn from few values so that the lexicographic order is
    # decided in different columns; rows are made distinct by the last column that varies
    rows = []
    while len(rows) < len(SIZES):
        r = [rng.choice([120.0, 450.5, 2000.25]), rng.choice([-0.5, 0.0]), rng.choice([0.0, 0.25]),
             rng.choice([-10.0, 5.5]), rng.choice([-1.5, 2.5]), rng.choice([0.125, 3.0]),
             rng.choice([100.0, 1000.0, 1999.5]), 939.565, 0.0]
        if r not in rows:
            rows.append(r)
    images, cond = [], []
    for g, size in enumerate(SIZES):
        centre = (rng.uniform(0.3, 0.7) * h, rng.uniform(0.3, 0.7) * w)
        x = showers(rng, size, h, w, centre, rng.uniform(2.0, 4.0))
        if g == IDENTICAL:
            x = np.repeat(np.round(x[:1] * 4.0) / 4.0, size, axis=0)
        images.append(x)
        cond += [rows[g]] * size
    images, cond = np.concatenate(images), np.array(cond, dtype=np.float64)
    order = rng.permutation(len(images))
    images, cond = images[order], cond[order]
    # an image whose maximum occurs twice (the first, in row-major order, is the peak)
    tie = int(np.flatnonzero((cond == np.array(rows[5])).all(axis=1))[0])
    top = images[tie].max() + np.log1p(3.0)
    images[tie, h // 3, w // 2] = top
    images[tie, h // 2, w // 4] = top
    return images, cond


def expected(images, cond):
    n, h, w = images.shape
    frame = pd.DataFrame(cond, columns=COND_COLUMNS)
    group = frame.groupby(COND_COLUMNS).ngroup().to_numpy()
    pixels = pd.DataFrame(images.reshape(n, -1))
    per_pixel_sd = pixels.groupby(group).transform(lambda column: np.std(column))
    per_sample = per_pixel_sd.sum(axis=1).to_numpy()
    group_sum = np.zeros(group.max() + 1)
    group_sum[group] = per_sample
    std = per_sample / per_sample.max()
    photon_sum = np.array([np.sum(img) for img in images])
    peaks = np.array([np.unravel_index(np.argmax(img), (h, w)) for img in images])
    return dict(group_number=group.astype(np.int64), group_sum=group_sum, std=std, photon_sum=photon_sum,
                max_x=peaks[:, 0].astype(np.int64), max_y=peaks[:, 1].astype(np.int64))


def main():
    for zdc, (h, w, seed) in CASES.items():
        images, cond = build(h, w, seed)
        out = expected(images, cond)
        counts = np.bincount(out["group_number"])
        assert sorted(counts.tolist()) == sorted(SIZES)
        assert (out["group_sum"][counts == 1] == 0.0).all() and (counts == 1).sum() == 2
        assert (out["group_sum"] == 0.0).sum() == 3, "the identical-images group must give exactly 0"
        assert any((img == img.max()).sum() == 2 for img in images)
        path = os.path.join(HERE, f"prepare_{zdc}.npz")
        np.savez_compressed(path, images=images, cond=cond, **out)
        print(f"{path}: {images.shape} {os.path.getsize(path)} bytes; group sums {out['group_sum']}")


if __name__ == "__main__":
    main()
