"""fp64 numpy restatement of es_image_features (csrc/features.hip) in the kernel's own arithmetic, and the
seeded inputs its tests share.

image_features_ref follows include/expertsim_hip.h to the letter: each column sum is the fp64 sum over
i = 0..h-1 in that order and each row sum the fp64 sum over j = 0..w-1 in that order, both from +0.0 (a
loop, not np.sum, whose inner-axis order is pairwise); the hit count and the index sums are integers; each
centre is one fp64 division; the peak is the first maximum in row-major order.  The kernel is therefore
compared with it bit for bit, and it with the reference's float32 sums (tests/golden/image_features.npz)
within the float32 summation bound.
"""
from __future__ import annotations

import functools

import numpy as np

from golden_utils import GOLDEN_DIR

SHAPES = [(1, 1), (2, 3), (7, 5), (44, 44), (56, 30), (56, 56), (64, 64)]
GOLDEN_SHAPES = SHAPES[:6]


def image_features_ref(images):
    """images [N,H,W] float32 (already in the domain to describe) -> (feat [N,5] float64, peak [N,2] int32)."""
    images = np.asarray(images)
    assert images.ndim == 3 and images.dtype == np.float32
    n, h, w = images.shape
    v = images.astype(np.float64)
    col = np.zeros((n, w))
    for i in range(h):
        col = col + v[:, i, :]
    row = np.zeros((n, h))
    for j in range(w):
        row = row + v[:, :, j]
    hit = images > 0
    cnt = hit.reshape(n, -1).sum(axis=1, dtype=np.int64)
    sx = (hit * np.arange(w, dtype=np.int64)[None, None, :]).reshape(n, -1).sum(axis=1, dtype=np.int64)
    sy = (hit * np.arange(h, dtype=np.int64)[None, :, None]).reshape(n, -1).sum(axis=1, dtype=np.int64)
    feat = np.empty((n, 5), dtype=np.float64)
    feat[:, 0] = col.max(axis=1)
    feat[:, 1] = row.max(axis=1)
    some = cnt > 0
    safe = np.maximum(cnt, 1).astype(np.float64)
    feat[:, 2] = np.where(some, sx.astype(np.float64) / safe, np.float64(w) / 2.0)
    feat[:, 3] = np.where(some, sy.astype(np.float64) / safe, np.float64(h) / 2.0)
    feat[:, 4] = cnt.astype(np.float64)
    flat = images.reshape(n, -1).argmax(axis=1)
    peak = np.stack([flat // w, flat % w], axis=1).astype(np.int32)
    return feat, peak


def max_sum_bounds(images):
    """(bound on max_x, bound on max_y) per image: the float32 summation bound of the reference's own sums,
    (h-1) 2^-24 max_j sum_i |v| and (w-1) 2^-24 max_i sum_j |v|."""
    a = np.abs(np.asarray(images, dtype=np.float64))
    n, h, w = a.shape
    u = 2.0 ** -24
    return (h - 1) * u * a.sum(axis=1).max(axis=1), (w - 1) * u * a.sum(axis=2).max(axis=1)


@functools.lru_cache(maxsize=None)
def golden():
    """{(h, w): (images [6,h,w] f32, features [5,6] f64, peak [6,2] i32)} of the reference (read-only)."""
    import os
    z = np.load(os.path.join(GOLDEN_DIR, "image_features.npz"))
    out = {}
    for h, w in GOLDEN_SHAPES:
        arrs = tuple(z[f"{h}x{w}/{k}"] for k in ("images", "features", "peak"))
        for a in arrs:
            a.setflags(write=False)
        out[(h, w)] = arrs
    return out


def assert_matches_golden(feat, peak, shape):
    """feat [6,5] / peak [6,2] of the golden images of `shape` against the reference's record: nonzero,
    center_x, center_y and peak exactly, max_x / max_y within max_sum_bounds."""
    images, gfeat, gpeak = golden()[shape]
    bx, by = max_sum_bounds(images)
    ex, ey = np.abs(feat[:, 0] - gfeat[0]), np.abs(feat[:, 1] - gfeat[1])
    worst = max((ex / np.maximum(bx, 1e-300)).max(), (ey / np.maximum(by, 1e-300)).max())
    print(f"golden {shape}: worst max-sum error / bound {worst:.3f}")
    assert np.array_equal(feat[:, 2:], gfeat[2:].T), shape
    assert np.array_equal(peak, gpeak), shape
    assert (ex <= bx).all() and (ey <= by).all(), (shape, ex, bx, ey, by)


@functools.lru_cache(maxsize=None)
def case(h, w, n, seed=0):
    """Seeded float32 images [n,h,w] for the kernel tests (read-only): expm1(relu(normal)) with an all-zero
    image, an all-negative image and a doubled maximum among them when n allows, and the restatement of
    them."""
    rng = np.random.default_rng(1000 * h + 10 * w + n + seed)
    x = np.expm1(np.maximum(rng.standard_normal((n, h, w)), 0.0)).astype(np.float32)
    if n >= 5:
        x[1] = 0.0
        x[2] = -np.abs(x[2]) - np.float32(0.25)
        if h * w >= 2:
            a, b = sorted(rng.choice(h * w, size=2, replace=False))
            top = np.float32(x[3].max() * np.float32(1.5) + np.float32(1.0))
            x[3].reshape(-1)[a] = top
            x[3].reshape(-1)[b] = top
    feat, peak = image_features_ref(x)
    for a in (x, feat, peak):
        a.setflags(write=False)
    return x, feat, peak
