"""fp64 numpy restatement of es_group_diversity and es_image_sum_peak (csrc/prepare.hip) in the kernels' own
arithmetic order, the goldens of the dataset-preparation tests and the bounds they share.

group_diversity_ref follows include/expertsim_hip.h to the letter.  Per group of n members and per pixel:
S = the sum of the members in perm order from +0.0, m = S / n, Q = the sum in the same order of the rounded
products d * d with d = x - m, var = Q / n, sd = sqrt(var); n <= SPLIT_MIN is one sequential chain, larger
groups are cut into CHUNKS chunks of L = ceil(n / CHUNKS) members, each summed sequentially from +0.0, the
chunk sums added in chunk order from +0.0.  group_sum adds sd over 128-pixel tiles (row-major pixel index,
padded with +0.0): inside a tile a[i] = sd[2i] + sd[2i+1], the 64 values by the butterfly
a[i] <- a[i] + a[i ^ o], o = 32 .. 1, then the tile sums in tile order from +0.0.  numpy's elementwise
+, -, *, / and sqrt on float64 arrays are IEEE operations without contraction, so loops over the members
(not np.sum, whose order is pairwise) restate the kernel.

image_sum_peak_ref: lane l of 64 adds the pixels l, l + 64, .. in that order from +0.0, then the same
butterfly; the peak is np.argmax in the input's own precision.

Bounds (the issue's): group_sum within (2 n_g + h w + 16) 2^-53 relative of pandas / numpy -- two n-term sums
and one (h w)-term sum of non-negative terms, plus slack for the division, square root and rounding steps;
photon_sum within h w 2^-53 relative.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from golden_utils import GOLDEN_DIR
from segment_refs import members

SPLIT_MIN = 256          # ES_PREP_SPLIT_MIN
CHUNKS = 16              # ES_PREP_CHUNKS
TILE = 128               # pixels of a tile of group_sum: two per lane
LANES = 64
U = 2.0 ** -53
_LANES = np.arange(LANES)


def _widen(x):
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64), x.dtype
    return x.astype(np.float64)


def _chain(rows, m=None):
    """Sequential sum over axis 0 from +0.0 of rows (m None) or of the rounded (rows - m)^2."""
    acc = np.zeros(rows.shape[1:], dtype=np.float64)
    for k in range(rows.shape[0]):
        if m is None:
            acc = acc + rows[k]
        else:
            d = rows[k] - m
            q = d * d
            acc = acc + q
    return acc


def _member_sum(rows, m=None):
    n = rows.shape[0]
    if n <= SPLIT_MIN:
        return _chain(rows, m)
    L = -(-n // CHUNKS)
    acc = np.zeros(rows.shape[1:], dtype=np.float64)
    for c in range(CHUNKS):
        acc = acc + _chain(rows[min(c * L, n):min((c + 1) * L, n)], m)
    return acc


def butterfly(a):
    """[..., 64] -> [...]: a[i] <- a[i] + a[i ^ o] for o = 32, 16, 8, 4, 2, 1 (wave_sum_d)."""
    a = np.asarray(a, dtype=np.float64)
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[..., _LANES ^ o]
    return a[..., 0]


def tile_sum(v):
    """[..., P] non-negative -> [...]: 128-value tiles (neighbours added, then the butterfly), the tile sums in
    tile order."""
    P = v.shape[-1]
    T = -(-P // TILE)
    pad = np.zeros(v.shape[:-1] + (T * TILE,), dtype=np.float64)
    pad[..., :P] = v
    pad = pad.reshape(v.shape[:-1] + (T, LANES, 2))
    parts = butterfly(pad[..., 0] + pad[..., 1])
    acc = np.zeros(v.shape[:-1], dtype=np.float64)
    for t in range(T):
        acc = acc + parts[..., t]
    return acc


def group_diversity_ref(x, perm, offs):
    """x [N,H,W] fp32 / fp64, perm [N], offs [G+1] -> (group_sum [G] fp64, pix_var [G, H*W] fp64)."""
    x = _widen(x)
    N = x.shape[0]
    flat = x.reshape(N, -1)
    perm, offs = np.asarray(perm), np.asarray(offs)
    G = len(offs) - 1
    pix_var = np.zeros((G, flat.shape[1]), dtype=np.float64)
    for g, m in enumerate(members(N, perm, np.stack([offs[:-1], offs[1:]], axis=1))):
        if len(m) == 0:
            continue
        rows = flat[m]
        n = np.float64(len(m))
        m = _member_sum(rows) / n
        pix_var[g] = _member_sum(rows, m) / n
    return tile_sum(np.sqrt(pix_var)), pix_var


def image_sum_peak_ref(x):
    """x [N,H,W] fp32 / fp64 -> (sum [N] fp64, peak [N,2] int32)."""
    x = np.asarray(x)
    N, H, W = x.shape
    flat = _widen(x).reshape(N, -1)
    P = flat.shape[1]
    K = -(-P // LANES)
    pad = np.zeros((N, K * LANES), dtype=np.float64)
    pad[:, :P] = flat
    pad = pad.reshape(N, K, LANES)
    lanes = np.zeros((N, LANES), dtype=np.float64)
    for k in range(K):                      # the padding adds +0.0 to a sum that is never -0.0
        lanes = lanes + pad[:, k]
    am = x.reshape(N, -1).argmax(axis=1)
    return butterfly(lanes), np.stack([am // W, am % W], axis=1).astype(np.int32)


def layout(group, n_groups):
    """(perm int32 [N], offs int32 [G+1]): members in ascending sample index (group_layout on the host)."""
    group = np.asarray(group)
    perm = np.argsort(group, kind="stable").astype(np.int32)
    offs = np.zeros(n_groups + 1, dtype=np.int32)
    offs[1:] = np.cumsum(np.bincount(group, minlength=n_groups))
    return perm, offs


def group_sum_bound(counts, hw):
    """Relative bound on group_sum per group: (2 n_g + h w + 16) 2^-53."""
    return (2.0 * np.asarray(counts, dtype=np.float64) + hw + 16.0) * U


GOLDEN_KEYS = ("images", "cond", "group_number", "group_sum", "std", "photon_sum", "max_x", "max_y")


@functools.lru_cache(maxsize=None)
def golden(zdc):
    """The record of tests/golden/make_prepare_goldens.py for "neutron" (44x44) or "proton" (56x30), read-only."""
    z = np.load(os.path.join(GOLDEN_DIR, f"prepare_{zdc}.npz"))
    out = {k: z[k] for k in GOLDEN_KEYS}
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def golden_ref(zdc, dtype="float64"):
    """The restatement on the golden images (as `dtype`): dict of perm, offs, counts, group_sum, pix_var, sum,
    peak.  Computed once and shared; read-only."""
    g = golden(zdc)
    x = g["images"].astype(dtype)
    n_groups = int(g["group_number"].max()) + 1
    perm, offs = layout(g["group_number"], n_groups)
    group_sum, pix_var = group_diversity_ref(x, perm, offs)
    s, peak = image_sum_peak_ref(x)
    out = dict(perm=perm, offs=offs, counts=np.diff(offs), group_sum=group_sum, pix_var=pix_var, sum=s, peak=peak)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(h, w, sizes, seed=0, dtype="float64"):
    """Seeded images for the kernel tests: groups of the given sizes, members interleaved so that perm is not
    the identity; returns (x [N,h,w], group [N], perm, offs, group_sum, pix_var), read-only."""
    rng = np.random.default_rng(7919 * h + 31 * w + 1000003 * seed + sum(sizes))
    group = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(group)
    N = len(group)
    x = np.log1p(rng.poisson(3.0, size=(N, h, w)) * rng.random((N, h, w))).astype(dtype)
    perm, offs = layout(group, len(sizes))
    group_sum, pix_var = group_diversity_ref(x, perm, offs)
    out = (x, group, perm, offs, group_sum, pix_var)
    for a in out:
        a.setflags(write=False)
    return out
