"""The segment rule of the analysis kernels (csrc/segment.h, include/expertsim_hip.h "Segments follow
es_wasserstein_1d") restated once in numpy for the tests."""
import numpy as np


def span(b, e, rows, cap=None):
    """(first position, length) of a segment with the bounds (b, e) over `rows` positions: b clamped to [0, rows],
    e to [b, rows], the length to cap (None: no cap)."""
    b = min(max(int(b), 0), rows)
    e = min(max(int(e), b), rows)
    n = e - b
    return b, n if cap is None else min(n, int(cap))


def row(idx, p, rows):
    """The row of position p: p itself without an index, else idx[p] clamped to [0, rows)."""
    return int(p) if idx is None else min(max(int(idx[p]), 0), rows - 1)


def members(rows, idx, seg, cap=None):
    """Per segment of seg [n_seg, 2] the row indices (int64 array) the kernels read, in member order."""
    out = []
    for b, e in np.asarray(seg).reshape(-1, 2):
        b, n = span(b, e, rows, cap)
        m = np.arange(b, b + n, dtype=np.int64)
        out.append(m if idx is None else np.clip(np.asarray(idx)[m], 0, rows - 1).astype(np.int64))
    return out
