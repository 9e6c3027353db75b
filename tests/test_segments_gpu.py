"""One segment rule for every segmented entry (csrc/segment.h): hostile bounds and indices against their clean
equivalent, bit for bit.

Each of es_wasserstein_1d, es_segment_histogram, es_segment_kde, es_knn_radius, es_prdc_count and
es_group_diversity runs twice on the same data: once with bounds that start below 0, end past the rows, end
before they start and exceed the cap, and with an index holding entries outside [0, rows); once with the bounds
and the index that tests/segment_refs.py (the rule restated in numpy) makes of them.  Both calls start from the
same sentinel-filled outputs and every output must be equal bit for bit: the integers, the fp64 bits and the
entries past a segment's length that no kernel may touch.  No tolerance enters: the clean call reads the same
rows in the same order.

Shapes: 40 rows, cap 12, five segments of 9, 12 (cut by the cap), 0, 12 (cut by the cap) and 0 members -- an
empty segment, one below the KDE's floor of 5 members and below k + 1 = 3, and ones that clear both; 3 fp64
columns (Wasserstein, histogram, KDE), 5 fp32 columns (k-NN, k = 2), 4x4 images (diversity, whose groups are
consecutive bounds offs[g], offs[g + 1] without a cap; its clean call lists every group's members)."""
import numpy as np
import pytest
import torch

import segment_refs as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, CAP, K = 40, 12, 2
SEG = [[-7, 9], [9, 64], [30, 18], [5, 35], [0, 0]]
CLEAN_SEG = [[0, 9], [9, 21], [30, 30], [5, 17], [0, 0]]


def _index(seed):
    idx = np.random.RandomState(seed).permutation(ROWS).astype(np.int32)
    idx[[3, 11, 27]] = (-3, 40, 45)
    return idx


def _clean(idx):
    """The clean bounds and index of (SEG, idx): what segment_refs makes of them."""
    seg = np.array([[b, b + n] for b, n in (S.span(b, e, ROWS, CAP) for b, e in SEG)], dtype=np.int32)
    assert seg.tolist() == CLEAN_SEG
    clean = np.clip(idx, 0, ROWS - 1).astype(np.int32)
    hostile, tidy = S.members(ROWS, idx, SEG, CAP), S.members(ROWS, clean, seg, CAP)
    assert all(np.array_equal(a, b) for a, b in zip(hostile, tidy))
    assert [len(m) for m in hostile] == [9, 12, 0, 12, 0]
    return seg, clean


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


def _both(run, *idx):
    """run(seg, *idx) -> dict of device tensors, with the hostile arguments and with their clean equivalent."""
    cleaned = [_clean(i) for i in idx]
    first = run(_dev(np.array(SEG, dtype=np.int32)), *(_dev(i) for i in idx))
    second = run(_dev(cleaned[0][0]), *(_dev(c) for _, c in cleaned))
    torch.cuda.synchronize()
    assert set(first) == set(second)
    for key in first:
        _same(first[key], second[key], key)
    return first


def _columns(seed, cols, dtype):
    rs = np.random.RandomState(seed)
    x = rs.gamma(2.0, 3.0, (ROWS, cols))
    x[:, -1] = rs.randint(0, 3, ROWS)                    # a categorical column: ties
    return _dev(x.astype(dtype))


def test_wasserstein_1d():
    from expertsim import hip
    u, v = _columns(1, 3, np.float64), _columns(2, 3, np.float64)

    def run(seg, u_idx, v_idx):                          # no wrapper takes the output: the entry itself
        out = torch.full((len(SEG), 3), float("nan"), dtype=torch.float64, device=DEV)
        with torch.cuda.device(u.device):
            hip.call("es_wasserstein_1d", hip.ptr(u), u.stride(0), ROWS, hip.ptr(u_idx), hip.ptr(seg), hip.ptr(v),
                     v.stride(0), ROWS, hip.ptr(v_idx), hip.ptr(seg), len(SEG), 3, CAP, CAP, hip.ptr(out), None, 0,
                     hip.stream_ptr())
        return {"out": out}

    got = _both(run, _index(3), _index(4))["out"].cpu().numpy()
    assert (got[[2, 4]] == 0).all() and (got[[0, 1, 3], :2] > 0).all()   # an empty side gives 0


def test_segment_histogram():
    from expertsim.train.diagnostics import segment_histogram_raw
    x = _columns(5, 3, np.float64)

    def run(seg, idx):
        counts, edges, outside = segment_histogram_raw(x, seg, idx, CAP, bins=7, right=True)
        return {"counts": counts, "edges": edges, "outside": outside}

    got = _both(run, _index(6))
    assert got["counts"].sum(dim=2).cpu().tolist() == [[n] * 3 for n in (9, 12, 0, 12, 0)]


def test_segment_kde():
    from expertsim.train.diagnostics import segment_kde_raw
    x = _columns(7, 3, np.float64)
    got = _both(lambda seg, idx: segment_kde_raw(x, seg, idx, CAP, points=9, cols=2), _index(8))
    valid = got["valid"].cpu().numpy()
    assert valid.tolist() == [[1, 1], [1, 1], [0, 0], [1, 1], [0, 0]]
    assert torch.isnan(got["density"][[2, 4]]).all() and torch.isfinite(got["density"][[0, 1, 3]]).all()


def test_knn_radius_and_prdc_count():
    from expertsim.train.fidelity import knn_radius, prdc_raw
    real, fake = _columns(9, 5, np.float32), _columns(10, 5, np.float32)

    def radius(seg, idx):
        out = torch.full((len(SEG), CAP), float("nan"), dtype=torch.float64, device=DEV)
        return {"radius2": knn_radius(real, K, idx, seg, CAP, out=out)}

    def count(seg, r_idx, f_idx):
        return prdc_raw(real, fake, K, r_idx=r_idx, r_seg=seg, r_cap=CAP, f_idx=f_idx, f_seg=seg, f_cap=CAP)

    r2 = _both(radius, _index(11))["radius2"].cpu().numpy()
    lengths = (9, 12, 0, 12, 0)
    for s, n in enumerate(lengths):
        assert np.isfinite(r2[s, :n]).all() and np.isnan(r2[s, n:]).all()
    got = _both(count, _index(11), _index(12))
    assert got["totals"][:, :3].cpu().tolist() == [[n, n, 1 if n > K else 0] for n in lengths]
    for s, n in enumerate(lengths):
        assert (got["f_count"][s, n:] == -1).all() and (got["r_hit"][s, n:] == -1).all()
        assert torch.isnan(got["r_min2"][s, n:]).all() and (got["r_hit"][s, :n] >= 0).all()


def test_group_diversity():
    from expertsim.utils.data_preparation import diversity_raw
    x = _dev(np.random.RandomState(13).gamma(2.0, 3.0, (ROWS, 4, 4)).astype(np.float32))
    offs = np.array([-7, 5, 9, 64, 30, 18], dtype=np.int32)              # groups (b, e) = consecutive entries
    perm = _index(14)
    groups = S.members(ROWS, perm, np.stack([offs[:-1], offs[1:]], axis=1))
    assert [len(m) for m in groups] == [5, 4, 31, 0, 0]                   # registers, registers, chained, empty
    clean_perm = np.concatenate(groups).astype(np.int32)                  # every group's rows, listed
    clean_offs = np.concatenate([[0], np.cumsum([len(m) for m in groups])]).astype(np.int32)
    assert len(clean_perm) == ROWS and clean_offs[-1] == ROWS
    first = diversity_raw(x, _dev(perm), _dev(offs), len(groups), return_maps=True)
    second = diversity_raw(x, _dev(clean_perm), _dev(clean_offs), len(groups), return_maps=True)
    torch.cuda.synchronize()
    _same(first[0], second[0], "group_sum")
    _same(first[1], second[1], "pix_var")
    assert (first[0][:3] > 0).all() and (first[0][3:] == 0).all()
