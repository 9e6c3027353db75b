"""es_segment_quantiles, es_bin_dispatch and expertsim.train.conditional.profile on the device against the numpy
restatement and the record of numpy, pandas and scipy (tests/conditional_refs.py, whose docstring derives every bound;
tests/golden/conditional_numpy.npz).  Quantiles must be bit-equal to the restatement, bins and groupings are integers
and must be equal; the scalars print their error and bound before they are asserted.  The shapes are the smallest at
which each piece can go wrong: segment lengths on both sides of a wave, both sides of the LDS limit, chunk counts
1, 2 and 3 of the dispatch, the class limit."""
import ctypes as C

import numpy as np
import pytest
import torch

import conditional_refs as R
from distance_refs import moment_bounds

pytestmark = pytest.mark.gpu
DEV = "cuda"
PROBS16 = (0.84, 0.0, 0.5, 1.0, 0.16, 1.0 / 3.0, 0.5, 0.999, 0.001, 0.25, 0.75, 0.5, 0.9, 0.1, 2.0 / 3.0, 0.16)


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _seg(pairs):
    return torch.tensor(pairs, dtype=torch.int32, device=DEV).reshape(-1, 2)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


def _same_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, got, want)
    assert np.array_equal(_bits(got[~nan]), _bits(want[~nan])), (what, got, want)


def _table(rs, rows, ld):
    """Columns: continuous with negative values; integer-valued with heavy ties, -0.0 among the zeros; positive."""
    t = rs.randn(rows, ld) * 3.0
    t[:, 1] = np.round(rs.randn(rows))
    t[::7, 1] *= -1.0                                   # turns some +0.0 into -0.0
    t[:, 2] = rs.gamma(2.0, 300.0, rows)
    return t


# ------------------------------------------------------------------------------------------ es_segment_quantiles
def test_quantiles_segments_index_stride_and_canaries():
    from expertsim.train.conditional import segment_quantiles
    rs = np.random.RandomState(5)
    rows_u, rows_v, ch, ld = 1500, 1400, 3, 5
    u, v = _table(rs, rows_u, ld), _table(rs, rows_v, ld) + 0.25
    assert np.signbit(u[u[:, 1] == 0, 1]).any() and not np.signbit(u[u[:, 1] == 0, 1]).all()
    iu, iv = rs.permutation(rows_u).astype(np.int32), rs.permutation(rows_v).astype(np.int32)
    lens = (0, 1, 2, 63, 64, 65, 1000)
    useg = [[10, 10 + L] for L in lens] + [[-5, 40], [1400, 9999], [700, 600], [5, 5]]   # clamped, clamped, inverted
    vseg = [[3, 3 + L] for L in reversed(lens)] + [[0, 17], [1390, 1500], [0, 50], [9, 9]]   # overlapping, unequal sides
    n_seg = len(useg)
    ut, vt = _dev(u)[:, :ch], _dev(v)[:, :ch]                                # a row stride above `channels`
    assert ut.stride(0) == ld
    for probs in (PROBS16, (0.5,)):
        nq = len(probs)
        out = (torch.full((n_seg + 2, ch, 2, nq), -7.0, dtype=torch.float64, device=DEV),
               torch.full((n_seg + 2, 2), -7, dtype=torch.int32, device=DEV))
        q, cnt = segment_quantiles(ut, vt, probs, u_idx=_dev(iu), u_seg=_seg(useg), u_cap=1000, v_idx=_dev(iv),
                                   v_seg=_seg(vseg), v_cap=1000, out=out)
        host, hc = q.cpu().numpy(), cnt.cpu().numpy()
        assert (host[n_seg:] == -7).all() and (hc[n_seg:] == -7).all()       # canary rows beyond n_seg
        for s in range(n_seg):
            (ub, ue), (vb, ve) = useg[s], vseg[s]
            ub, vb = min(max(ub, 0), rows_u), min(max(vb, 0), rows_v)
            ue, ve = min(max(ue, ub), rows_u), min(max(ve, vb), rows_v)
            assert hc[s].tolist() == [ue - ub, ve - vb], s
            for c in range(ch):
                _same_bits(host[s, c, 0], R.quantiles(u[iu[ub:ue], c], probs), ("u", s, c))
                _same_bits(host[s, c, 1], R.quantiles(v[iv[vb:ve], c], probs), ("v", s, c))
        assert np.isnan(host[0, :, 0]).all() and np.isfinite(host[0, :, 1]).all()       # one side empty, the other right
        assert np.isnan(host[6, :, 1]).all() and np.isfinite(host[6, :, 0]).all()
        assert np.isnan(host[9, :, 0]).all() and np.isfinite(host[9, :, 1]).all()       # inverted bounds: empty
        assert np.isnan(host[10]).all() and hc[10].tolist() == [0, 0]                   # both empty
        again = segment_quantiles(ut, vt, probs, u_idx=_dev(iu), u_seg=_seg(useg), u_cap=1000, v_idx=_dev(iv),
                                  v_seg=_seg(vseg), v_cap=1000)
        assert torch.equal(again[0].view(torch.int64), q[:n_seg].view(torch.int64)) and torch.equal(again[1], cnt[:n_seg])
    # the restatement is np.quantile wherever no -0.0 is involved
    assert _bits(host[6, 0, 0, 0]) == _bits(np.quantile(u[iu[10:1010], 0], 0.5))
    # a cap below a segment's length cuts it
    cut, ccut = segment_quantiles(ut, vt, PROBS16, u_seg=_seg([[0, 500]]), u_cap=100, v_seg=_seg([[0, 500]]), v_cap=64)
    _same_bits(cut[0, 2, 0].cpu().numpy(), R.quantiles(u[:100, 2], PROBS16), "cut u")
    _same_bits(cut[0, 2, 1].cpu().numpy(), R.quantiles(v[:64, 2], PROBS16), "cut v")
    assert ccut.cpu().tolist() == [[100, 64]]
    print("quantiles over segments: bit-equal")


@pytest.mark.parametrize("nu,nv", [(4096, 4096), (4096, 4097), (20000, 13000)])
def test_quantiles_both_paths_and_one_sample(nu, nv):
    """u_cap + v_cap = 8192 is the last LDS problem, 8193 the first on the global path (two tiles); 33000 values take
    four tiles of a 65536 padding."""
    from expertsim import hip
    from expertsim.train.conditional import segment_quantiles
    assert (nu + nv <= hip.WS_LDS_MAX) == (hip.segment_quantiles_workspace(1, 2, nu, nv) == 0)
    rs = np.random.RandomState(nu + nv)
    u, v = _table(rs, nu, 3)[:, 1:], _table(rs, nv, 3)[:, 1:] * 1.5          # a tied column and a continuous one
    q, cnt = segment_quantiles(_dev(u), _dev(v), PROBS16)
    host = q.cpu().numpy()
    assert cnt.cpu().tolist() == [[nu, nv]]
    for c in range(2):
        _same_bits(host[0, c, 0], R.quantiles(u[:, c], PROBS16), ("u", c))
        _same_bits(host[0, c, 1], R.quantiles(v[:, c], PROBS16), ("v", c))
    _same_bits(host[0, 1, 0], np.quantile(u[:, 1], PROBS16), "np.quantile")
    q2, _ = segment_quantiles(_dev(u), _dev(v), PROBS16)
    assert torch.equal(q2.view(torch.int64), q.view(torch.int64))                        # a rerun is bit-equal
    # the one-sample form on the same path, and a side that is empty through its segment
    one, c1 = segment_quantiles(_dev(u), None, PROBS16, u_cap=nu + nv)
    _same_bits(one[0, :, 0].cpu().numpy(), host[0, :, 0], "one-sample")
    assert np.isnan(one[0, :, 1].cpu().numpy()).all() and c1.cpu().tolist() == [[nu, 0]]
    alone, c2 = segment_quantiles(_dev(u), _dev(v), PROBS16, v_seg=_seg([[5, 5]]))
    _same_bits(alone[0, :, 0].cpu().numpy(), host[0, :, 0], "v empty")
    assert np.isnan(alone[0, :, 1].cpu().numpy()).all() and c2.cpu().tolist() == [[nu, 0]]


def test_quantiles_reject_bad_arguments_and_write_nothing():
    from expertsim import hip
    from expertsim.train.conditional import segment_quantiles
    u = _dev(np.random.RandomState(0).randn(9000, 1))
    for probs in ((0.5, 1.5), (float("nan"),), tuple([0.5] * 17)):
        out = (torch.full((1, 1, 2, len(probs)), -7.0, dtype=torch.float64, device=DEV),
               torch.full((1, 2), -7, dtype=torch.int32, device=DEV))
        with pytest.raises(hip.HipError, match=r"failed \(1\)"):
            segment_quantiles(u, u, probs, out=out)
        assert (out[0] == -7).all() and (out[1] == -7).all()
    need = hip.segment_quantiles_workspace(1, 1, 9000, 9000)
    assert need == 32768 * 9
    out, cnt = torch.full((1, 1, 2, 1), -7.0, dtype=torch.float64, device=DEV), torch.full((1, 2), -7, dtype=torch.int32, device=DEV)
    work = torch.zeros(need - 1, dtype=torch.uint8, device=DEV)
    seg = _seg([[0, 9000]])
    half = (C.c_double * 1)(0.5)
    with pytest.raises(hip.HipError, match="workspace"):
        hip.call("es_segment_quantiles", hip.ptr(u), 1, 9000, None, hip.ptr(seg), hip.ptr(u), 1, 9000, None, hip.ptr(seg),
                 1, 1, 9000, 9000, C.cast(half, C.c_void_p), 1, hip.ptr(out), hip.ptr(cnt), hip.ptr(work), need - 1,
                 hip.stream_ptr())
    torch.cuda.synchronize()
    assert (out == -7).all() and (cnt == -7).all() and not work.any()


@pytest.mark.parametrize("nu,nv", [(700, 900), (5000, 4000)])
def test_quantiles_leave_wasserstein_and_rank_stats_alone(nu, nv):
    """The sort's kernels gained a template parameter: the instantiations of wasserstein.hip and rank.hip must give
    the bits they gave, before and after an es_segment_quantiles call, on both paths."""
    from scipy.stats import wasserstein_distance

    from classifier_refs import rank_stats as rank_ref
    from expertsim.train.classifier import rank_stats
    from expertsim.train.conditional import segment_quantiles
    from expertsim.train.utils import wasserstein_1d_device
    u, v = np.random.RandomState(1).randn(nu), np.round(np.random.RandomState(2).randn(nv), 1)
    ut, vt = _dev(u[:, None]), _dev(v[:, None])
    ws0, rk0 = wasserstein_1d_device(ut, vt).clone(), rank_stats(ut, vt).clone()
    q, _ = segment_quantiles(ut, vt, (0.5,))
    ws1, rk1 = wasserstein_1d_device(ut, vt), rank_stats(ut, vt)
    assert torch.equal(ws0.view(torch.int64), ws1.view(torch.int64)) and torch.equal(rk0, rk1)
    assert tuple(int(x) for x in rk1.cpu().reshape(4)) == rank_ref(u, v)
    ref = wasserstein_distance(u, v)
    err, bound = abs(float(ws1[0, 0]) - ref), 2 * (nu + nv) * 2.0 ** -52 * ref
    print(f"wasserstein around segment_quantiles: bit-equal, error / bound {err / bound:.3f}")
    assert err <= bound
    _same_bits(q[0, 0].cpu().numpy().reshape(2), [np.quantile(u, 0.5), np.quantile(v, 0.5)], "medians")


# ------------------------------------------------------------------------------------------ es_bin_dispatch
def _edges(kind, n_bins, x, rs):
    if n_bins == 1:
        return np.zeros(0)
    if kind == "data":                                  # edges that ARE values of x: rows exactly on an edge
        e = np.sort(rs.choice(x, n_bins - 1, replace=True))
    elif kind == "repeated":                            # equal neighbours: empty bins
        e = np.sort(np.repeat(rs.choice(x, (n_bins + 1) // 2, replace=True), 2)[:n_bins - 1])
    else:                                               # all rows in one bin
        e = np.full(n_bins - 1, x.max() + 1.0)
    return e.astype(np.float64)


def _check_dispatch(x_host, x_dev, edges, n_bins, expert=None, E=1, what=""):
    from expertsim.train.conditional import bin_dispatch
    ed = _dev(edges) if n_bins > 1 else None
    ex = _dev(expert) if expert is not None else None
    bins, perm, offs = bin_dispatch(x_dev, ed, n_bins, ex, E)
    want_bin = np.searchsorted(edges, x_host.astype(np.float64), side="left")
    assert (want_bin == R.bin_of(edges, x_host)).all()
    n_classes = n_bins * (E if expert is not None else 1)
    want_perm, want_offs = R.grouping(R.classes(want_bin, n_bins, expert, E), n_classes)
    assert bins.cpu().numpy().tolist() == want_bin.tolist(), what
    assert offs.cpu().numpy().tolist() == want_offs.tolist(), what
    assert perm.cpu().numpy().tolist() == want_perm.tolist(), what
    again = bin_dispatch(x_dev, ed, n_bins, ex, E)
    assert all(torch.equal(a, b) for a, b in zip(again, (bins, perm, offs))), what
    return want_bin


@pytest.mark.parametrize("rows", [1, 1023, 1024, 1025, 3000])
def test_bin_dispatch_matches_searchsorted_and_stable_argsort(rows):
    rs = np.random.RandomState(rows)
    table = np.round(rs.randn(rows, 3) * 4.0, 1)                                # a coarse grid: many values on edges
    x64, x32 = table[:, 1].copy(), table.astype(np.float32)[:, 2].copy()
    t64, t32 = _dev(table), _dev(table.astype(np.float32))
    expert = rs.randint(-2, 7, rows).astype(np.int32)                          # out of range on both sides: clamped
    on_edge = empty = 0
    for n_bins in (1, 2, 8, 64):
        for kind in ("data", "repeated", "one"):
            e = _edges(kind, n_bins, x64, rs)
            b = _check_dispatch(x64, t64[:, 1], e, n_bins, what=(rows, n_bins, kind, "f64"))           # ld = 3
            on_edge += int(np.isin(x64, e).sum())
            empty += int((np.bincount(b, minlength=n_bins) == 0).sum())
            _check_dispatch(x64, t64[:, 1], e, n_bins, expert, 4, what=(rows, n_bins, kind, "f64", "E4"))
            e32 = _edges(kind, n_bins, x32.astype(np.float64), rs)
            _check_dispatch(x32, t32[:, 2], e32, n_bins, what=(rows, n_bins, kind, "f32"))
    assert on_edge > 0 and empty > 0
    if rows == 3000:                                                            # the class limit: 16 experts x 64 bins
        ex16 = rs.randint(0, 16, rows).astype(np.int32)
        _check_dispatch(x64, t64[:, 1], _edges("data", 64, x64, rs), 64, ex16, 16, what="1024 classes")
    print("bin_dispatch rows", rows, ": integers equal")


def test_bin_dispatch_rejects_bad_arguments():
    from expertsim import hip
    from expertsim.train.conditional import bin_dispatch
    x = _dev(np.linspace(0.0, 1.0, 50))
    expert = torch.zeros(50, dtype=torch.int32, device=DEV)
    out = tuple(torch.full((n,), -7, dtype=torch.int32, device=DEV) for n in (50, 50, 1100))
    for n_bins, ex, E in ((65, None, 1), (41, expert, 25)):
        with pytest.raises(hip.HipError, match=r"failed \(1\)"):
            bin_dispatch(x, _dev(np.linspace(0.1, 0.9, n_bins - 1)), n_bins, ex, E, out=out)
        assert all((t == -7).all() for t in out)
    with pytest.raises(ValueError):
        bin_dispatch(x, _dev(np.linspace(0.1, 0.9, 3)), 8)


def test_bin_edges_are_np_quantile():
    from expertsim.train.conditional import bin_edges
    rs = np.random.RandomState(3)
    by32 = rs.randn(777).astype(np.float32)
    cond = _dev(np.stack([by32, by32 * 2], axis=1))
    for n_bins in (1, 2, 8, 17, 64):                                           # 64: four calls of at most 16 edges
        got = bin_edges(cond[:, 0], n_bins)
        want = np.quantile(by32.astype(np.float64), [k / n_bins for k in range(1, n_bins)]) if n_bins > 1 else np.zeros(0)
        assert got.dtype == torch.float64 and got.is_cuda
        _same_bits(got.cpu().numpy(), want, n_bins)


# ------------------------------------------------------------------------------------------ profile
def _check_tables(p, t, real, fake, what):
    """The device tables p of profile(details=True) against the reference tables t; returns worst error / bound."""
    _same_bits(p["edges"].cpu().numpy(), t["edges"], (what, "edges"))
    assert p["bin"].cpu().numpy().tolist() == t["bin"].tolist(), what
    assert p["count"].cpu().numpy().tolist() == t["count"].tolist(), what
    for k in ("q_real", "q_gen", "scale"):
        _same_bits(p[k].cpu().numpy(), t[k], (what, k))
    ws, ks, count = p["ws"].cpu().numpy(), p["ks"].cpu().numpy(), t["count"]
    worst = 0.0
    for s in range(count.shape[0]):
        for b in range(count.shape[1]):
            n = int(count[s, b])
            bound = 4 * n * 2.0 ** -52 * t["ws"][s, b]
            err = np.abs(ws[s, b] - t["ws"][s, b])
            assert (err <= bound).all(), (what, s, b, err, bound)
            assert (np.abs(ks[s, b] - t["ks"][s, b]) <= 3 * R.U).all(), (what, s, b)
            if (bound > 0).any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
    mean_r, std_r = p["mean_real"].cpu().numpy(), p["std_real"].cpu().numpy()
    rows = t["bin"]
    for b in range(count.shape[1]):                                             # the joint bins' moments
        x = real[rows == b]
        if len(x) < 2:
            continue
        mb, cb = moment_bounds(x)
        assert (np.abs(mean_r[0, b] - x.mean(axis=0)) <= mb).all(), (what, b)
        var = x.var(axis=0, ddof=1)
        assert (np.abs(std_r[0, b] ** 2 - var) <= np.diag(cb) + 4 * R.U * var).all(), (what, b)
    assert np.isnan(p["q_gen"].cpu().numpy()[count == 0]).all() and (ws[count == 0] == 0).all()
    return worst


@pytest.mark.parametrize("case", ["redraw", "shuffled", "experts"])
def test_profile_against_the_record(case, golden):
    from expertsim.train.conditional import profile
    by, real, redraw, shuffled, expert = R.fixture()
    fake = shuffled if case == "shuffled" else redraw
    ex, E = (_dev(expert), 3) if case == "experts" else (None, 1)
    t = R.golden_tables(golden, case)
    p = profile(_dev(real), _dev(fake), _dev(by), R.BINS, ex, E, names=R.NAMES, details=True)
    worst = _check_tables(p, t, real, fake, case)
    worst = max(worst, R.check_scalars(p, t, R.NAMES, E if ex is not None else 0, case))
    print(f"profile {case}: worst error / bound {worst:.3f}")
    again = profile(_dev(real), _dev(fake), _dev(by), R.BINS, ex, E, names=R.NAMES)
    assert all(v == p[k] or (np.isnan(v) and np.isnan(p[k])) for k, v in again.items())
    if case == "experts":                                                       # an expert that owns no row
        joint = profile(_dev(real), _dev(fake), _dev(by), R.BINS, names=R.NAMES)
        assert all(p[k] == v for k, v in joint.items())                         # ... and nothing else moves
        assert np.isnan(p["cond_ws_1"]) and all(np.isnan(p[f"cond_ws_{o}_1"]) for o in R.NAMES)
        assert np.isfinite(p["cond_ws_0"]) and np.isfinite(p["cond_ws_2"])
        assert p["count"][2].sum().item() == 0 and p["count"].shape == (4, R.BINS)


def test_shuffled_conditions_fool_the_marginal_distance_only(golden):
    """The property behind the feature: generated rows that are the real rows shuffled across the conditions are at
    marginal distance exactly 0 in every column, and their conditional distance of the column that follows the
    condition is the record's, at least five times that of an independent redraw."""
    from expertsim.train.conditional import profile
    from expertsim.train.utils import wasserstein_1d_device
    by, real, redraw, shuffled, _ = R.fixture()
    assert (wasserstein_1d_device(_dev(real), _dev(shuffled)) == 0).all()
    sh = profile(_dev(real), _dev(shuffled), _dev(by), R.BINS, names=R.NAMES)
    rd = profile(_dev(real), _dev(redraw), _dev(by), R.BINS, names=R.NAMES)
    rec_sh, rec_rd = R.golden_tables(golden, "shuffled"), R.golden_tables(golden, "redraw")
    for got, rec in ((sh, rec_sh), (rd, rec_rd)):
        ref = rec["scalars"]["cond_ws_lin"]
        assert abs(got["cond_ws_lin"] - ref) <= R.bound("ws", ref, rec)
    assert rec_sh["scalars"]["cond_ws_lin"] >= 5 * rec_rd["scalars"]["cond_ws_lin"]
    assert sh["cond_ws_lin"] >= 5 * rd["cond_ws_lin"]
    print("cond_ws_lin shuffled", sh["cond_ws_lin"], "redraw", rd["cond_ws_lin"])


# ------------------------------------------------------------------------------------------ wiring
def _bytes(t):
    return t.contiguous().view(torch.uint8)


def running_stats(n, expert):
    i = np.arange(n, dtype=np.float64)
    return ((0.1 * np.sin(0.37 * i + expert)).astype(np.float32),
            (0.75 + 0.25 * np.cos(0.11 * i + 2 * expert)).astype(np.float32))


def _cfg(E, extra=()):
    from expertsim.config import load_config
    return load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                  f"model.n_experts={E}", "train.precision=fp32", "model.router.diff_strength=1e-6",
                                  *extra])


def _moe(E, extra=(), seed=4):
    from expertsim.train.loop import setup_moe_system
    cfg = _cfg(E, extra)
    torch.manual_seed(seed)
    moe = setup_moe_system(cfg, torch.device(DEV))
    with torch.no_grad():   # distinct, non-trivial running statistics per expert
        for e, g in enumerate(moe.generators):
            for m in g.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    mean, var = running_stats(m.num_features, e)
                    m.running_mean.copy_(torch.from_numpy(mean))
                    m.running_var.copy_(torch.from_numpy(var))
    moe.eval()
    return moe, cfg


def _batch(n):
    from expertsim.utils.synthetic import make_batch
    b = make_batch(n, "neutron", seed=11)
    return b, torch.from_numpy(b["real_images"]), torch.from_numpy(b["cond"]).to(DEV)


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


TABLE_KEYS = {"cond_obs_real", "cond_obs_gen", "cond_edges", "cond_count", "cond_q_real", "cond_q_gen", "cond_mean_real",
              "cond_mean_gen", "cond_std_real", "cond_std_gen", "cond_ws_bins", "cond_ks_bins", "cond_scale", "cond_bin"}


@pytest.mark.parametrize("E", [1, 3])
def test_evaluate_device_conditional(E):
    from expertsim.train import conditional as K
    from expertsim.train.distances import OBSERVABLE_NAMES
    N, B, seed, col = 256, 4, 17, 0
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    keys = set(K.scalar_keys(OBSERVABLE_NAMES, E))
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, conditional=True, conditional_bins=B,
                              conditional_column=col)
    assert set(det) == set(plain) | keys | TABLE_KEYS
    for key, v in plain.items():                                                   # bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(_bytes(det[key]), _bytes(v)), key
        else:
            assert det[key] == v, key
    assert tuple(det["cond_obs_real"].shape) == (N, 10) and det["cond_obs_real"].dtype == torch.float64
    assert torch.equal(det["cond_obs_real"][:, :5], det["sums_real"])
    assert torch.equal(det["cond_obs_gen"][:, :5], det["sums_gen"][0])
    assert tuple(det["cond_count"].shape) == (1 + E, B) and int(det["cond_count"][0].sum()) == N
    assert tuple(det["cond_q_real"].shape) == (1 + E, B, 10, 3) and tuple(det["cond_bin"].shape) == (N,)
    want = K.profile(det["cond_obs_real"], det["cond_obs_gen"], cond[:, col], B, det["expert"], E,
                     names=OBSERVABLE_NAMES, details=True)
    assert all(_same_float(det[k], want[k]) for k in keys) and np.isfinite(det["cond_ws"])
    assert torch.equal(_bytes(det["cond_q_gen"]), _bytes(want["q_gen"])) and torch.equal(det["cond_bin"], want["bin"])
    # the tables are the numpy restatement's on the host copies of the same observables
    t = R.profile(det["cond_obs_real"].cpu().numpy(), det["cond_obs_gen"].cpu().numpy(), cond[:, col].cpu().numpy(),
                  B, det["expert"].cpu().numpy(), E, names=OBSERVABLE_NAMES)
    worst = _check_tables(want, t, det["cond_obs_real"].cpu().numpy(), det["cond_obs_gen"].cpu().numpy(), f"E={E}")
    worst = max(worst, R.check_scalars(det, t, OBSERVABLE_NAMES, E, f"E={E}"))
    print(f"evaluate_device conditional E={E}: worst error / bound {worst:.3f}")
    again = moe.evaluate_device(5, cond, x, cfg, seed=seed, conditional=True, conditional_bins=B)
    assert set(again) == (set(plain) - {"sums_real", "sums_gen", "expert", "ws"}) | keys
    assert all(_same_float(again[k], det[k]) for k in again)                      # a rerun is bit-equal
    both = moe.evaluate_device(5, cond, x, cfg, seed=seed, conditional=True, conditional_bins=B, distances=True,
                               classifier=True, classifier_degree=1, features=True)
    alone = moe.evaluate_device(5, cond, x, cfg, seed=seed, distances=True, classifier=True, classifier_degree=1,
                                features=True)
    assert set(both) == set(alone) | keys
    assert all(_same_float(both[k], alone[k]) for k in alone) and all(_same_float(both[k], det[k]) for k in keys)
    with pytest.raises(ValueError, match="conditional_column"):
        moe.evaluate_device(5, cond, x, cfg, seed=seed, conditional=True, conditional_column=99)


def test_evaluate_epoch_passes_the_conditional_keys():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train import conditional as K
    from expertsim.train.distances import OBSERVABLE_NAMES
    from expertsim.train.loop import evaluate_epoch
    E, N, bs = 3, 106, 48
    on = ("train.eval_on_device=true", "train.eval_conditional=true", "train.eval_conditional_bins=3",
          "train.eval_conditional_column=1")
    moe, cfg = _moe(E, extra=on)
    b, x, cond = _batch(N)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg, device=torch.device(DEV))
    cfg_off = _cfg(E, extra=("train.eval_on_device=true",))
    off = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_off, device=torch.device(DEV))
    keys = set(K.scalar_keys(OBSERVABLE_NAMES, E))
    assert set(out) == set(off) | keys and all(out[key] == off[key] for key in off)
    per = [moe.evaluate_device(0, cond[i:i + bs], x[i:i + bs], cfg, seed=int(cfg.train.rng_seed), sample_offset=i,
                               conditional=True, conditional_bins=3, conditional_column=1) for i in range(0, N, bs)]
    assert np.isfinite(out["cond_ws"])
    for key in keys:
        finite = [m[key] for m in per if np.isfinite(m[key])]
        if finite:
            assert out[key] == sum(finite) / len(finite), key
        else:
            assert np.isnan(out[key]), key
    # the column and the bin count reach the profile: the first batch's bins are numpy's of column 1, not of column 0
    det = moe.evaluate_device(0, cond[:bs], x[:bs], cfg, seed=int(cfg.train.rng_seed), conditional=True,
                              conditional_bins=3, conditional_column=1, details=True)
    c0, c1 = (b["cond"][:bs, j].astype(np.float64) for j in (0, 1))
    bins0, bins1 = (np.searchsorted(np.quantile(c, [1 / 3, 2 / 3]), c, side="left") for c in (c0, c1))
    assert det["cond_bin"].cpu().numpy().tolist() == bins1.tolist() != bins0.tolist()
    assert tuple(det["cond_count"].shape) == (1 + E, 3) and all(_same_float(det[k], per[0][k]) for k in keys)
    cfg_bad = _cfg(E, extra=("train.eval_conditional=true",))
    with pytest.raises(ValueError, match="train.eval_conditional needs train.eval_on_device"):
        evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_bad, device=torch.device(DEV))


def test_cli_simulate_real_conditional(tmp_path):
    import os
    import subprocess
    import sys

    from conftest import REPO
    from expertsim.train import conditional as K
    from expertsim.train import distances as dist
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    E, N, B = 3, 64, 3
    moe, cfg = _moe(E)
    models = tmp_path / "models"
    models.mkdir()
    save_checkpoint(str(models), 0, moe, *setup_optimizers(moe, cfg))
    b, x, _ = _batch(N)
    np.save(tmp_path / "cond.npy", b["cond"])
    np.save(tmp_path / "real.npy", b["real_images"])
    out = tmp_path / "sim.npz"
    r = subprocess.run([sys.executable, os.path.join(REPO, "cli.py"), "-o", "model.architecture=neutron",
                        "dataset.input_image_shape=[44,44]", f"model.n_experts={E}", "model.router.diff_strength=1e-6",
                        "--simulate", "--checkpoint", str(models), "--cond", str(tmp_path / "cond.npy"),
                        "--sim-batch-size", "16", "--real", str(tmp_path / "real.npy"), "--conditional",
                        "--conditional-bins", str(B), "--seed", "5", "--out", str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    keys = K.scalar_keys(dist.OBSERVABLE_NAMES, E)
    assert set(keys) | (TABLE_KEYS - {"cond_obs_real", "cond_obs_gen"}) | {"cond_column"} <= set(z.files)
    images, expert = torch.from_numpy(z["images"]).to(DEV), torch.from_numpy(z["expert"]).to(DEV)
    obs_real = dist.observables(x.to(DEV), log_domain=True)
    obs_gen = dist.observables(images, log_domain=False, sums=torch.from_numpy(z["sums"]).to(DEV))
    want = K.profile(obs_real, obs_gen, _dev(b["cond"][:, 0]), B, expert, E, names=dist.OBSERVABLE_NAMES, details=True)
    for key in keys:
        assert z[key].dtype == np.float64 and _same_float(float(z[key]), want[key]), key
        assert f"{key} = " in r.stdout
    assert z["cond_count"].shape == (1 + E, B) and int(z["cond_count"][0].sum()) == N and int(z["cond_column"]) == 0
    assert np.array_equal(z["cond_q_real"], want["q_real"].cpu().numpy(), equal_nan=True)
