"""Host-side checks of the distribution distances (no GPU): the numpy restatement (tests/distance_refs.py) against
the record of numpy / scipy / scikit-learn (tests/golden/distances_scipy.npz), the host halves of
expertsim.train.distances against np.polyfit / np.median / np.percentile on recorded tables, the C ABI entries
and the Python surface.  Bounds: tests/distance_refs.py's docstring."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import distance_refs as R
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
ENTRIES = {"es_segment_moments": "int", "es_frechet": "int", "es_mmd_poly": "int",
           "es_segment_moments_workspace": "size_t", "es_mmd_poly_workspace": "size_t"}


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _prototype(name, res="int"):
    src = open(HEADER).read()
    m = re.search(r"^%s %s\((.*?)\);" % (res, name), src, re.S | re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


# ------------------------------------------------------------------------------------------ 1. restatement, record
def test_moments_restatement_rules():
    rs = np.random.RandomState(0)
    x = rs.randn(65, 3)
    n, mean, cov = R.moments(x)
    assert n == 65 and np.array_equal(mean, x.mean(0)) and np.array_equal(cov, np.cov(x, rowvar=False))
    assert np.array_equal(cov, cov.T)
    n, mean, cov = R.moments(x[:1])
    assert n == 1 and np.array_equal(mean, x[0]) and np.isnan(cov).all() and cov.shape == (3, 3)
    n, mean, cov = R.moments(x[:0])
    assert n == 0 and np.isnan(mean).all() and np.isnan(cov).all()
    assert R.moments(x[:, :1])[2].shape == (1, 1)
    mb, cb = R.moment_bounds(x)
    assert mb.shape == (3,) and cb.shape == (3, 3) and (mb > 0).all() and (cb > 0).all()


def test_record_frechet_is_self_consistent(golden):
    for kind, cols in R.FRECHET_CASES:
        key = f"fr_{kind}_{cols}"
        a, b = R.frechet_case(kind, cols)
        (_, ma, ca), (_, mb, cb) = R.moments(a), R.moments(b)
        for name, v in (("mean_a", ma), ("cov_a", ca), ("mean_b", mb), ("cov_b", cb)):
            assert golden[f"{key}_{name}"].shape == v.shape
            np.testing.assert_allclose(golden[f"{key}_{name}"], v, rtol=1e-12, atol=1e-300)
        ma, ca, mb, cb = (golden[f"{key}_{n}"] for n in ("mean_a", "cov_a", "mean_b", "cov_b"))
        unit = R.frechet_unit(ma, ca, mb, cb)
        eigh = R.frechet_eigh(ma, ca, mb, cb)
        D = float(golden[f"{key}_D"])
        assert np.abs(eigh - golden[f"{key}_eigh"]).max() <= unit            # the same algorithm, the same bits in
        assert np.abs(golden[f"{key}_eigh"] - golden[f"{key}_sqrtm"]).max() <= D * unit * (1 + 1e-12)
        assert D <= 4.0 and (golden[f"{key}_cond"] <= 1e3).all()
        assert eigh[0] > 0 and abs(eigh[0] - (eigh[1] + eigh[2] - 2 * eigh[3])) <= unit
    same = R.frechet_eigh(ma, ca, ma, ca)
    assert abs(same[0]) <= 8 * R.frechet_unit(ma, ca, ma, ca) and same[1] == 0.0
    assert np.isnan(R.frechet_eigh(ma, np.full_like(ca, np.nan), mb, cb)).all()


def test_record_kernel_sums_match_the_restatement(golden):
    for i, (cols, m, n, degree) in enumerate(R.MMD_CASES):
        x, y = R.mmd_case(cols, m, n, degree)
        assert x.dtype == np.float32 and x.shape == (m, cols) and y.shape == (n, cols)
        assert np.array_equal(x, golden[f"mmd_{i}_x"]) and np.array_equal(y, golden[f"mmd_{i}_y"])
        sums, absum = R.poly_sums(x, y, degree)
        bound = R.poly_bound(m, n, cols, degree, absum)
        assert (np.abs(sums - golden[f"mmd_{i}_sums"]) <= bound).all(), i
    # the diagonal is left out by index: one row has no pair, two equal rows have two
    x = golden["mmd_2_x"]
    one, _ = R.poly_sums(x[:1], x[:1])
    assert one[0] == 0.0 and one[1] == 0.0 and one[2] > 0
    two, _ = R.poly_sums(np.repeat(x[:1], 2, 0), x[:1])
    k = (np.dot(x[0].astype(np.float64), x[0].astype(np.float64)) / x.shape[1] + 1.0) ** 4
    assert abs(two[0] - 2 * k) <= 8 * R.U * 2 * k
    assert (R.poly_sums(x[:0], x[:3])[0][[0, 2]] == 0).all()
    assert R.poly_terms(3, 5).tolist() == [6, 20, 15]


# ------------------------------------------------------------------------------------------ 2. host halves
def test_prefix_lengths():
    from expertsim.train.distances import prefix_lengths
    for L in (0, 1, 7, 19, 400, 16384):
        n = prefix_lengths(L, 10)
        assert n.tolist() == R.prefix_lengths(L, 10).tolist() and n[-1] == L and (np.diff(n) >= 0).all()
        assert abs(int(n[0]) - L / 2) <= 0.03 * L + 1
    assert prefix_lengths(400, 10).tolist() == [210, 231, 252, 273, 294, 315, 336, 357, 378, 400]


def test_fpd_host_half_against_polyfit(golden):
    from expertsim.train.distances import fpd_from_table, summary_dict
    tables = np.stack([golden[f"ex_s{s}_fpd_table"] for s in range(4)])
    got = fpd_from_table(tables, R.EXPERT_COLS)
    assert got.dtype == np.float64 and got.shape == (4, 3)
    assert np.isnan(got).all(axis=1).tolist() == golden["ex_fpd_nan"].tolist() == [False, False, True, True]
    for s in (0, 1):
        fd, n = tables[s, :, 0], tables[s, :, 1]
        coef, cov = np.polyfit(1.0 / n, fd, 1, cov=True)
        scale = np.abs(fd).max()
        assert abs(got[s, 0] - coef[1]) <= 1e-10 * scale and abs(got[s, 1] - np.sqrt(cov[1, 1])) <= 1e-8 * scale
        assert got[s, 2] == fd[-1]
        np.testing.assert_allclose(got[s], golden[f"ex_s{s}_fpd"], rtol=1e-8)
        assert 0 < got[s, 0] < got[s, 2]                                  # the 1 / n bias is positive
    # an exact line: intercept recovered, no residual
    n = R.prefix_lengths(1000, 10).astype(np.float64)
    line = np.stack([0.25 + 3.0 / n, n, n], axis=1)[None]
    a, err, full = fpd_from_table(line, 10)[0]
    assert abs(a - 0.25) <= 1e-12 and err <= 1e-12 and full == line[0, -1, 0]
    # n_0 <= cols on the generated side alone is not valid either
    short = line.copy()
    short[0, 0, 2] = 10
    assert np.isnan(fpd_from_table(short, 10)).all()
    d = summary_dict(got, None, True)
    assert set(d) == {"fpd", "fpd_err", "fd_full", *[f"{k}_{e}" for k in ("fpd", "fpd_err", "fd_full") for e in range(3)]}
    assert d["fpd"] == got[0, 0] and np.isnan(d["fpd_1"]) and np.isnan(d["fd_full_2"])


def test_kpd_host_half_against_numpy(golden):
    from expertsim.train.distances import KEYS, kpd_from_table, mmd2, summary_dict
    tables = np.stack([golden[f"ex_s{s}_kpd_table"] for s in range(4)])
    got = kpd_from_table(tables)
    assert got.shape == (4, 3)
    assert np.isnan(got).all(axis=1).tolist() == golden["ex_kpd_nan"].tolist() == [False, False, True, True]
    for s in (0, 1):
        t = tables[s]
        v = np.array([R.mmd2(row[:3], row[3], row[4]) for row in t])
        assert np.array_equal(mmd2(t[:, :3], t[:, 3:5]), v)
        q75, q25 = np.percentile(v[:-1], [75, 25])
        assert got[s].tolist() == [np.median(v[:-1]), 0.5 * (q75 - q25), v[-1]]
        assert got[s].tolist() == golden[f"ex_s{s}_kpd"].tolist()
        assert got[s, 2] > 0 and got[s, 1] >= 0
    assert np.isnan(mmd2(np.ones((1, 3)), np.array([[1, 5]]))).all()
    d = summary_dict(None, got, False)
    assert set(d) == {"kpd", "kpd_err", "mmd_full"}
    both = summary_dict(np.zeros((2, 3)), got[:2], True)
    assert set(both) == {*KEYS, *[f"{k}_0" for k in KEYS]}


# ------------------------------------------------------------------------------------------ 3. ABI
def test_header_declares_the_entries():
    assert _prototype("es_segment_moments") == [
        "const void* x", "int x_f64", "int64_t ld", "int rows", "int cols", "const int32_t* idx", "const int32_t* seg",
        "int n_seg", "int32_t* count", "double* mean", "double* cov", "void* work", "size_t work_bytes",
        "es_stream_t stream"]
    assert _prototype("es_frechet") == [
        "const double* mean_a", "const double* cov_a", "const double* mean_b", "const double* cov_b", "int n",
        "int cols", "double* out", "es_stream_t stream"]
    assert _prototype("es_mmd_poly") == [
        "const float* real", "int64_t r_ld", "int r_rows", "const int32_t* r_idx", "const int32_t* r_seg",
        "int r_cap", "const float* fake", "int64_t f_ld", "int f_rows", "const int32_t* f_idx",
        "const int32_t* f_seg", "int f_cap", "int cols", "int n_seg", "int degree", "double gamma", "double coef0",
        "double* sums", "int32_t* counts", "void* work", "size_t work_bytes", "es_stream_t stream"]
    src = open(HEADER).read()
    doc = src[src.index("Distances between the joint distributions"):src.index("size_t es_segment_moments_workspace")]
    for words in ("np.cov(rowvar=False)", "same bits", "NaN when n < 2", "NaN when n == 0", "cyclic Jacobi",
                  "excluded by member position", "No float atomics", "bit-equal", "es_wasserstein_1d"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in ENTRIES.items():
        assert name in hip._SIGS, name
        r, args = hip._SIGS[name]
        assert r is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(_prototype(name, res)), name
        assert hasattr(hip.lib(), name)
    src = open(HEADER).read()
    for macro, value in (("ES_DIST_MAX_SEG", hip.DIST_MAX_SEG), ("ES_MOMENTS_MAX_COLS", hip.MOMENTS_MAX_COLS),
                         ("ES_MMD_MAX_COLS", hip.MMD_MAX_COLS), ("ES_MMD_MAX_DEGREE", hip.MMD_MAX_DEGREE)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert hip.DIST_MAX_ROWS == 1 << 20 and "#define ES_DIST_MAX_ROWS (1 << 20)" in src
    mk = open(os.path.join(REPO, "generative-dnn-for-physics-simulations-cern_amd", "csrc", "Makefile")).read()
    assert "distance.hip" in mk


def test_workspace_limits():
    from expertsim import hip
    mw, pw = hip.segment_moments_workspace, hip.mmd_poly_workspace
    assert mw(1, 1) > 0 and mw(1024, 32) >= 1024 * 16 * (32 + 528) * 8
    for n_seg, cols in ((0, 4), (1025, 4), (1, 0), (1, 33)):
        assert mw(n_seg, cols) == 0, (n_seg, cols)
    assert pw(1, 1, 1) > 0 and pw(55, 16384, 16384) >= 3 * 55 * 128 * 8
    for n_seg, r_cap, f_cap in ((0, 4, 4), (1025, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 20) + 1, 4)):
        assert pw(n_seg, r_cap, f_cap) == 0, (n_seg, r_cap, f_cap)


def test_entries_reject_bad_arguments_before_any_launch():
    from expertsim import hip
    f = C.c_void_p(256)
    big = 1 << 30

    def moments(x=f, ld=8, rows=16, cols=8, seg=f, n_seg=1, count=f, mean=f, cov=f, work=f, wb=big):
        return hip.call("es_segment_moments", x, 0, ld, rows, cols, None, seg, n_seg, count, mean, cov, work, wb, None)

    def frechet(ma=f, ca=f, mb=f, cb=f, n=1, cols=8, out=f):
        return hip.call("es_frechet", ma, ca, mb, cb, n, cols, out, None)

    def mmd(real=f, r_ld=8, r_rows=16, r_seg=f, r_cap=16, fake=f, f_ld=8, f_rows=16, f_seg=f, f_cap=16, cols=8,
            n_seg=1, degree=4, sums=f, counts=f, work=f, wb=big):
        return hip.call("es_mmd_poly", real, r_ld, r_rows, None, r_seg, r_cap, fake, f_ld, f_rows, None, f_seg, f_cap,
                        cols, n_seg, degree, 0.125, 1.0, sums, counts, work, wb, None)

    bad = [lambda: moments(x=None), lambda: moments(seg=None), lambda: moments(count=None), lambda: moments(mean=None),
           lambda: moments(cov=None), lambda: moments(cols=0), lambda: moments(cols=33, ld=33), lambda: moments(ld=7),
           lambda: moments(rows=0), lambda: moments(rows=(1 << 20) + 1), lambda: moments(n_seg=0),
           lambda: moments(n_seg=1025), lambda: moments(work=None), lambda: moments(wb=8),
           lambda: frechet(ma=None), lambda: frechet(cb=None), lambda: frechet(out=None), lambda: frechet(n=0),
           lambda: frechet(n=1025), lambda: frechet(cols=0), lambda: frechet(cols=33),
           lambda: mmd(real=None), lambda: mmd(fake=None), lambda: mmd(r_seg=None), lambda: mmd(f_seg=None),
           lambda: mmd(sums=None), lambda: mmd(counts=None), lambda: mmd(degree=0), lambda: mmd(degree=9),
           lambda: mmd(cols=65, r_ld=65, f_ld=65), lambda: mmd(cols=0), lambda: mmd(r_ld=7), lambda: mmd(f_ld=7),
           lambda: mmd(f_rows=0), lambda: mmd(r_cap=(1 << 20) + 1), lambda: mmd(f_cap=0), lambda: mmd(n_seg=1025),
           lambda: mmd(work=None), lambda: mmd(wb=8)]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError):
            fn()
        assert hip.lib().es_last_error(), i


# ------------------------------------------------------------------------------------------ 4. Python surface
def test_wrappers_need_a_device():
    import torch

    from expertsim import hip
    from expertsim.train import distances as D
    x = np.zeros((8, 4), dtype=np.float32)                        # host data: never copied to a device silently
    t = torch.from_numpy(x)
    for fn in (lambda: D.segment_moments(x), lambda: D.frechet(x[0], x[:4], x[0], x[:4]), lambda: D.mmd_poly_sums(x, x),
               lambda: D.fpd(t, t), lambda: D.kpd(t, t), lambda: D.distances(t, t, torch.zeros(8), 1)):
        with pytest.raises(hip.HipError):
            fn()


def test_names_and_normalise():
    import torch

    from expertsim.train import distances as D
    from expertsim.train.utils import FEATURE_NAMES
    assert len(D.OBSERVABLE_NAMES) == 10 and D.OBSERVABLE_NAMES[5:] == tuple(FEATURE_NAMES)
    assert D.KEYS == ("fpd", "fpd_err", "fd_full", "kpd", "kpd_err", "mmd_full")
    real = torch.tensor([[1.0, -4.0, 0.0], [2.0, 2.0, 0.0]], dtype=torch.float64)
    fake = torch.tensor([[4.0, 8.0, 3.0]], dtype=torch.float64)
    r, f, scale = D.normalise(real, fake)                          # plain torch: runs where the tensors are
    assert scale.tolist() == [2.0, 4.0, 1.0] and r.dtype == torch.float64
    assert r.tolist() == [[0.5, -1.0, 0.0], [1.0, 0.5, 0.0]] and f.tolist() == [[2.0, 2.0, 3.0]]


def test_eval_distances_defaults_off_and_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    assert load_config().train.get("eval_distances", None) is False
    cfg = load_config(overrides=["train.eval_distances=true"])
    assert cfg.train.eval_distances is True and not cfg.train.eval_on_device

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_distances needs train.eval_on_device"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")
    assert "eval_distances" in evaluate_epoch.__doc__


def test_signature_and_cli_flag_default_off():
    import inspect

    import cli
    from expertsim.models.moe import MoEWrapper
    assert inspect.signature(MoEWrapper.evaluate_device).parameters["distances"].default is False
    assert cli.parse_args(["--simulate"]).distances is False
    assert cli.parse_args(["--simulate", "--real", "r.npy", "--distances"]).distances is True
