"""Host-side checks of the sample-level fidelity feature (no GPU): the numpy restatement (tests/prdc_refs.py)
against scikit-learn's record (tests/golden/prdc_sklearn.npz), the restatement's invariants, the C ABI entries, the
argument checks that return before any launch, the configuration keys and the CLI flags.

Bounds against the record: the integer totals equal (the tool asserted a gap of at least 1000 B around every
strict comparison); the squared radii within B = (cols + 3) 2^-52 4 max|x|^2, the rounding bound of scikit-learn's
expansion form (prdc_refs.bound)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prdc_refs as R
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
ENTRIES = {"es_knn_radius": "int", "es_prdc_count": "int", "es_knn_radius_workspace": "size_t",
           "es_prdc_workspace": "size_t"}


def _prototype(name, res="int"):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("arch", list(R.ARCHS))
def test_recipe_reproduces_the_recorded_inputs(golden, arch):
    real, fake, e_r, e_f = R.make_inputs(arch)
    for name, v in (("real", real), ("fake", fake), ("expert_r", e_r), ("expert_f", e_f)):
        assert np.array_equal(golden[f"{arch}_{name}"], v) and golden[f"{arch}_{name}"].dtype == v.dtype, name
    assert real.shape[0] == R.ARCHS[arch][0] and fake.shape[0] == R.ARCHS[arch][1]
    assert (real == 0).mean() > 0.9                              # sparse images: the record compresses
    assert os.path.getsize(R.GOLDEN) < 512 * 1024


@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("arch", list(R.ARCHS))
def test_restatement_reproduces_sklearn(golden, arch, k):
    real, fake = golden[f"{arch}_real"], golden[f"{arch}_fake"]
    m_r = R.members(golden[f"{arch}_expert_r"], R.N_EXPERTS)
    m_f = R.members(golden[f"{arch}_expert_f"], R.N_EXPERTS)
    totals = golden[f"{arch}_k{k}_totals"]
    assert totals.shape == (R.N_EXPERTS + 1, 8) and totals.dtype == np.int64
    valid = []
    for s, (ir, jf) in enumerate(zip(m_r, m_f)):
        a, b = real[ir], fake[jf]
        seg = R.segment(a, b, k)
        assert np.array_equal(seg["totals"], totals[s]), (s, seg["totals"], totals[s])
        valid.append(bool(totals[s, 2]))
        if totals[s, 2]:
            B = R.bound(a, b)
            assert np.abs(seg["r_radius2"] - golden[f"{arch}_k{k}_s{s}_r_radius2"]).max() <= B
            assert np.abs(seg["f_radius2"] - golden[f"{arch}_k{k}_s{s}_f_radius2"]).max() <= B
            assert R.min_gap(a, b, k) >= 1000.0 * B
            assert np.isfinite(R.metrics(totals[s], k)).all()
        else:
            assert np.isnan(R.metrics(totals[s], k)).all() and not totals[s, 3:].any()
    assert valid == [True, False, k < 9, True]                   # expert 0 empty, expert 1 of 12 x 9 rows


def test_restatement_invariants():
    rs = np.random.RandomState(5)
    a = (rs.rand(23, 37) * (rs.rand(23, 37) < 0.3)).astype(np.float32)
    b = (rs.rand(19, 37) * (rs.rand(19, 37) < 0.3)).astype(np.float32)
    assert (np.diag(R.d2(a, a)) == 0).all()                      # exactly zero self-distance
    assert np.array_equal(R.d2(a, b).view(np.int64), R.d2(b, a).T.copy().view(np.int64))   # bitwise symmetry
    assert (R.radius2(a[:5], 5) == np.inf).all() and np.isfinite(R.radius2(a[:6], 5)).all()
    same = np.repeat(b[:1], 19, axis=0)                          # a fully collapsed generator
    seg = R.segment(a, same, 3)
    assert (seg["f_radius2"] == 0).all() and (seg["r_hit"] == 0).all() and seg["totals"][4] == 0
    assert np.isnan(R.metrics(R.segment(a[:3], b, 3)["totals"], 3)).all()
    # one real row among its own copies: every count by hand
    seg = R.segment(np.repeat(a[:1], 4, axis=0), np.repeat(a[:1], 4, axis=0), 2)
    assert seg["totals"].tolist() == [4, 4, 1, 0, 0, 0, 0, 0]    # radii 0 and strict comparisons: nothing is inside


def test_metrics_from_totals_matches_the_restatement():
    from expertsim.train.fidelity import METRICS, metrics_dict, metrics_from_totals
    assert METRICS == ("precision", "recall", "density", "coverage")
    totals = np.array([[161, 149, 1, 33, 28, 1139, 150, 0], [0, 0, 0, 0, 0, 0, 0, 0], [12, 9, 0, 0, 0, 0, 0, 0]])
    m = metrics_from_totals(totals, 5)
    assert m.dtype == np.float64 and m.shape == (3, 4)
    assert m[0].tolist() == [33 / 149, 28 / 161, 1139 / (5 * 149), 150 / 161] == list(R.metrics(totals[0], 5))
    assert np.isnan(m[1:]).all()
    d = metrics_dict(totals, 5, True)
    assert set(d) == {*METRICS, *[f"{n}_{e}" for n in METRICS for e in range(2)]}
    assert d["precision"] == 33 / 149 and np.isnan(d["coverage_1"])
    assert set(metrics_dict(totals[:1], 5, False)) == set(METRICS)


# ------------------------------------------------------------------------------------------ 2. ABI
def test_header_declares_the_entries():
    assert _prototype("es_knn_radius") == [
        "const float* x", "int64_t ld", "int rows", "int cols", "const int32_t* idx", "const int32_t* seg",
        "int n_seg", "int cap", "int k", "double* radius2", "void* work", "size_t work_bytes", "es_stream_t stream"]
    assert _prototype("es_prdc_count") == [
        "const float* real", "int64_t r_ld", "int r_rows", "const int32_t* r_idx", "const int32_t* r_seg",
        "int r_cap", "const float* fake", "int64_t f_ld", "int f_rows", "const int32_t* f_idx",
        "const int32_t* f_seg", "int f_cap", "int cols", "int n_seg", "int k", "const double* r_radius2",
        "const double* f_radius2", "int32_t* f_count", "int32_t* r_hit", "double* r_min2", "int64_t* totals",
        "void* work", "size_t work_bytes", "es_stream_t stream"]
    src = open(HEADER).read()
    doc = src[src.index("Sample-level fidelity and diversity"):src.index("size_t es_knn_radius_workspace")]
    for words in ("no contraction, no FMA", "d2(a, a) is exactly 0", "bitwise", "self included", "+inf",
                  "strict", "vector\n * atomics", "not written", "es_wasserstein_1d"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in ENTRIES.items():
        r, args = hip._SIGS[name]
        assert r is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(_prototype(name, res)), name
        assert hasattr(hip.lib(), name)
    src = open(HEADER).read()
    for macro, value in (("ES_KNN_MAX_K", hip.KNN_MAX_K), ("ES_KNN_MAX_COLS", hip.KNN_MAX_COLS),
                         ("ES_KNN_MAX_SEG", hip.KNN_MAX_SEG)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert (hip.KNN_MAX_K, hip.KNN_MAX_COLS, hip.KNN_MAX_SEG) == (16, 4096, 65)
    assert hip.KNN_MAX_ROWS == 1 << 20 and "#define ES_KNN_MAX_ROWS (1 << 20)" in src


def test_workspace_limits():
    from expertsim import hip
    kw, pw = hip.knn_radius_workspace, hip.prdc_workspace
    assert kw(1, 1, 1) > 0 and kw(65, 1 << 20, 16) > 0 and kw(5, 16384, 5) >= 5 * 16384 * 6 * 8
    for n_seg, cap, k in ((0, 4, 1), (66, 4, 1), (1, 0, 1), (1, (1 << 20) + 1, 1), (1, 4, 0), (1, 4, 17)):
        assert kw(n_seg, cap, k) == 0, (n_seg, cap, k)
    assert pw(1, 1, 1) > 0 and pw(65, 1 << 20, 1 << 20) >= 65 * (1 << 20) * 16
    for n_seg, r_cap, f_cap in ((0, 4, 4), (66, 4, 4), (1, 0, 4), (1, 4, 0), (1, (1 << 20) + 1, 4), (1, 4, (1 << 20) + 1)):
        assert pw(n_seg, r_cap, f_cap) == 0, (n_seg, r_cap, f_cap)


def test_entries_reject_bad_arguments_before_any_launch():
    from expertsim import hip
    f = C.c_void_p(256)
    big = 1 << 30

    def radius(x=f, ld=8, rows=16, cols=8, idx=None, seg=f, n_seg=1, cap=16, k=5, out=f, work=f, wb=big):
        return hip.call("es_knn_radius", x, ld, rows, cols, idx, seg, n_seg, cap, k, out, work, wb, None)

    def count(real=f, r_ld=8, r_rows=16, r_seg=f, r_cap=16, fake=f, f_ld=8, f_rows=16, f_seg=f, f_cap=16, cols=8,
              n_seg=1, k=5, rr=f, fr=f, totals=f, work=f, wb=big):
        return hip.call("es_prdc_count", real, r_ld, r_rows, None, r_seg, r_cap, fake, f_ld, f_rows, None, f_seg,
                        f_cap, cols, n_seg, k, rr, fr, None, None, None, totals, work, wb, None)

    bad = [lambda: radius(x=None), lambda: radius(seg=None), lambda: radius(out=None), lambda: radius(k=0),
           lambda: radius(k=17), lambda: radius(cols=4097, ld=4097), lambda: radius(cols=0), lambda: radius(ld=7),
           lambda: radius(rows=0), lambda: radius(rows=(1 << 20) + 1), lambda: radius(cap=0), lambda: radius(n_seg=0),
           lambda: radius(n_seg=66), lambda: radius(work=None), lambda: radius(wb=8),
           lambda: count(real=None), lambda: count(fake=None), lambda: count(r_seg=None), lambda: count(f_seg=None),
           lambda: count(rr=None), lambda: count(fr=None), lambda: count(totals=None), lambda: count(k=0),
           lambda: count(k=17), lambda: count(cols=4097, r_ld=4097, f_ld=4097), lambda: count(r_ld=7),
           lambda: count(f_ld=7), lambda: count(f_rows=0), lambda: count(r_cap=(1 << 20) + 1), lambda: count(n_seg=66),
           lambda: count(work=None), lambda: count(wb=8)]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError):
            fn()
        assert hip.lib().es_last_error(), i


# ------------------------------------------------------------------------------------------ 3. Python surface
def test_wrappers_need_a_device():
    import torch

    from expertsim import hip
    from expertsim.train import fidelity
    x = np.zeros((8, 4), dtype=np.float32)                        # host data: never copied to a device silently
    for fn in (lambda: fidelity.knn_radius(x, 2), lambda: fidelity.prdc_raw(x, x, 2), lambda: fidelity.prdc(x, x, 2),
               lambda: fidelity.prdc(torch.from_numpy(x), torch.from_numpy(x), k=2, expert=torch.zeros(8), n_experts=1)):
        with pytest.raises(hip.HipError):
            fn()


def test_eval_prdc_defaults_off_and_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    base = load_config()
    assert base.train.get("eval_prdc", None) is False and base.train.get("eval_prdc_k", None) == 5
    cfg = load_config(overrides=["train.eval_prdc=true"])
    assert cfg.train.eval_prdc is True and not cfg.train.eval_on_device

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_on_device"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")
    assert "batch size" in evaluate_epoch.__doc__ and "eval_prdc_k" in evaluate_epoch.__doc__


def test_evaluate_device_signature_defaults_off():
    import inspect

    from expertsim.models.moe import MoEWrapper
    p = inspect.signature(MoEWrapper.evaluate_device).parameters
    assert p["prdc"].default is False and p["prdc_k"].default == 5


def test_cli_flags():
    import cli
    a = cli.parse_args(["--simulate"])
    assert a.real is None and a.prdc_k == 5
    a = cli.parse_args(["--simulate", "--real", "r.npy", "--prdc-k", "3"])
    assert a.real == "r.npy" and a.prdc_k == 3
