"""Host-side checks of the conditional profiles (no GPU): csrc/quantile_rule.h compiled host-only
(tests/quantile_main.hip) against np.quantile and np.searchsorted bit for bit, the numpy restatement
(tests/conditional_refs.py) and the host half of expertsim.train.conditional against the record of numpy, pandas and
scipy (tests/golden/conditional_numpy.npz), the C ABI entries and the Python surface.  Bounds: conditional_refs'
docstring."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import conditional_refs as R
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
CSRC = os.path.join(REPO, "generative-dnn-for-physics-simulations-cern_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ENTRIES = {"es_segment_quantiles": "int", "es_bin_dispatch": "int", "es_segment_quantiles_workspace": "size_t",
           "es_bin_dispatch_workspace": "size_t"}
PS = (0.0, 1.0, 0.5, 0.16, 0.84, 1.0 / 3.0)


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    """run(lines) -> the output lines of the host-only program on those input lines."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.fail("hipcc not found: the header is compiled host-only with it")
    exe = str(tmp_path_factory.mktemp("quantile") / "quantile_main")
    cmd = [HIPCC, "-O1", "-std=c++17", "--offload-host-only", "-Wall", "-I" + CSRC,
           os.path.join(REPO, "tests", "quantile_main.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert r.returncode == 0, "the program rejected its input"
        return [line.split() for line in r.stdout.splitlines()]

    return run


def _prototype(name, res="int"):
    src = open(HEADER).read()
    m = re.search(r"^%s %s\((.*?)\);" % (res, name), src, re.S | re.M)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------ 1. the compiled rules
def _quantile_cases():
    rng = np.random.default_rng(5)
    cases = []
    for n in (1, 2, 3, 64, 65):
        cases.append(rng.normal(0.0, 3.0, n))                                 # negative values too
        cases.append(np.round(rng.normal(0.0, 2.0, n)))                       # heavy ties
        cases.append(rng.gamma(2.0, 300.0, n))
    cases.append(np.array([7.5] * 9))
    cases.append(np.array([-1e300, -2.5, 0.0, 1e-300, 2.5, 1e300]))
    return cases


def test_compiled_quantile_rule_is_np_quantile_bit_for_bit(rule):
    cases = [(np.sort(x), p) for x in _quantile_cases() for p in PS]
    lines = [f"Q {float(p).hex()} {x.size} " + " ".join(float(v).hex() for v in x) for x, p in cases]
    out = rule(lines)
    assert len(out) == len(cases)
    for (x, p), line in zip(cases, out):
        got = float.fromhex(line[1])
        want = float(np.quantile(x, p))
        assert _bits(got) == _bits(want), (x.size, p, got, want)
        assert _bits(R.quantile(x, p)) == _bits(want), (x.size, p)            # the numpy restatement too


def test_compiled_bin_rule_is_np_searchsorted(rule):
    rng = np.random.default_rng(6)
    edge_sets = [np.array([]), np.array([0.25]), np.array([-1.0, 0.0, 0.0, 2.5]),          # repeated edges
                 np.sort(rng.normal(0.0, 1.0, 7)), np.sort(rng.normal(0.0, 1.0, 63)), np.array([3.0] * 5)]
    cases = []
    for e in edge_sets:
        xs = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf), rng.normal(0.0, 1.5, 20),
                             [-1e300, 1e300, 0.0, -0.0]])
        cases += [(e, float(x)) for x in xs]
    lines = [f"B {x.hex()} {e.size} " + " ".join(float(v).hex() for v in e) for e, x in cases]
    out = rule(lines)
    assert len(out) == len(cases)
    on_edge = 0
    for (e, x), line in zip(cases, out):
        want = int(np.searchsorted(e, x, side="left"))
        assert int(line[1]) == want == int(R.bin_of(e, [x])[0]), (e, x)
        on_edge += int(x in e)
    assert on_edge >= 80                                                       # values exactly on an edge were tried
    # a value equal to an edge belongs to the lower bin; a repeated edge leaves an empty bin behind it
    assert [int(v[1]) for v in rule(["B 0x0p+0 4 -0x1p+0 0x0p+0 0x0p+0 0x1.4p+1", "B 0x1p-1074 4 -0x1p+0 0x0p+0 0x0p+0 "
                                     "0x1.4p+1"])] == [1, 3]


def test_compiled_class_and_probability_rules(rule):
    lines, want = [], []
    for e in (-3, 0, 1, 3, 4, 9):
        for b in (0, 5, 7):
            lines.append(f"C {b} 8 {e} 4")
            want.append(min(max(e, 0), 3) * 8 + b)
    assert [int(v[1]) for v in rule(lines)] == want
    probs = [0.0, 1.0, 0.5, -1e-300, 1.5, float("nan"), float("inf"), np.nextafter(1.0, 2.0)]
    assert [int(v[1]) for v in rule([f"P {float(p).hex()}" for p in probs])] == [1, 1, 1, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 2. restatement, record
def test_restatement_against_the_record(golden):
    by, real, redraw, shuffled, expert = R.fixture()
    assert _bits(R.bin_edges(by, R.BINS)).tolist() == _bits(golden["np_edges"]).tolist()
    bins = R.bin_of(golden["np_edges"], by)
    assert bins.tolist() == golden["np_bin"].tolist() == golden["qcut_codes"].tolist()      # pandas' (a, b]
    assert np.bincount(bins, minlength=R.BINS).min() > 0
    perm, offs = R.grouping(R.classes(bins, R.BINS, expert, 3), 3 * R.BINS)
    assert sorted(perm.tolist()) == list(range(R.N)) and offs[-1] == R.N
    assert all(np.all(np.diff(perm[offs[c]:offs[c + 1]]) > 0) for c in range(3 * R.BINS))
    for case, fake, ex, E in (("redraw", redraw, None, 1), ("shuffled", shuffled, None, 1), ("experts", redraw, expert, 3)):
        rec = R.golden_tables(golden, case)
        t = R.profile(real, fake, by, R.BINS, ex, E, names=R.NAMES)
        for k in ("edges", "q_real", "q_gen", "scale"):
            assert np.array_equal(_bits(t[k]), _bits(rec[k])), (case, k)
        assert np.array_equal(t["count"], rec["count"]) and np.array_equal(t["bin"], rec["bin"])
        for k in ("ws", "ks", "mean_real", "std_gen"):
            np.testing.assert_allclose(t[k], rec[k], rtol=1e-13, atol=0, equal_nan=True)
        assert R.check_scalars(t["scalars"], rec, R.NAMES, 3 if ex is not None else 0, case) <= 1.0
    # the property behind the feature, as a condition on the fixture: the shuffled table has the real marginals ...
    for c in range(3):
        assert np.array_equal(np.sort(real[:, c]), np.sort(shuffled[:, c]))
    # ... and a conditional distance of the column that follows the condition at least five times the redraw's
    sh, rd = R.golden_tables(golden, "shuffled")["scalars"], R.golden_tables(golden, "redraw")["scalars"]
    assert sh["cond_ws_lin"] >= 5 * rd["cond_ws_lin"] and 2.0 < sh["cond_ws_lin"] < 3.5 and rd["cond_ws_lin"] < 0.3
    ex = R.golden_tables(golden, "experts")
    assert ex["count"][2].sum() == 0 and np.isnan(ex["scalars"]["cond_ws_1"]) and np.isnan(ex["scalars"]["cond_ws_lin_1"])
    assert np.array_equal(ex["count"][1] + ex["count"][3], ex["count"][0])


def test_summary_from_tables_against_the_record(golden):
    from expertsim.train.conditional import PROBS, scalar_keys, summary_from_tables, weighted_mean
    assert PROBS == R.PROBS
    for case, E in (("redraw", 0), ("shuffled", 0), ("experts", 3)):
        rec = R.golden_tables(golden, case)
        got = summary_from_tables(rec["count"], rec["q_real"], rec["q_gen"], rec["ws"], rec["ks"], rec["scale"],
                                  R.PROBS, R.NAMES, E)
        assert list(got) == scalar_keys(R.NAMES, E) and all(isinstance(v, float) for v in got.values())
        worst = R.check_scalars(got, rec, R.NAMES, E, case)
        print("worst error / bound", worst)
    # empty bins are skipped, a side of no rows gives NaN, the order of the sum is the bins'
    assert weighted_mean([2, 0, 6], [[1.0], [np.nan], [3.0]])[0] == (2.0 * 1.0 + 6.0 * 3.0) / 8
    assert np.isnan(weighted_mean([0, 0], [[1.0], [2.0]])[0])
    with pytest.raises(ValueError, match="0.16"):
        summary_from_tables(rec["count"], rec["q_real"], rec["q_gen"], rec["ws"], rec["ks"], rec["scale"],
                            (0.1, 0.5, 0.84), R.NAMES, 0)
    default = summary_from_tables(rec["count"], rec["q_real"], rec["q_gen"], rec["ws"], rec["ks"], rec["scale"])
    assert "cond_bias_c0" in default and "cond_ws_c2" in default


# ------------------------------------------------------------------------------------------ 3. ABI
def test_header_declares_the_entries():
    q = _prototype("es_segment_quantiles")
    assert q[:14] == _prototype("es_wasserstein_1d")[:14] == _prototype("es_rank_stats")[:14]
    assert q[14:] == ["const double* probs", "int n_q", "double* out", "int32_t* count", "void* work",
                      "size_t work_bytes", "es_stream_t stream"]
    assert _prototype("es_bin_dispatch") == [
        "const void* x", "int x_f64", "int64_t ld", "int rows", "const double* edges", "int n_bins",
        "const int32_t* expert", "int n_experts", "int32_t* bin", "int32_t* perm", "int32_t* offs", "void* work",
        "size_t work_bytes", "es_stream_t stream"]
    assert _prototype("es_segment_quantiles_workspace", "size_t") == _prototype("es_rank_stats_workspace", "size_t")
    assert _prototype("es_bin_dispatch_workspace", "size_t") == ["int rows", "int n_classes"]
    src = open(HEADER).read()
    doc = src[src.index("Conditional fidelity: order statistics per segment"):src.index("int es_bin_dispatch(")]
    for words in ("ONE HOST pointer", "outside [0, 1] or NaN", "numpy's default rule", "no fused multiply-add",
                  "one-sample form", "ONE tagged sort", "exclusive prefix count", "-0.0 and +0.0 are the same value",
                  "strictly below", "(a, b]", "kind=\"stable\"", "there is no atomic", "no host synchronisation",
                  "a rerun is bit-equal"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in ENTRIES.items():
        assert name in hip._SIGS, name
        r, args = hip._SIGS[name]
        proto = _prototype(name, res)
        assert r is (C.c_int if res == "int" else C.c_size_t), name
        assert len(args) == len(proto), name
        assert hasattr(hip.lib(), name)
    src = open(HEADER).read()
    for macro, value in (("ES_QUANTILE_MAX_Q", hip.QUANTILE_MAX_Q), ("ES_BINS_MAX", hip.BINS_MAX)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert (hip.QUANTILE_MAX_Q, hip.BINS_MAX, hip.BINS_MAX_CLASSES, hip.BINS_MAX_ROWS) == (16, 64, 1024, 1 << 20)
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "quantile.hip" in mk and "bins.hip" in mk and "quantile_rule.h" in mk


def test_workspace_limits():
    from expertsim import hip
    qw, bw = hip.segment_quantiles_workspace, hip.bin_dispatch_workspace
    assert qw(3, 2, 4096, 4096) == 0 and qw(3, 2, 4097, 4096) == 3 * 2 * 16384 * 9 == hip.rank_stats_workspace(3, 2, 4097, 4096)
    assert qw(1, 1, 8193, 0) == 16384 * 9                                        # the one-sample form
    for args in ((0, 1, 5000, 5000), (1, 0, 5000, 5000), (1, 1, -1, 9000), (1, 1, 1 << 20, 1)):
        assert qw(*args) == 0, args
    assert bw(1, 1) >= 4 + 4096 and bw(3000, 1024) >= 4 * (3 * 1024 + 3 * 1024)
    assert bw(1 << 20, 1024) >= 4 * (1024 * 1024 + (1 << 20))
    for args in ((0, 4), ((1 << 20) + 1, 4), (16, 0), (16, 1025)):
        assert bw(*args) == 0, args


def test_entries_reject_bad_arguments_before_any_launch():
    from expertsim import hip
    f = C.c_void_p(256)
    big = 1 << 30
    half = (C.c_double * 17)(*([0.5] * 17))

    def quant(u=f, u_ld=2, u_rows=16, u_seg=f, v=f, v_ld=2, v_rows=16, v_seg=f, n_seg=1, ch=2, u_cap=16, v_cap=16,
              probs=half, n_q=3, out=f, count=f, work=f, wb=big):
        probs = C.cast(probs, C.c_void_p) if probs is not None else None
        return hip.call("es_segment_quantiles", u, u_ld, u_rows, None, u_seg, v, v_ld, v_rows, None, v_seg, n_seg, ch,
                        u_cap, v_cap, probs, n_q, out, count, work, wb, None)

    def p(*vals):
        return (C.c_double * len(vals))(*vals)

    def bins(x=f, ld=1, rows=16, edges=f, n_bins=8, expert=None, n_experts=1, bin_=f, perm=f, offs=f, work=f, wb=big):
        return hip.call("es_bin_dispatch", x, 1, ld, rows, edges, n_bins, expert, n_experts, bin_, perm, offs, work,
                        wb, None)

    bad = [lambda: quant(u=None), lambda: quant(u_seg=None), lambda: quant(out=None), lambda: quant(count=None),
           lambda: quant(probs=None), lambda: quant(v_seg=None), lambda: quant(v_rows=0),
           lambda: quant(v=None), lambda: quant(v=None, v_rows=0), lambda: quant(n_seg=0), lambda: quant(ch=0),
           lambda: quant(u_rows=0), lambda: quant(u_ld=1), lambda: quant(v_ld=1), lambda: quant(u_cap=-1),
           lambda: quant(u_cap=1 << 20, v_cap=1), lambda: quant(n_seg=40000), lambda: quant(n_q=0),
           lambda: quant(n_q=17), lambda: quant(probs=p(0.5, 1.5, 0.5)), lambda: quant(probs=p(0.5, 0.5, float("nan"))),
           lambda: quant(probs=p(-0.1, 0.5, 0.5)), lambda: quant(u_cap=8000, v_cap=193, work=None),
           lambda: quant(u_cap=8000, v_cap=193, wb=8),
           lambda: bins(x=None), lambda: bins(perm=None), lambda: bins(offs=None), lambda: bins(edges=None),
           lambda: bins(n_bins=0), lambda: bins(n_bins=65), lambda: bins(n_experts=4), lambda: bins(n_experts=0),
           lambda: bins(expert=f, n_experts=17, n_bins=64), lambda: bins(expert=f, n_experts=129),
           lambda: bins(rows=0), lambda: bins(rows=(1 << 20) + 1), lambda: bins(ld=0), lambda: bins(work=None),
           lambda: bins(wb=8)]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError, match=r"failed \(1\)"):
            fn()
        assert hip.lib().es_last_error(), i


# ------------------------------------------------------------------------------------------ 4. Python surface
def test_wrappers_need_a_device():
    import torch

    from expertsim import hip
    from expertsim.train import conditional as K
    x = np.zeros((8, 3), dtype=np.float64)                        # host data: never copied to a device silently
    t = torch.from_numpy(x)
    for fn in (lambda: K.segment_quantiles(x), lambda: K.segment_quantiles(t, t), lambda: K.bin_edges(t[:, 0], 4),
               lambda: K.bin_dispatch(t[:, 0], None, 1), lambda: K.profile(t, t, t[:, 0], 4)):
        with pytest.raises(hip.HipError):
            fn()
    assert "ALIGNED" in K.profile.__doc__ and "(a, b]" in K.profile.__doc__
    assert K.scalar_keys(("a", "b"), 1) == ["cond_ws", "cond_ws_a", "cond_bias_a", "cond_width_a", "cond_ks_a",
                                            "cond_ws_b", "cond_bias_b", "cond_width_b", "cond_ks_b", "cond_ws_0",
                                            "cond_ws_a_0", "cond_ws_b_0"]


def test_eval_conditional_defaults_off_and_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    assert load_config().train.get("eval_conditional", None) is False
    assert load_config().train.get("eval_conditional_bins", None) == 8
    assert load_config().train.get("eval_conditional_column", None) == 0
    cfg = load_config(overrides=["train.eval_conditional=true"])
    assert cfg.train.eval_conditional is True and not cfg.train.eval_on_device

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_conditional needs train.eval_on_device"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")
    assert "eval_conditional_bins" in evaluate_epoch.__doc__


def test_signature_and_cli_flag_default_off():
    import inspect

    import cli
    from expertsim.models.moe import MoEWrapper
    params = inspect.signature(MoEWrapper.evaluate_device).parameters
    assert params["conditional"].default is False and params["conditional_bins"].default == 8
    assert params["conditional_column"].default == 0
    assert cli.parse_args(["--simulate"]).conditional is False
    args = cli.parse_args(["--simulate", "--real", "r.npy", "--conditional"])
    assert args.conditional is True and args.conditional_bins == 8 and args.conditional_column == 0
    args = cli.parse_args(["--simulate", "--checkpoint", "d", "--out", "o.npz", "--num-samples", "4", "--conditional"])
    with pytest.raises(SystemExit, match="--conditional needs --real"):
        cli.simulate(args)
