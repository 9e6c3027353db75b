"""Host-side checks of the expert diagnostics (no GPU): the C ABI entries and their ctypes bindings, the
argument checks that return before any launch, the workspace sizes, the numpy restatement (tests/diag_refs.py)
against numpy / pandas / scipy, the golden of the KDE tests, and the configuration, model and CLI entry points.

Bounds (tests/diag_refs.py): binning and edges exactly; the golden's density against scipy within
(n + 40 A_j + 9) 2^-53 relative per grid point."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import diag_refs as DR
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
HIST_ARGS = ["const void* x", "int x_f64", "int64_t ld", "int rows", "int cols", "const int32_t* idx",
             "const int32_t* seg", "int n_seg", "int seg_cap", "int bins", "int right", "const double* edges",
             "double* edges_out", "int32_t* counts", "int32_t* outside", "void* work", "size_t work_bytes",
             "es_stream_t stream"]
KDE_ARGS = ["const void* x", "int x_f64", "int64_t ld", "int rows", "int cols", "const int32_t* idx",
            "const int32_t* seg", "int n_seg", "int seg_cap", "int points", "const double* grid", "int min_samples",
            "double std_eps", "double* grid_out", "double* density", "double* bw", "int32_t* valid", "double* sd",
            "void* work", "size_t work_bytes", "es_stream_t stream"]


def _prototype(name, res="int"):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, open(HEADER).read()).group(1))


# ------------------------------------------------------------------------------------------ 1. ABI
def test_header_declares_the_entries():
    assert _prototype("es_segment_histogram") == HIST_ARGS
    assert _prototype("es_segment_kde") == KDE_ARGS
    assert _prototype("es_segment_histogram_workspace", "size_t") == ["int cols", "int bins"]
    assert _prototype("es_segment_kde_workspace", "size_t") == ["int n_seg", "int cols", "int points", "int seg_cap"]
    src = open(HEADER).read()
    doc = src[src.index("Expert diagnostics"):src.index("int es_segment_kde(")]
    for words in ("Values must be finite", "np.histogram", "include_lowest=True", "np.linspace", "outside[s][c]",
                  "ES_DIAG_HIST_MAX_CELLS", "ES_DIAG_KDE_CHUNK", "ES_PREP_SPLIT_MIN", "ES_PREP_CHUNKS",
                  "no float atomics", "ES_ERR_ARG", "NOTHING is written", "bw_method='scott'", "ddof = 1"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in (("es_segment_histogram", "int"), ("es_segment_kde", "int"),
                      ("es_segment_histogram_workspace", "size_t"), ("es_segment_kde_workspace", "size_t")):
        r, args = hip._SIGS[name]
        assert r is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(_prototype(name, res)), name
        assert hasattr(hip.lib(), name)
    assert hip._SIGS["es_segment_kde"][1][KDE_ARGS.index("double std_eps")] is C.c_double
    assert hip._SIGS["es_segment_histogram"][1][HIST_ARGS.index("int64_t ld")] is C.c_int64
    assert _define("ES_DIAG_MAX_COLS") == hip.DIAG_MAX_COLS
    assert _define("ES_DIAG_HIST_MAX_CELLS") == hip.DIAG_HIST_MAX_CELLS
    assert _define("ES_DIAG_KDE_CHUNK") == hip.DIAG_KDE_CHUNK == DR.KDE_CHUNK
    assert _define("ES_DIAG_KDE_MAX_POINTS") == hip.DIAG_KDE_MAX_POINTS
    assert _define("ES_DIAG_RANGE_BYTES") == hip.DIAG_RANGE_BYTES == 2 * 8 * hip.DIAG_MAX_COLS


def test_workspace_sizes():
    from expertsim import hip
    hw, kw = hip.segment_histogram_workspace, hip.segment_kde_workspace
    # the histogram: the range keys [2][ES_DIAG_MAX_COLS] uint64; 0 outside the limits
    assert hw(9, 50) == hw(1, 1) == hw(9, 257) == 1024
    assert hw(0, 50) == hw(65, 1) == hw(9, 0) == 0
    assert hw(1, 2559) == 1024 and hw(1, 2560) == 0          # cols * (2 bins + 1) <= 5120
    assert hw(64, 39) == 1024 and hw(64, 40) == 0
    # the KDE: the range + chunk sums [n_seg][cols][ceil(seg_cap / 256)][points] fp64
    assert kw(4, 8, 100, 16384) == 1024 + 4 * 8 * 64 * 100 * 8
    assert kw(1, 1, 1, 1) == 1024 + 8 and kw(2, 3, 7, 256) == 1024 + 2 * 3 * 7 * 8
    assert kw(2, 3, 7, 257) == 1024 + 2 * 3 * 2 * 7 * 8
    assert kw(0, 8, 100, 5) == kw(1, 0, 100, 5) == kw(1, 65, 100, 5) == kw(1, 8, 0, 5) == kw(1, 8, 1025, 5) == 0
    assert kw(1, 8, 100, 0) == 0


# ------------------------------------------------------------------- 2. argument errors, no device
def test_segment_histogram_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)

    def call(x=fake, f64=1, ld=9, rows=100, cols=9, idx=None, seg=fake, n_seg=2, cap=100, bins=50, right=0, edges=None,
             eo=fake, counts=fake, outside=fake, work=fake, wb=1024):
        return hip.call("es_segment_histogram", x, f64, ld, rows, cols, idx, seg, n_seg, cap, bins, right, edges, eo,
                        counts, outside, work, wb, None)

    for kw in (dict(x=None), dict(seg=None), dict(eo=None), dict(counts=None), dict(outside=None), dict(f64=2),
               dict(f64=-1), dict(right=2), dict(right=-1), dict(cols=0), dict(cols=65, ld=65), dict(ld=8), dict(rows=-1),
               dict(rows=(1 << 20) + 1), dict(n_seg=-1), dict(n_seg=65536), dict(cap=0), dict(bins=0), dict(bins=-3),
               dict(bins=284), dict(cols=64, ld=64, bins=40), dict(work=None), dict(wb=1023), dict(wb=0)):
        with pytest.raises(hip.HipError):
            call(**kw)
    with pytest.raises(hip.HipError, match="workspace"):
        call(wb=8)
    # nothing to do: ES_OK without a launch (and without a workspace)
    assert call(rows=0, work=None, wb=0) == 0
    assert call(n_seg=0, work=None, wb=0) == 0


def test_segment_kde_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)
    need = hip.segment_kde_workspace(2, 8, 100, 100)

    def call(x=fake, f64=1, ld=9, rows=100, cols=8, idx=None, seg=fake, n_seg=2, cap=100, points=100, grid=None,
             ms=5, eps=1e-12, go=fake, dens=fake, bw=fake, valid=fake, sd=None, work=fake, wb=need):
        return hip.call("es_segment_kde", x, f64, ld, rows, cols, idx, seg, n_seg, cap, points, grid, ms, eps, go, dens,
                        bw, valid, sd, work, wb, None)

    for kw in (dict(x=None), dict(seg=None), dict(go=None), dict(dens=None), dict(bw=None), dict(valid=None),
               dict(f64=2), dict(cols=0), dict(cols=65, ld=65), dict(ld=7), dict(rows=-1), dict(rows=(1 << 20) + 1),
               dict(n_seg=-1), dict(n_seg=65536), dict(cap=0), dict(points=0), dict(points=1025), dict(ms=-1),
               dict(eps=float("nan")), dict(work=None), dict(wb=need - 1), dict(wb=0)):
        with pytest.raises(hip.HipError):
            call(**kw)
    with pytest.raises(hip.HipError, match="workspace"):
        call(wb=8)
    # a caller-given grid does not spare the workspace: the chunk sums live there
    with pytest.raises(hip.HipError, match="workspace"):
        call(grid=fake, wb=1024)
    assert call(rows=0, work=None, wb=0) == 0
    assert call(n_seg=0, work=None, wb=0) == 0


def test_device_functions_raise_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from expertsim import hip
    from expertsim.train import diagnostics as D
    x = np.zeros((8, 3))
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        D.segment_histogram(x)
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        D.segment_kde(x)
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        D.expert_diagnostics(x, None, 1, np.zeros(8))


# --------------------------------------------------------------------- 3. restatement = the libraries
def _tie_values(rng, e, n):
    """n values inside [e[0], e[-1]], a third of them exactly on edges (both ends included)."""
    x = rng.uniform(e[0], e[-1], n)
    on = rng.choice(n, n // 3, replace=False)
    x[on] = e[rng.integers(0, len(e), len(on))]
    x[:2] = e[0], e[-1]
    return x


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_binning_matches_numpy_and_pandas(dtype):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(12)
    for bins, lo, hi in ((1, -1.0, 2.0), (50, 0.1, 7.3), (257, -1e3, 1e-2), (7, 3.0, 3.0 + 1e-9)):
        e = np.linspace(lo, hi, bins + 1)
        x = _tie_values(rng, e, 5000).astype(dtype)          # float32: rounding may leave [e[0], e[-1]]
        wide = x.astype(np.float64)
        inside = (wide >= e[0]) & (wide <= e[-1])
        got0, out0 = DR.histogram_ref(x, e, right=False)
        assert np.array_equal(got0, np.histogram(wide, bins=e)[0]) and out0 == int((~inside).sum())
        got1, out1 = DR.histogram_ref(x, e, right=True)
        codes = pd.cut(wide, bins=e, include_lowest=True, labels=False)
        want1 = np.bincount(codes[~np.isnan(codes)].astype(np.int64), minlength=bins)
        assert np.array_equal(got1, want1) and out1 == int(np.isnan(codes).sum()) == int((~inside).sum())
        assert got0.sum() + out0 == got1.sum() + out1 == 5000
        if dtype == "float64":
            assert out0 == 0 and (bins == 1 or not np.array_equal(got0, got1))   # ties tell the modes apart
    # values outside caller-given edges are in no bin
    e = np.array([0.0, 1.0, 2.5, 2.5, 4.0])
    x = np.array([-0.5, 0.0, 1.0, 2.5, 4.0, 4.5, 3.0])
    assert DR.bin_index(x, e, False).tolist() == [-1, 0, 1, 3, 3, -1, 3]
    assert DR.bin_index(x, e, True).tolist() == [-1, 0, 0, 1, 3, -1, 3]
    assert np.array_equal(DR.histogram_ref(x[1:5], e, False)[0], np.histogram(x[1:5], bins=e)[0])


def test_all_equal_edges():
    # a constant column: lo == hi, every edge equal; numpy puts every value into the last bin, the right = 1
    # definition into bin 0
    x = np.full(17, 2.75)
    e = DR.linspace_ref(x.min(), x.max(), 6)
    assert (e == 2.75).all() and np.array_equal(e, np.linspace(2.75, 2.75, 6))
    assert DR.histogram_ref(x, e, False)[0].tolist() == [0, 0, 0, 0, 17] == np.histogram(x, bins=e)[0].tolist()
    assert DR.histogram_ref(x, e, True)[0].tolist() == [17, 0, 0, 0, 0]
    counts, edges, outside = DR.segment_histogram_ref(x[:, None], [np.arange(17), np.arange(3)], 5, False)
    assert counts[:, 0, 4].tolist() == [17, 3] and not outside.any() and np.array_equal(edges[0], e)


def test_linspace_restatement_is_numpy_bit_for_bit():
    rng = np.random.default_rng(3)
    for _ in range(2000):
        lo = rng.normal() * 10.0 ** rng.integers(-8, 9)
        hi = lo + abs(rng.normal()) * 10.0 ** rng.integers(-8, 9)
        num = int(rng.integers(2, 300))
        assert np.array_equal(DR.linspace_ref(lo, hi, num).view(np.int64), np.linspace(lo, hi, num).view(np.int64))
    for lo, hi, num in ((1.5, 1.5, 51), (0.0, 0.0, 2), (-3.0, 4.0, 1), (5e-324, 1e-323, 51), (-1.0, 1.0, 101)):
        assert np.array_equal(DR.linspace_ref(lo, hi, num).view(np.int64), np.linspace(lo, hi, num).view(np.int64))
    g = DR.kde_grid_ref(2.0, 2.0, 100)                       # the reference widens a constant column
    assert np.array_equal(g, np.linspace(2.0 - 1e-6, 2.0 + 1e-6, 100))


def test_moments_restatement_order():
    # one chain up to SPLIT_MIN members; above, CHUNKS chunks of ceil(n / CHUNKS), chunk sums in chunk order
    import prepare_refs as PR
    rng = np.random.default_rng(5)
    for n in (5, PR.SPLIT_MIN, PR.SPLIT_MIN + 1, 1000):
        d = rng.gamma(2.0, 1.5, n)
        L = n if n <= PR.SPLIT_MIN else -(-n // PR.CHUNKS)

        def ordered(term):
            total = 0.0
            for first in range(0, n, L):
                part = 0.0
                for v in d[first:first + L]:
                    part += term(v)
                total += part
            return total

        S = ordered(lambda v: v)
        m = S / n
        Q = ordered(lambda v: (v - m) * (v - m))
        assert DR.moments_ref(d) == (S, m, Q)
        assert abs(np.sqrt(Q / (n - 1)) - np.std(d, ddof=1)) <= 4 * n * DR.U * np.std(d, ddof=1)


# ------------------------------------------------------------------------------------ 4. the golden
def test_golden_holds_the_required_cases():
    g = DR.golden()
    assert sorted(len(c["d"]) for c in g.values()) == [5, 64, 65, 1000, 4097]
    assert sorted(len(c["grid"]) for c in g.values()) == [37, 100, 100, 100, 100]
    assert sum(a.size for c in g.values() for a in c.values()) < 20000
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "diag_kde.npz")) < 256 * 1024
    for name, c in g.items():
        n = len(c["d"])
        assert c["density"].shape == c["A"].shape == c["grid"].shape and (c["A"] >= 0).all()
        _, _, Q = DR.moments_ref(c["d"])
        assert c["sd"] == np.sqrt(Q / (n - 1.0)) and c["h"] == c["sd"] * np.float64(n) ** -0.2
    far = g["n1000_clusters"]
    d = np.sort(far["d"])
    assert np.diff(d).max() > 0.5 * (d[-1] - d[0])                           # two far-apart clusters
    assert (far["density"] < 2.0 ** -1000).sum() >= 2 and (far["density"] > 2.0 ** -1000).sum() >= 20


def test_golden_density_matches_scipy_and_the_restatement():
    stats = pytest.importorskip("scipy.stats")
    for name, c in DR.golden().items():
        n = len(c["d"])
        kde = stats.gaussian_kde(c["d"], bw_method="scott")
        h = float(np.sqrt(kde.covariance[0, 0]))
        assert abs(h - c["h"]) <= 4 * n * DR.U * c["h"], name                # scipy's own moments: np.cov
        ratio = DR.check_density(kde(c["grid"]), c)
        own = DR.kde_ref(c["d"], c["grid"])
        assert own["valid"] == 1 and own["sd"] == c["sd"] and own["bw"] == c["h"]
        print(f"{name}: scipy error / bound {ratio:.3f}, restatement {DR.check_density(own['density'], c):.3f}")
    # the skip rules of the reference
    grid = np.linspace(0.0, 1.0, 7)
    assert DR.kde_ref(np.arange(4.0), grid)["valid"] == 0 and DR.kde_ref(np.arange(5.0), grid)["valid"] == 1
    flat = DR.kde_ref(np.full(9, 0.3), grid)
    assert flat["valid"] == 0 and flat["bw"] == 0.0 and np.isnan(flat["density"]).all()


# ------------------------------------------------------------------------- 5. configuration, model, CLI
def test_eval_diagnostics_defaults_off_and_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    assert load_config().train.get("eval_diagnostics", None) is False
    cfg = load_config(overrides=["train.eval_diagnostics=true"])
    assert cfg.train.eval_diagnostics is True and not cfg.train.eval_on_device

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_on_device"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")


def test_diagnose_raises_off_the_hip_device():
    from expertsim import hip
    from expertsim.config import inject_shared, load_config
    from expertsim.models import build_model
    from expertsim.models.moe import MoEWrapper
    cfg = inject_shared(load_config(overrides=["model.architecture=neutron", "model.n_experts=1"]))
    torch.manual_seed(0)
    parts = [build_model(f"neutron.{k}", getattr(cfg.model, k), "cpu") for k in ("generator", "discriminator", "aux_reg")]
    router = build_model("router_v1", cfg.model.router, "cpu")
    moe = MoEWrapper(*parts, router, 1, cfg, image_shape=(44, 44))
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        moe.diagnose(torch.zeros(4, 9))


def test_cli_knows_diagnose():
    import cli
    assert cli.parse_args([]).diagnose is False and cli.parse_args(["--simulate"]).diagnose is False
    a = cli.parse_args(["--diagnose", "--checkpoint", "d", "--conditions", "c.npy", "--out", "o.npz"])
    assert a.diagnose and not a.simulate and not a.prepare
    assert (a.checkpoint, a.conditions, a.out) == ("d", "c.npy", "o.npz")
    with pytest.raises(SystemExit):
        cli.diagnose(cli.parse_args(["--diagnose", "--conditions", "c.npy"]))


def test_save_diagnostics_round_trip(tmp_path):
    from expertsim.train.diagnostics import DIAGNOSTIC_KEYS, save_diagnostics
    diag = {k: np.arange(6.0).reshape(2, 3) + i for i, k in enumerate(DIAGNOSTIC_KEYS)}
    path = save_diagnostics(tmp_path / "diag", diag)
    assert path.endswith("diag.npz")
    z = np.load(path)
    assert set(z.files) == set(DIAGNOSTIC_KEYS) and all(np.array_equal(z[k], diag[k]) for k in diag)
