"""Host-side checks of the conditioning embeddings (no GPU): the C ABI entries and their ctypes bindings, the
argument checks that return before any launch, the workspace sizes, the numpy restatement (tests/embed_refs.py)
against scikit-learn, the golden of the end-to-end test, and the configuration, model and CLI entry points."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import embed_refs as ER
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
PCA_ARGS = ["const void* x", "int x_f64", "int64_t ld", "int rows", "int cols", "int k", "double* scores",
            "double* components", "double* explained_variance", "double* explained_variance_ratio", "double* mean",
            "void* work", "size_t work_bytes", "es_stream_t stream"]
AFF_ARGS = ["const float* x", "int64_t ld", "int rows", "int cols", "double perplexity", "double* beta",
            "double* log_s", "float* dmin", "int32_t* steps", "es_stream_t stream"]
GRAD_ARGS = ["const float* x", "int64_t ld", "int rows", "int cols", "const double* beta", "const double* log_s",
             "const float* dmin", "const float* y", "double exaggeration", "double* g", "double* z_kl", "void* work",
             "size_t work_bytes", "es_stream_t stream"]
RUN_ARGS = ["const float* x", "int64_t ld", "int rows", "int cols", "const double* beta", "const double* log_s",
            "const float* dmin", "float* y", "double* upd", "double* gains", "int n_iter", "int iter0",
            "double exaggeration", "int exaggeration_iters", "double momentum0", "double momentum1",
            "double learning_rate", "double min_gain", "int check_every", "double* log", "int log_rows", "void* work",
            "size_t work_bytes", "es_stream_t stream"]
ENTRIES = {"es_pca_project": PCA_ARGS, "es_tsne_affinities": AFF_ARGS, "es_tsne_gradient": GRAD_ARGS,
           "es_tsne_run": RUN_ARGS}


def _prototype(name, res="int"):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _define(name):
    return int(re.search(r"#define %s (\d+)" % name, open(HEADER).read()).group(1))


# ------------------------------------------------------------------------------------------ 1. ABI
def test_header_declares_the_entries():
    for name, args in ENTRIES.items():
        assert _prototype(name) == args, name
    assert _prototype("es_pca_project_workspace", "size_t") == ["int cols"]
    assert _prototype("es_tsne_workspace", "size_t") == ["int rows"]
    src = open(HEADER).read()
    doc = src[src.index("Conditioning embeddings"):src.index("int es_tsne_run(")]
    for words in ("Values must be finite", "NOTHING is written", "ES_ERR_ARG", "no float atomics", "ddof = 1",
                  "svd_flip", "ES_PREP_SPLIT_MIN", "ES_PREP_CHUNKS", "d_ij == d_ji bitwise", "dmin_i", "at most 100",
                  "1e-5", "steps = 100", "DBL_EPSILON", "ES_TSNE_TILE", "ES_TSNE_MAX_SPLITS", "split order",
                  "early-stop rules", "999 of 1000", "min_gain", "iter0", "check_every"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, args in ENTRIES.items():
        r, sig = hip._SIGS[name]
        assert r is C.c_int and len(sig) == len(args), name
        for a, t in zip(args, sig):
            want = (C.c_double if a.startswith("double ") else C.c_int64 if a.startswith("int64_t ") else
                    C.c_size_t if a.startswith("size_t ") else C.c_int if a.startswith("int ") else C.c_void_p)
            assert t is want, (name, a)
        assert hasattr(hip.lib(), name)
    for name in ("es_pca_project_workspace", "es_tsne_workspace"):
        assert hip._SIGS[name] == (C.c_size_t, [C.c_int]) and hasattr(hip.lib(), name)
    assert _define("ES_TSNE_TILE") == hip.TSNE_TILE == ER.TILE
    assert _define("ES_TSNE_MAX_SPLITS") == hip.TSNE_MAX_SPLITS == ER.MAX_SPLITS
    assert (ER.SPLIT_MIN, ER.CHUNKS) == (hip.PREP_SPLIT_MIN, hip.PREP_CHUNKS)


def test_workspace_sizes():
    from expertsim import hip
    pw, tw = hip.pca_project_workspace, hip.tsne_workspace
    assert pw(9) == 2 * 81 * 8 and pw(1) == 16 and pw(64) == 2 * 4096 * 8
    assert pw(0) == pw(65) == pw(-1) == 0

    def want(rows):
        r256 = lambda v: (v + 255) // 256 * 256
        ns = min(max(-(-rows // 256), 1), hip.TSNE_MAX_SPLITS)
        return r256(ns * rows * 8 * 8) + r256(rows * 16) + 256 + 2 * r256(rows * 4)

    for rows in (2, 255, 256, 257, 300, 4097, 16384, 1 << 17):
        assert tw(rows) == want(rows), rows
    assert tw(1) == tw(0) == tw((1 << 17) + 1) == tw(-5) == 0


# ------------------------------------------------------------------- 2. argument errors, no device
def test_pca_project_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)
    need = hip.pca_project_workspace(9)

    def call(x=fake, f64=0, ld=9, rows=100, cols=9, k=2, sc=fake, co=fake, ev=fake, evr=fake, mean=fake, work=fake,
             wb=need):
        return hip.call("es_pca_project", x, f64, ld, rows, cols, k, sc, co, ev, evr, mean, work, wb, None)

    for kw in (dict(x=None), dict(sc=None), dict(co=None), dict(ev=None), dict(evr=None), dict(mean=None), dict(f64=2),
               dict(f64=-1), dict(rows=1), dict(rows=0), dict(rows=-3), dict(rows=(1 << 20) + 1), dict(cols=0),
               dict(cols=65, ld=65, wb=1 << 20), dict(ld=8), dict(k=0), dict(k=10), dict(k=-1), dict(work=None),
               dict(wb=need - 1), dict(wb=0)):
        with pytest.raises(hip.HipError):
            call(**kw)
    with pytest.raises(hip.HipError, match="workspace"):
        call(wb=8)


def test_tsne_affinities_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)

    def call(x=fake, ld=9, rows=100, cols=9, perp=30.0, beta=fake, ls=fake, dmin=fake, steps=fake):
        return hip.call("es_tsne_affinities", x, ld, rows, cols, perp, beta, ls, dmin, steps, None)

    for kw in (dict(x=None), dict(beta=None), dict(ls=None), dict(dmin=None), dict(steps=None), dict(rows=1),
               dict(rows=0), dict(rows=(1 << 17) + 1), dict(cols=0), dict(cols=65, ld=65), dict(ld=8),
               dict(perp=100.0), dict(perp=150.0), dict(rows=30), dict(perp=0.0), dict(perp=-1.0),
               dict(perp=float("nan"))):
        with pytest.raises(hip.HipError):
            call(**kw)
    with pytest.raises(hip.HipError, match="perplexity"):
        call(rows=30, perp=30.0)


def test_tsne_gradient_and_run_reject_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)
    need = hip.tsne_workspace(100)

    def grad(x=fake, ld=9, rows=100, cols=9, beta=fake, ls=fake, dmin=fake, y=fake, a=12.0, g=fake, zkl=fake,
             work=fake, wb=need):
        return hip.call("es_tsne_gradient", x, ld, rows, cols, beta, ls, dmin, y, a, g, zkl, work, wb, None)

    def run(x=fake, ld=9, rows=100, cols=9, beta=fake, ls=fake, dmin=fake, y=fake, upd=fake, gains=fake, n=10, i0=0,
            a=12.0, ai=250, m0=0.5, m1=0.8, lr=50.0, mg=0.01, ce=50, log=fake, lrows=1, work=fake, wb=need):
        return hip.call("es_tsne_run", x, ld, rows, cols, beta, ls, dmin, y, upd, gains, n, i0, a, ai, m0, m1, lr, mg,
                        ce, log, lrows, work, wb, None)

    common = (dict(x=None), dict(beta=None), dict(ls=None), dict(dmin=None), dict(y=None), dict(rows=1), dict(rows=0),
              dict(rows=(1 << 17) + 1, wb=1 << 40), dict(cols=0), dict(cols=65, ld=65), dict(ld=8), dict(a=0.0),
              dict(a=float("nan")), dict(work=None), dict(wb=need - 1), dict(wb=0))
    for kw in common + (dict(g=None), dict(zkl=None)):
        with pytest.raises(hip.HipError):
            grad(**kw)
    for kw in common + (dict(upd=None), dict(gains=None), dict(log=None), dict(n=-1), dict(i0=-1), dict(ce=0),
                        dict(lr=0.0), dict(mg=-1.0), dict(ai=-1), dict(n=51), dict(n=10, i0=45), dict(lrows=0)):
        with pytest.raises(hip.HipError):
            run(**kw)
    with pytest.raises(hip.HipError, match="workspace"):
        grad(wb=8)
    with pytest.raises(hip.HipError, match="workspace"):
        run(wb=8)
    with pytest.raises(hip.HipError, match="log"):
        run(n=100, lrows=1)
    assert run(n=0, work=None, wb=0) == 0                       # nothing to do: ES_OK without a launch


def test_device_functions_raise_without_a_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from expertsim import hip
    from expertsim.train import embedding as E
    x = np.zeros((64, 3), dtype=np.float32)
    for fn in (lambda: E.pca_project(x), lambda: E.tsne_embed(x), lambda: E.tsne_affinities(x),
               lambda: E.cond_embedding(x, None, 1)):
        with pytest.raises(hip.HipError, match="no CPU fallback"):
            fn()


# --------------------------------------------------------------------- 3. restatement = scikit-learn
def _clusters(n, cols, seed, dup=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (3, cols))
    x = (centres[rng.integers(0, 3, n)] + rng.normal(0.0, 1.0, (n, cols))).astype(np.float32)
    if dup is not None:
        x[dup[0]:dup[1]] = x[dup[0]]
    return x


def test_gradient_and_kl_match_sklearn():
    """embed_refs.gradient_ref against sklearn.manifold._t_sne._kl_divergence (exact method) on 300 points, at y of
    scale 1e-4 and of scale 5: both agreed to 1.5e-15 of the largest entry when written; asserted at 1e-12."""
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    x = _clusters(300, 9, 1)
    aff = ER.affinities_ref(x, 30.0)
    P = ER.joint_P(aff["beta"], aff["log_s"], aff["dmin"], aff["d"])
    assert abs(P.sum() - 1.0) < 1e-12 and np.array_equal(P, P.T)
    rng = np.random.default_rng(2)
    for scale in (1e-4, 5.0):
        y = (rng.normal(0.0, scale, (300, 2))).astype(np.float32)
        g, Z, KL = ER.gradient_ref(P, y, 1.0)
        kl_sk, g_sk = _t_sne._kl_divergence(y.astype(np.float64).ravel(), squareform(P), 1.0, 300, 2)
        assert abs(KL - kl_sk) <= 1e-12 * max(abs(kl_sk), 1.0), scale
        assert np.abs(g.ravel() - g_sk).max() <= 1e-12 * np.abs(g_sk).max(), scale
        print(f"scale {scale}: KL {KL:.6f}, gradient error {np.abs(g.ravel() - g_sk).max() / np.abs(g_sk).max():.2e}")


def test_pca_restatement_matches_sklearn():
    """embed_refs.pca_ref (the header's moments, eigh, the sign rule) against PCA(svd_solver='full'): components
    agreed to 1.3e-15 when written; asserted at 1e-12."""
    from sklearn.decomposition import PCA
    g = ER.golden()
    for x, k in ((g["X"], 2), (_clusters(257, 9, 3).astype(np.float64), 3)):
        mine = ER.pca_ref(x, k)
        sk = PCA(n_components=k, svd_solver="full").fit(x.astype(np.float64))
        assert np.abs(mine["components"] - sk.components_).max() <= 1e-12
        assert np.abs(mine["explained_variance"] - sk.explained_variance_).max() <= 1e-12 * sk.explained_variance_[0]
        assert np.abs(mine["explained_variance_ratio"] - sk.explained_variance_ratio_).max() <= 1e-12
        assert np.abs(mine["mean"] - sk.mean_).max() <= 1e-12
        assert np.abs(mine["scores"] - sk.transform(x.astype(np.float64))).max() <= 1e-11
    # the sign rule: the first index wins a tie
    assert np.array_equal(ER.sign_rule([[-0.5, 0.5, 0.1], [0.2, -0.7, 0.7]]), [[0.5, -0.5, -0.1], [-0.2, 0.7, -0.7]])
    # the chunked order of the moments, and a constant column
    x = np.random.default_rng(4).normal(0, 1, (1000, 4))
    x[:, 2] = 0.75
    mean, cov = ER.moments_ref(x)
    assert mean[2] == 0.75 and not cov[2].any() and not cov[:, 2].any()
    assert np.abs(cov - np.cov(x.T)).max() <= 1000 * ER.U * np.abs(cov).max() * 4


def test_joint_probabilities_match_sklearn():
    """The restatement's P on a duplicate-free set against sklearn's _joint_probabilities, which searches in
    float32 on float32 distances with its unshifted sums.  Worst |P - P_sklearn| / max P measured when written:
    MEASURED below; asserted at four times that."""
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    MEASURED = 2.8e-13
    x = _clusters(300, 9, 5)
    aff = ER.affinities_ref(x, 30.0)
    assert aff["converged"].all() and (aff["dmin"] > 0).all()
    P = ER.joint_P(aff["beta"], aff["log_s"], aff["dmin"], aff["d"])
    D = aff["d"].astype(np.float32)
    P_sk = squareform(_t_sne._joint_probabilities(D, 30.0, 0))
    worst = np.abs(P - P_sk).max() / P_sk.max()
    print(f"worst |P - P_sklearn| / max P = {worst:.3e}")
    assert worst <= 4 * MEASURED
    # the search itself: H within 1e-5 of log(perplexity) at the returned beta
    for i in (0, 17, 299):
        dd = np.delete(aff["d"][i].astype(np.float64) - np.float64(aff["dmin"][i]), i)
        assert abs(ER.entropy(aff["beta"][i], dd)[0] - np.log(30.0)) <= 1e-5


def test_unreachable_rows_of_the_restatement():
    x = _clusters(300, 9, 6, dup=(10, 50))
    aff = ER.affinities_ref(x, 30.0)
    assert not aff["converged"][10:50].any() and (aff["steps"][10:50] == 100).all()
    assert (aff["beta"][10:50] == 2.0 ** 99).all() and (aff["dmin"][10:50] == 0).all()
    assert aff["converged"].sum() >= 200
    C_ = ER.conditional_P(aff["beta"], aff["log_s"], aff["dmin"], aff["d"])
    assert np.abs(C_[10, 11:50] - 1.0 / 39).max() <= 1e-12 and abs(C_[10].sum() - 1.0) <= 1e-12
    d = aff["d"]
    assert np.array_equal(d, d.T) and not d[10:50, 10:50].any()


def test_run_restatement_schedule():
    x = _clusters(64, 5, 7)
    aff = ER.affinities_ref(x, 10.0)
    P = ER.joint_P(aff["beta"], aff["log_s"], aff["dmin"], aff["d"])
    y0 = np.random.default_rng(8).normal(0, 1e-4, (64, 2)).astype(np.float32)
    kw = dict(exaggeration_iters=4, check_every=5)
    y, upd, gains, log = ER.run_ref(P, y0, 10, **kw)
    assert sorted(log) == [0, 1] and y.dtype == np.float32
    y5, u5, g5, log5 = ER.run_ref(P, y0, 5, **kw)
    y10, u10, g10, log10 = ER.run_ref(P, y5, 5, iter0=5, upd=u5, gains=g5, **kw)
    assert np.array_equal(y10, y) and np.array_equal(u10, upd) and np.array_equal(g10, gains)
    assert log5[0] == log[0] and log10[1] == log[1]
    assert ER.auto_learning_rate(16384) == 16384 / 48 and ER.auto_learning_rate(300) == 50.0


# ------------------------------------------------------------------------------------ 4. the golden
def test_golden_keys_and_shapes():
    g = ER.golden()
    shapes = {"X": (1024, 9), "labels": (1024,), "y_pca": (1024, 2), "kl_pca": (), "n_iter_pca": (),
              "y_random": (5, 1024, 2), "kl_random": (5,), "purity_pca": (), "purity_random": (5,),
              "sklearn_version": ()}
    assert {k: g[k].shape for k in shapes} == shapes and set(g.files) == set(shapes)
    assert g["X"].dtype == np.float32 and np.array_equal(np.bincount(g["labels"]), [256] * 4)
    assert os.path.getsize(os.path.join(REPO, "tests", "golden", "tsne_sklearn.npz")) < 256 * 1024
    kls = np.concatenate([[g["kl_pca"]], g["kl_random"]])
    assert (kls > 0.5).all() and (kls.max() - kls.min()) / kls.min() < 0.1
    assert abs(ER.knn_purity(g["y_pca"], g["labels"]) - g["purity_pca"]) < 1e-12
    lam = ER.pca_ref(g["X"], 2)["eigenvalues"]
    assert lam[0] - lam[1] > 0.2 * lam[0] and lam[1] - lam[2] > 0.2 * lam[0]      # well-separated leading eigenvalues


# ------------------------------------------------------------------------- 5. configuration, model, CLI
def test_eval_embedding_defaults_off_and_needs_eval_diagnostics():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    cfg = load_config()
    assert cfg.train.get("eval_embedding", None) is False
    assert cfg.train.eval_embedding_max == 16384 and cfg.train.eval_embedding_iters == 1000
    cfg = load_config(overrides=["train.eval_embedding=true", "train.eval_on_device=true"])

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_diagnostics"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")


def test_diagnose_signature_and_cli_flags():
    from expertsim.models.moe import MoEWrapper
    from expertsim.train import embedding as E
    p = inspect.signature(MoEWrapper.diagnose).parameters
    assert (p["embedding"].default, p["embedding_iters"].default, p["embedding_max"].default) == (False, 1000, 16384)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("embedding", "embedding_iters", "embedding_max"))
    p = inspect.signature(E.tsne_embed).parameters
    assert [(k, v.default) for k, v in p.items()][1:] == [
        ("perplexity", 30.0), ("n_iter", 1000), ("init", "pca"), ("exaggeration", 12.0), ("exaggeration_iters", 250),
        ("learning_rate", "auto"), ("y0", None)]
    p = inspect.signature(E.cond_embedding).parameters
    assert (p["max_rows"].default, p["n_iter"].default) == (16384, 1000)
    assert E.EMBEDDING_KEYS == ("embed_rows", "embed_expert", "pca", "pca_components", "pca_explained_variance",
                                "pca_explained_variance_ratio", "tsne", "tsne_kl")
    import cli
    a = cli.parse_args(["--diagnose"])
    assert a.embedding is False and a.embedding_iters == 1000
    a = cli.parse_args(["--diagnose", "--embedding", "--embedding-iters", "60"])
    assert a.diagnose and a.embedding is True and a.embedding_iters == 60


def test_embedding_rows_stride():
    from expertsim.train.embedding import embedding_rows
    assert np.array_equal(embedding_rows(600, 16384), np.arange(600))
    assert np.array_equal(embedding_rows(16384, 16384), np.arange(16384))
    assert np.array_equal(embedding_rows(2 * 300 + 1, 300), np.arange(0, 601, 3))       # ceil(601 / 300) = 3
    assert np.array_equal(embedding_rows(16385, 16384), np.arange(0, 16385, 2))
    with pytest.raises(ValueError):
        embedding_rows(10, 1)
