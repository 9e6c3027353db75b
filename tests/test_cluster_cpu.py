"""Host-side checks of the clustering feature (no GPU): the numpy restatement (tests/cluster_refs.py) against
scikit-learn's record (tests/golden/kmeans_sklearn.npz), the agreement numbers against sklearn.metrics, the
renumbering rule, prepare_dataset's argument errors, the new CLI flags, the C ABI entries and the argument
checks that return before any launch.

Bounds against the record: labels and n_iter equal (the tool asserted a nearest / second-nearest gap of at
least 1e-7 and a shift / threshold margin of at least 1e-6 in every iteration); a centre is the mean of at most
n_max rows of equal labels, so it holds n_max 2^-52 max|x| whatever the summation order; the inertia sums
N cols non-negative terms: N cols 2^-52 relative."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cluster_refs as R
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
ENTRIES = {"es_kmeans_assign": "int", "es_kmeans_update": "int", "es_kmeans_plusplus": "int",
           "es_confusion_matrix": "int", "es_kmeans_workspace": "size_t", "es_kmeans_plusplus_workspace": "size_t",
           "es_kmeans_trials": "int"}
EPS = 2.0 ** -52


def _prototype(name, res="int"):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


# ------------------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("case", R.CASES)
def test_restatement_reproduces_sklearn(golden, case):
    images = golden["neutron_images" if case == "neutron" else "proton_images"]
    X = images.reshape(len(images), -1).astype(np.float64)
    trace = {}
    labels, centres, inertia, n_iter = R.lloyd(X, golden[f"{case}_init"], trace=trace)
    assert np.array_equal(labels, golden[f"{case}_labels"])
    assert n_iter == int(golden[f"{case}_n_iter"])
    n_max = np.bincount(labels).max()
    assert np.abs(centres - golden[f"{case}_centres"]).max() <= n_max * EPS * np.abs(X).max()
    assert abs(inertia - float(golden[f"{case}_inertia"])) <= X.size * EPS * float(golden[f"{case}_inertia"])
    assert sum(trace["relocated"]) == (1 if case == "proton_empty" else 0)
    assert min(trace["gap"]) >= 1e-7 and min(trace["margin"]) >= 1e-6


def test_restatement_without_centring_gives_the_same_clustering(golden):
    X = golden["proton_images"].reshape(768, -1).astype(np.float64)
    labels, _, _, n_iter = R.lloyd(X, golden["proton_init"], centre=False)
    assert np.array_equal(labels, golden["proton_labels"]) and n_iter == int(golden["proton_n_iter"])


def test_plusplus_restatement_reproduces_the_record(golden):
    X = golden["proton_images"].reshape(768, -1).astype(np.float64)
    u = golden["pp_draws"]
    assert u.shape == (8, R.trials(8)) and R.trials(1) == 2 and R.trials(8) == 4 and R.trials(64) == 6
    trace = {}
    index, centres = R.plusplus(X, 8, u, trace=trace)
    assert np.array_equal(index, golden["pp_index"])
    assert np.array_equal(centres, X[index])
    assert trace["search_gap"] >= 1e-9 and trace["pot_gap"] >= 1e-9


def test_prefix_sums_are_monotone_and_close_to_cumsum():
    rs = np.random.RandomState(3)
    for rows in (1, 5, 1024, 1025, 5000):
        v = rs.rand(rows) ** 4
        cum = R.prefix_sums(v)
        assert (np.diff(cum) >= 0).all()
        np.testing.assert_allclose(cum, np.cumsum(v), rtol=rows * 2.0 ** -52)


# ------------------------------------------------------------------------------------------ 2. metrics
def _pairs(rs, n, k_true, k_pred, kind):
    t = rs.randint(0, k_true, n)
    p = rs.randint(0, k_pred, n)
    if kind == "never_predicted":
        p[p == 1] = 0
    elif kind == "one_class":
        t[:] = k_true - 1
        p[:] = k_true - 1
    elif kind == "one_predicted":
        p[:] = 0
    elif kind == "permuted":
        p = (t + 1) % k_true
    return p, t


@pytest.mark.parametrize("kind", ["random", "never_predicted", "one_class", "one_predicted", "permuted"])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_metrics_agree_with_sklearn(kind, k):
    sk = pytest.importorskip("sklearn.metrics")
    from expertsim.train.diagnostics import agreement_metrics
    rs = np.random.RandomState(100 * k + len(kind))
    p, t = _pairs(rs, 200, k, k, kind)
    cm, invalid = R.confusion(p, t, k, k)
    assert invalid == 0 and cm.sum() == 200
    got, ref = agreement_metrics(cm), R.metrics(cm)
    pr, rc, f1, _ = sk.precision_recall_fscore_support(t, p, average="macro", zero_division=0)
    want = {"accuracy": sk.accuracy_score(t, p), "precision": pr, "recall": rc, "f1": f1,
            "adjusted_rand": sk.adjusted_rand_score(t, p)}
    for key, w in want.items():
        assert abs(got[key] - w) <= 1e-12, (key, got[key], w)
        assert abs(ref[key] - w) <= 1e-12, (key, ref[key], w)
    assert abs(got["matched_accuracy"] - ref["matched_accuracy"]) <= 1e-12
    assert got["matched_accuracy"] >= got["accuracy"] - 1e-15
    if kind == "permuted":
        assert got["matched_accuracy"] == 1.0 and got["adjusted_rand"] == 1.0 and got["accuracy"] == 0.0


def test_metrics_of_degenerate_and_rectangular_matrices():
    from expertsim.train.diagnostics import agreement_metrics
    z = agreement_metrics(np.zeros((3, 3), dtype=np.int64))
    assert z == {"accuracy": 0.0, "precision": 0.0, "recall": 0.0, "f1": 0.0, "adjusted_rand": 1.0,
                 "matched_accuracy": 0.0}
    cm = np.array([[5, 0, 1], [0, 7, 2]])                 # two true classes, three predicted
    got, ref = agreement_metrics(cm), R.metrics(cm)
    for key in got:
        assert abs(got[key] - ref[key]) <= 1e-12, key
    big = agreement_metrics(np.array([[2 ** 40, 3], [5, 2 ** 41]]))   # pair counts beyond int64
    assert 0.999999 < big["adjusted_rand"] < 1.0


# ------------------------------------------------------------------------------------------ 3. renumbering
def test_renumbering_rule():
    from expertsim.utils.clustering import renumber_by_brightness
    centres = np.array([[3.0, 1.0], [0.5, 0.5], [2.0, 2.0], [0.25, 0.75]])   # sums 4, 1, 4, 1
    order = renumber_by_brightness(centres)
    assert order.tolist() == [1, 3, 0, 2]                 # ascending sum, the original index first on a tie
    assert renumber_by_brightness(centres[order]).tolist() == [0, 1, 2, 3]


# ------------------------------------------------------------------------------------------ 4. prepare_dataset
def _frame(n, zdc):
    import pandas as pd
    from expertsim.utils.data_transformations import COND_COLUMNS
    return pd.DataFrame(np.zeros((n, len(COND_COLUMNS))), columns=COND_COLUMNS)


def test_prepare_dataset_rejects_n_clusters_misuse():
    from expertsim.utils.data_preparation import prepare_dataset
    images = np.zeros((4, 56, 30), dtype=np.float32)
    with pytest.raises(ValueError, match="proton"):
        prepare_dataset(np.zeros((4, 44, 44), dtype=np.float32), _frame(4, "neutron"), "neutron", n_clusters=2)
    with pytest.raises(ValueError, match="expert_number"):
        prepare_dataset(images, _frame(4, "proton"), "proton", n_clusters=2, expert_number=np.zeros(4))
    frame = _frame(4, "proton")
    frame["expert_number"] = 0
    with pytest.raises(ValueError, match="expert_number"):
        prepare_dataset(images, frame, "proton", n_clusters=2)
    with pytest.raises(ValueError, match="n_clusters"):
        prepare_dataset(images, _frame(4, "proton"), "proton", n_clusters=0)


# ------------------------------------------------------------------------------------------ 5. CLI
def test_cli_flags():
    import cli
    a = cli.parse_args(["--prepare", "--clusters", "4", "--cluster-seed", "7", "--cluster-restarts", "3"])
    assert (a.clusters, a.cluster_seed, a.cluster_restarts) == (4, 7, 3)
    a = cli.parse_args(["--prepare"])
    assert (a.clusters, a.cluster_seed, a.cluster_restarts) == (None, 0, 10)
    a = cli.parse_args(["--diagnose", "--expert-number", "e.npy"])
    assert a.expert_number == "e.npy" and cli.parse_args(["--diagnose"]).expert_number is None


# ------------------------------------------------------------------------------------------ 6. ABI
def test_header_declares_the_entries():
    assert _prototype("es_kmeans_assign") == [
        "const void* x", "int x_f64", "int64_t ld", "int rows", "int cols", "const double* centres", "int K",
        "const int32_t* label_old", "int32_t* label", "double* dist", "int64_t* changed", "double* inertia",
        "void* work", "size_t work_bytes", "es_stream_t stream"]
    assert _prototype("es_confusion_matrix") == [
        "const int32_t* pred", "const int32_t* target", "int64_t n", "int n_true", "int n_pred", "int64_t* counts",
        "int64_t* invalid", "es_stream_t stream"]
    src = open(HEADER).read()
    doc = src[src.index("Clustering (the proton"):src.index("int es_kmeans_trials")]
    for words in ("translation invariant", "mean-centring", "the lowest k on a tie", "no float atomics",
                  "one empty cluster only", "non-decreasing", "_relocate_empty_clusters_dense"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in ENTRIES.items():
        r, args = hip._SIGS[name]
        assert r is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(_prototype(name, res)), name
        assert hasattr(hip.lib(), name)
    src = open(HEADER).read()
    for macro, value in (("ES_KMEANS_MAX_COLS", hip.KMEANS_MAX_COLS), ("ES_KMEANS_MAX_K", hip.KMEANS_MAX_K),
                         ("ES_CONFUSION_MAX_CELLS", hip.CONFUSION_MAX_CELLS)):
        assert int(re.search(r"#define %s (\d+)" % macro, src).group(1)) == value
    assert hip.KMEANS_MAX_ROWS == 1 << 24 and "#define ES_KMEANS_MAX_ROWS (1 << 24)" in src
    for K in (1, 2, 3, 7, 8, 20, 21, 54, 55, 64):
        assert hip.lib().es_kmeans_trials(K) == R.trials(K)


def test_workspace_limits():
    from expertsim import hip
    ws, pp = hip.kmeans_workspace, hip.kmeans_plusplus_workspace
    assert ws(768, 1680, 4) > 0 and pp(768, 1680, 4) > 0
    for rows, cols, K in ((0, 4, 1), (4, 0, 1), (4, 4097, 1), (4, 4, 0), (100, 4, 65), (3, 4, 4), ((1 << 24) + 1, 4, 2)):
        assert ws(rows, cols, K) == 0 and pp(rows, cols, K) == 0, (rows, cols, K)
    assert ws(64, 4096, 64) > 0 and ws(1, 1, 1) > 0


def test_entries_reject_bad_arguments_before_any_launch():
    from expertsim import hip
    f = C.c_void_p(256)
    big = 1 << 30

    def assign(x=f, f64=0, ld=8, rows=16, cols=8, c=f, K=2, lo=None, lab=f, dist=f, ch=f, inert=f, work=f, wb=big):
        return hip.call("es_kmeans_assign", x, f64, ld, rows, cols, c, K, lo, lab, dist, ch, inert, work, wb, None)

    def update(x=f, f64=0, ld=8, rows=16, cols=8, lab=f, dist=f, co=f, K=2, cn=C.c_void_p(512), sh=f, work=f, wb=big):
        return hip.call("es_kmeans_update", x, f64, ld, rows, cols, lab, dist, co, K, cn, sh, work, wb, None)

    def pp(x=f, f64=0, ld=8, rows=16, cols=8, K=2, u=f, trials=2, c=f, idx=f, work=f, wb=big):
        return hip.call("es_kmeans_plusplus", x, f64, ld, rows, cols, K, u, trials, c, idx, work, wb, None)

    def cm(p=f, t=f, n=4, nt=2, npred=2, counts=f, inv=f):
        return hip.call("es_confusion_matrix", p, t, n, nt, npred, counts, inv, None)

    bad = [lambda: assign(x=None), lambda: assign(f64=2), lambda: assign(ld=7), lambda: assign(cols=4097, ld=4097),
           lambda: assign(K=0), lambda: assign(K=65, rows=100), lambda: assign(K=17), lambda: assign(rows=0),
           lambda: assign(lo=f), lambda: assign(wb=8), lambda: assign(work=None), lambda: assign(ch=None),
           lambda: update(cn=f), lambda: update(K=17), lambda: update(wb=8), lambda: update(dist=None),
           lambda: pp(trials=0), lambda: pp(trials=9), lambda: pp(u=None), lambda: pp(wb=8), lambda: pp(K=17),
           lambda: cm(nt=0), lambda: cm(nt=65, npred=64), lambda: cm(n=-1), lambda: cm(p=None), lambda: cm(counts=None)]
    for i, fn in enumerate(bad):
        with pytest.raises(hip.HipError):
            fn()
        assert hip.lib().es_last_error(), i
