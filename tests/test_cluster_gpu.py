"""Clustering on the GPU: es_kmeans_assign / es_kmeans_update / es_kmeans_plusplus / es_confusion_matrix against
scikit-learn's record (tests/golden/kmeans_sklearn.npz) and the numpy restatement (tests/cluster_refs.py), then
the wiring: cluster_images, prepare_dataset(n_clusters=), evaluate_router, diagnose(expert_number=) and the CLI.

Tolerances (include/expertsim_hip.h fixes every summation order, but not to numpy's, so nothing here is bitwise
against the host):
* labels and n_iter equal -- the golden tool asserted, over every iteration, a relative gap of at least 1e-7
  between a row's nearest and second-nearest centre and |shift - threshold| / threshold >= 1e-6, six orders
  above the cols 2^-52 relative error of a distance;
* centres within n_max 2^-52 max|x| (n_max the largest cluster): with equal labels a centre is a plain mean of
  at most n_max values of magnitude at most max|x|, so nothing compounds over the iterations;
* inertia within N cols 2^-52 relative: a sum of N cols non-negative terms;
* a rerun is bitwise equal.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cluster_refs as R
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _bits(t):
    return t.detach().cpu().reshape(-1).numpy().tobytes()


def _check(got, want, X):
    """kmeans_raw's 4-tuple against (labels, centres, inertia, n_iter) of the record / the restatement."""
    labels, centres, inertia, n_iter = got
    w_labels, w_centres, w_inertia, w_iter = want
    assert labels.dtype == torch.int32 and centres.dtype == torch.float64 and inertia.dtype == torch.float64
    labels, centres, inertia = labels.cpu().numpy(), centres.cpu().numpy(), float(inertia)
    print(f"n_iter {n_iter} / {w_iter}  labels differing {int((labels != w_labels).sum())}  "
          f"centres {np.abs(centres - w_centres).max():.3g}  inertia {inertia!r} / {float(w_inertia)!r}")
    assert n_iter == int(w_iter)
    assert np.array_equal(labels, w_labels)
    n_max = np.bincount(labels).max()
    assert np.abs(centres - w_centres).max() <= n_max * EPS * np.abs(X).max()
    assert abs(inertia - float(w_inertia)) <= X.size * EPS * float(w_inertia)


# --------------------------------------------------------------------------------------- 1. the record
@pytest.mark.parametrize("case", R.CASES)
def test_kmeans_raw_reproduces_sklearn(golden, case):
    from expertsim.utils.clustering import kmeans_raw
    images = golden["neutron_images" if case == "neutron" else "proton_images"]
    x = torch.from_numpy(images.reshape(len(images), -1)).to(DEV)          # fp32, as stored
    init = golden[f"{case}_init"]
    got = kmeans_raw(x, init)
    _check(got, (golden[f"{case}_labels"], golden[f"{case}_centres"], golden[f"{case}_inertia"],
                 golden[f"{case}_n_iter"]), images.astype(np.float64))
    again = kmeans_raw(x, torch.from_numpy(init).to(DEV))
    assert again[3] == got[3] and all(_bits(a) == _bits(b) for a, b in zip(again[:3], got[:3]))


# --------------------------------------------------------------------------------------- 2. the restatement
def _blobs(rows, cols, modes, seed, dtype):
    rs = np.random.RandomState(seed)
    centre = rs.uniform(-4.0, 4.0, (modes, cols))
    x = centre[rs.randint(0, modes, rows)] + rs.normal(0.0, 1.0, (rows, cols))
    return x.astype(dtype)


def _device(x, pad):
    if not pad:
        return torch.from_numpy(x).to(DEV)
    buf = torch.full((x.shape[0], x.shape[1] + pad), 1e30, dtype=torch.from_numpy(x).dtype, device=DEV)
    view = buf[:, :x.shape[1]]
    view.copy_(torch.from_numpy(x))
    assert view.stride(0) == x.shape[1] + pad
    return view


# rows 1 | 63 | 1025 (one wave, under a workgroup step, past a 4-chunk update and a reduction chunk boundary);
# cols 1 | 37 | 64 | 65 | 4096 (one lane, a partial sweep, the wave width and one past it, the cap);
# K 1, K = rows, K = 64, 9 (two sweeps of 8 centres); K cols 8 = 64 KiB is the last shape with the centres in LDS
# and 1025 x 4096 x 3 the first from global memory; a padded row stride; fp64 input; a tolerance stop
SHAPES = [(1, 1, 1, np.float32, 0, 1e-4), (63, 1, 3, np.float32, 0, 1e-4), (63, 37, 63, np.float32, 0, 1e-4),
          (1025, 64, 64, np.float32, 0, 1e-4), (1025, 65, 5, np.float32, 3, 1e-4),
          (63, 4096, 2, np.float32, 0, 1e-4), (1025, 4096, 3, np.float32, 0, 1e-4),
          (1025, 37, 9, np.float64, 1, 1e-4), (1025, 37, 5, np.float32, 0, 0.05)]


@pytest.mark.parametrize("rows,cols,K,dtype,pad,tol", SHAPES)
def test_kmeans_raw_equals_the_restatement(rows, cols, K, dtype, pad, tol):
    from expertsim.utils.clustering import kmeans_raw
    x = _blobs(rows, cols, min(K, 7), 1000 + rows + cols + K, dtype)
    init = x[np.random.RandomState(5).choice(rows, K, replace=False)].astype(np.float64)
    X = x.astype(np.float64)
    want = R.lloyd(X, init, tol=tol)
    if tol > 1e-4:
        assert want[3] < R.lloyd(X, init)[3], "the tolerance did not stop the run: the case shows nothing"
    _check(kmeans_raw(_device(x, pad), init, tol=tol), want, X)


def test_duplicate_rows_tie_goes_to_the_lowest_centre_and_the_empty_cluster_is_refilled():
    from expertsim.utils.clustering import _Lloyd, kmeans_raw
    x = _blobs(200, 65, 3, 77, np.float32)
    x[10] = x[3]                                                       # a duplicate row
    init = x[[3, 10, 150]].astype(np.float64)                          # centres 0 and 1 are equal
    xd = torch.from_numpy(x).to(DEV)
    run = _Lloyd(xd, 3)
    centres = torch.from_numpy(init).to(DEV)
    run.assign(centres, run.labels[0], None)
    labels = run.labels[0].cpu().numpy()
    d = R.sq_dist(x, init)
    assert np.array_equal(labels, d.argmin(axis=1)) and not (labels == 1).any() and (labels == 0).any()
    dist = run.dist.cpu().numpy()
    assert dist[3] == 0.0 and dist[10] == 0.0                          # the difference form: exactly zero
    assert np.abs(dist - d.min(axis=1)).max() <= 65 * EPS * d.max()
    stat = run.stat.cpu().numpy()
    assert int(stat.view(np.int64)[0]) == 200 and abs(stat[1] - dist.sum()) <= 200 * EPS * dist.sum()
    run.labels[1].copy_(run.labels[0])
    run.labels[1][:7] += 1
    run.assign(centres, run.labels[0], run.labels[1])                  # against other labels: 7 rows changed
    assert int(run.stat.cpu().numpy().view(np.int64)[0]) == 7
    X = x.astype(np.float64)
    for max_iter in (1, 300):                                          # the relocation alone, then the whole run
        trace = {}
        want = R.lloyd(X, init, max_iter=max_iter, trace=trace)
        assert trace["relocated"][0] == 1
        _check(kmeans_raw(xd, init, max_iter=max_iter), want, X)


# --------------------------------------------------------------------------------------- 3. k-means++
def test_plusplus_reproduces_the_record(golden):
    from expertsim.utils.clustering import kmeans_plusplus_raw
    images = golden["proton_images"]
    x = torch.from_numpy(images.reshape(len(images), -1)).to(DEV)
    centres, index = kmeans_plusplus_raw(x, 8, golden["pp_draws"])
    assert np.array_equal(index.cpu().numpy(), golden["pp_index"])
    assert np.array_equal(centres.cpu().numpy(), images.reshape(len(images), -1).astype(np.float64)[golden["pp_index"]])
    again = kmeans_plusplus_raw(x, 8, torch.from_numpy(golden["pp_draws"]).to(DEV))
    assert _bits(again[0]) == _bits(centres) and _bits(again[1]) == _bits(index)


@pytest.mark.parametrize("rows,cols,K,dtype,pad", [(1025, 37, 64, np.float64, 2), (63, 65, 63, np.float32, 0),
                                                   (1, 5, 1, np.float32, 0), (2049, 1, 3, np.float32, 0)])
def test_plusplus_equals_the_restatement(rows, cols, K, dtype, pad):
    from expertsim.utils.clustering import kmeans_plusplus_raw, kmeans_trials
    x = _blobs(rows, cols, 5, 31 + rows, dtype)
    u = np.random.RandomState(rows + K).rand(K, kmeans_trials(K))
    trace = {}
    want, _ = R.plusplus(x, K, u, trace=trace)
    assert trace["search_gap"] >= 1e-11 and trace["pot_gap"] >= 1e-11, trace   # else: choose another seed
    centres, index = kmeans_plusplus_raw(_device(x, pad), K, u)
    assert np.array_equal(index.cpu().numpy(), want)
    assert np.array_equal(centres.cpu().numpy(), x.astype(np.float64)[want])


# --------------------------------------------------------------------------------------- 4. confusion matrix
@pytest.mark.parametrize("n", [1, 1000, 1 << 20])
def test_confusion_matrix_equals_add_at(n):
    from expertsim.train.diagnostics import confusion_matrix
    rs = np.random.RandomState(n % 1000)
    n_true, n_pred = 5, 7
    pred = rs.randint(-1, n_pred + 2, n).astype(np.int32)                # -1, n_pred and n_pred + 1 are outside
    target = rs.randint(-2, n_true + 1, n).astype(np.int64)
    want, invalid = R.confusion(pred, target, n_pred, n_true)
    counts, bad = confusion_matrix(torch.from_numpy(pred).to(DEV), torch.from_numpy(target), n_pred, n_true)
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want) and int(bad) == invalid
    assert int(counts.sum()) + int(bad) == n
    again = confusion_matrix(pred, target, n_pred, n_true)
    assert _bits(again[0]) == _bits(counts) and _bits(again[1]) == _bits(bad)


def test_confusion_matrix_limits():
    from expertsim.train.diagnostics import confusion_matrix
    counts, bad = confusion_matrix(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 64, 64)
    assert tuple(counts.shape) == (64, 64) and int(counts.sum()) == 0 and int(bad) == 0
    full = confusion_matrix(np.full(3000, 63), np.full(3000, 63), 64, 64)[0]
    assert int(full[63, 63]) == 3000 and int(full.sum()) == 3000
    with pytest.raises(ValueError):
        confusion_matrix(np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64), 65, 64)
    with pytest.raises(ValueError):
        confusion_matrix(np.zeros(4), np.zeros(4, dtype=np.int64), 2, 2)


# --------------------------------------------------------------------------------------- 5. wiring
def test_kmeans_restarts_equal_the_restatement_and_rerun(golden):
    from expertsim.utils.clustering import kmeans, kmeans_trials
    images = golden["proton_images"]
    X = images.reshape(len(images), -1).astype(np.float64)
    K, seed, n_init = 4, 5, 3
    runs = []
    for r in range(n_init):
        u = np.random.Generator(np.random.Philox(key=[seed, r])).random((K, kmeans_trials(K)))
        index, _ = R.plusplus(X, K, u)
        runs.append(R.lloyd(X, X[index]))
    best = runs[int(np.argmin([r[2] for r in runs]))]
    x = torch.from_numpy(images.reshape(len(images), -1)).to(DEV)
    got = kmeans(x, K, n_init=n_init, seed=seed)
    _check(got, best, X)
    again = kmeans(x, K, n_init=n_init, seed=seed)
    assert again[3] == got[3] and all(_bits(a) == _bits(b) for a, b in zip(again[:3], got[:3]))
    other = kmeans(x, K, init="random", n_init=2, seed=seed)
    assert float(other[2]) > 0 and other[0].shape == (len(images),)
    with pytest.raises(ValueError):
        kmeans(x, K, init="farthest")
    with pytest.raises(ValueError):
        kmeans(x[:3], K)


def test_cluster_images_does_not_depend_on_the_order_of_the_init(golden):
    from expertsim.utils.clustering import cluster_images
    images = golden["proton_images"]
    init = golden["proton_init"]
    a = cluster_images(images, 4, init=init)
    b = cluster_images(torch.from_numpy(images).to(DEV), 4, init=init[[2, 0, 3, 1]])
    assert a[0].dtype == torch.int64 and tuple(a[0].shape) == (len(images),) and tuple(a[1].shape) == (4, 56 * 30)
    assert _bits(a[0]) == _bits(b[0]) and _bits(a[1]) == _bits(b[1]) and _bits(a[2]) == _bits(b[2])
    brightness = a[1].sum(dim=1).cpu().numpy()
    assert (np.diff(brightness) > 0).all()                             # cluster 0 is the faintest
    order = np.argsort(golden["proton_centres"].sum(axis=1), kind="stable")
    rank = np.empty(4, dtype=np.int64)
    rank[order] = np.arange(4)
    assert np.array_equal(a[0].cpu().numpy(), rank[golden["proton_labels"]])


def _cfg(paths, tmp):
    from expertsim.config import AttrDict as A
    return A(limit_samples=None, config=A(run_name="t", experiment_dir=str(tmp / "exp")), model=A(architecture="proton"),
             dataset=A(zdc_type="proton", source="pickle", MIN_INTENSITY_THRESHOLD=None, MAX_INTENSITY_THRESHOLD=None,
                       read_n_samples=None, shuffle_train_test_split=False, test_size=0.25, resident=True,
                       input_image_shape=[56, 30], **paths),
             train=A(save_experiments_dir=str(tmp), checkpoint_experiment_dir=None, epoch_to_load=None,
                     save_experiment_data=False, batch_size=16))


def _conditions(n):
    rs = np.random.RandomState(9)
    cond = np.repeat(rs.randint(0, 3, (n // 4, 9)).astype(np.float64), 4, axis=0)
    cond[:, 0] += np.repeat(np.arange(n // 4), 4) * 10.0                 # n / 4 distinct rows of 4 samples
    return cond


def test_prepare_dataset_with_clusters_round_trip(golden, tmp_path):
    pd = pytest.importorskip("pandas")
    from expertsim.utils import data_preparation as DP
    from expertsim.utils import data_transformations as DT
    from expertsim.utils.clustering import cluster_images
    images = golden["proton_images"][:256]
    frame = pd.DataFrame(_conditions(256), columns=DT.COND_COLUMNS)
    out_images, cond, pos = DP.prepare_dataset(images, frame, "proton", n_clusters=3, cluster_seed=2, cluster_restarts=2)
    want = cluster_images(images, 3, n_init=2, seed=2)[0].cpu().numpy()
    en = cond["expert_number"].to_numpy()
    assert en.dtype == np.int64 and np.array_equal(en, want) and set(en.tolist()) == {0, 1, 2}
    plain = DP.prepare_dataset(images, frame, "proton")[1]                # without n_clusters: today's zeros
    assert (plain["expert_number"] == 0).all()
    assert plain.drop(columns="expert_number").equals(cond.drop(columns="expert_number"))
    # the photon-sum filter comes first: the clustering is that of the kept images
    ps = cond["proton_photon_sum"].to_numpy()
    lo = float(np.quantile(ps, 0.2))
    cond2 = DP.prepare_dataset(images, frame, "proton", lo, None, n_clusters=3, cluster_seed=2, cluster_restarts=2)[1]
    keep = ps >= lo
    assert np.array_equal(cond2["expert_number"], cluster_images(images[keep], 3, n_init=2, seed=2)[0].cpu().numpy())
    paths = DP.write_dataset(tmp_path / "data", "proton", out_images, cond, pos)
    cfg = _cfg(paths, tmp_path)
    data, data_cond, data_posi = DT.get_dataset(cfg)
    assert np.array_equal(data_cond["expert_number"], want)
    out = DT.transform_data_for_training(cfg, data, data_cond, data_posi)
    en_train, en_test = out[12], out[13]
    assert np.array_equal(en_train, want[:192]) and np.array_equal(en_test, want[192:])
    assert len(out[0]) == 192 and len(out[1]) == 64


class _FixedRouter(torch.nn.Module):
    """A router whose scores are given: evaluate_router's own arithmetic is what the test checks."""

    def __init__(self, scores):
        super().__init__()
        self.scores = scores

    def forward(self, y):
        return self.scores[:y.shape[0]]


def test_evaluate_router_equals_the_restatement():
    from expertsim.models import build_model
    from expertsim.train.utils import evaluate_router
    rs = np.random.RandomState(12)
    n, E = 500, 4
    scores = torch.from_numpy(rs.rand(n, E).astype(np.float32)).to(DEV)
    target = rs.randint(0, E, n)
    target[target == 3] = 1                                              # class 3 never occurs in the target
    pred = scores.argmax(dim=1).cpu().numpy()
    want = R.metrics(R.confusion(pred, target, E, E)[0])
    router = _FixedRouter(scores)
    router.train()
    got = evaluate_router(router, torch.zeros(n, 9), torch.from_numpy(target).to(DEV))
    assert not router.training and isinstance(got, tuple) and len(got) == 4
    for g, key in zip(got, ("accuracy", "precision", "recall", "f1")):
        assert isinstance(g, float) and abs(g - want[key]) <= 1e-12, key
    # a given metric is called as the reference calls it; the others are still computed
    calls = []

    def metric(p, t):
        calls.append((p, t))
        return torch.tensor(0.25, device=DEV)

    mixed = evaluate_router(router, torch.zeros(n, 9), target, None, metric, None, metric)
    assert mixed == (got[0], 0.25, got[2], 0.25) and len(calls) == 2
    assert np.array_equal(calls[0][0].cpu().numpy(), pred) and np.array_equal(calls[0][1].cpu().numpy(), target)
    # the project's router: read through its logits, the arg-max free of the Gumbel draw
    torch.manual_seed(1)
    real = build_model("router_v1", dict(cond_dim=9, n_experts=3), DEV)
    y = torch.from_numpy(rs.normal(size=(300, 9)).astype(np.float32))
    expo = torch.ones(300, 3, device=DEV)
    idx = real.fwd(y.to(DEV), expo, 1.0)[2].cpu().numpy()                # ones: the arg-max of the logits
    t3 = rs.randint(0, 3, 300)
    got3 = evaluate_router(real, y, t3)
    want3 = R.metrics(R.confusion(idx, t3, 3, 3)[0])
    assert got3 == evaluate_router(real, y, t3)
    for g, key in zip(got3, ("accuracy", "precision", "recall", "f1")):
        assert abs(g - want3[key]) <= 1e-12, key


def _moe(E):
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", "train.precision=fp32", "model.router.diff_strength=1e-6"])
    torch.manual_seed(4)
    moe = setup_moe_system(cfg, torch.device(DEV))
    moe.eval()
    moe.eval_batch_size = 128
    return moe, cfg


def _agreement_want(expert, target, E):
    n_true = max(E, int(target.max()) + 1)
    cm, invalid = R.confusion(expert, target, E, n_true)
    return cm, invalid, R.metrics(cm)


def _check_agreement(got, expert, target, E):
    cm, invalid, want = _agreement_want(expert, target, E)
    assert np.array_equal(got["confusion"], cm) and got["invalid"] == invalid
    for key, w in want.items():
        assert abs(float(got[key]) - w) <= 1e-12, key


def test_diagnose_with_expert_number():
    from expertsim.train.diagnostics import DIAGNOSTIC_KEYS
    from expertsim.utils.synthetic import make_batch
    E, N, seed = 4, 257, 13
    moe, _ = _moe(E)
    cond = torch.from_numpy(make_batch(N, "neutron", seed=11)["cond"].astype(np.float32)).to(DEV)
    target = np.random.RandomState(3).randint(0, 5, N)                   # five classes against four experts
    plain = moe.diagnose(cond, seed=seed)
    assert set(plain) == set(DIAGNOSTIC_KEYS)                            # without the vector: today's dict
    diag = moe.diagnose(cond, seed=seed, expert_number=target)
    assert set(diag) == set(DIAGNOSTIC_KEYS) | {"router_agreement"}
    assert all(np.array_equal(diag[k], plain[k], equal_nan=True) for k in plain)
    expert = moe.simulate(cond, seed=seed, domain="photons")["expert"].cpu().numpy()
    assert diag["router_agreement"]["confusion"].shape == (5, 4)
    _check_agreement(diag["router_agreement"], expert, target, E)
    with pytest.raises(ValueError):
        moe.diagnose(cond, seed=seed, expert_number=target[:-1])


def test_cli_prepare_with_clusters(golden, tmp_path):
    pd = pytest.importorskip("pandas")
    from expertsim.utils.clustering import cluster_images
    images = golden["proton_images"][:128]
    np.save(tmp_path / "images.npy", images)
    np.save(tmp_path / "cond.npy", _conditions(128))
    out = tmp_path / "prepared"
    r = subprocess.run([sys.executable, os.path.join(REPO, "cli.py"), "-o", "dataset.zdc_type=proton", "--prepare",
                        "--images", str(tmp_path / "images.npy"), "--conditions", str(tmp_path / "cond.npy"),
                        "--out-dir", str(out), "--clusters", "3", "--cluster-seed", "4", "--cluster-restarts", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Prepared 128 proton samples" in r.stdout and "writing zeros" not in r.stdout
    path = [kv.split("=", 1)[1] for line in r.stdout.splitlines() if "Wrote " in line
            for kv in line.split("Wrote ")[1].split() if kv.startswith("dataset.DATA_COND_PATH=")][0]
    frame = pd.read_pickle(path)
    want = cluster_images(images, 3, n_init=2, seed=4)[0].cpu().numpy()
    assert np.array_equal(frame["expert_number"], want) and len(set(want.tolist())) == 3


def test_cli_diagnose_with_expert_number(tmp_path):
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    from expertsim.utils.synthetic import make_batch
    E = 4
    moe, cfg = _moe(E)
    models = tmp_path / "models"
    models.mkdir()
    save_checkpoint(str(models), 0, moe, *setup_optimizers(moe, cfg))
    cond = make_batch(64, "neutron", seed=11)["cond"]
    target = np.random.RandomState(6).randint(0, E, 64)
    np.save(tmp_path / "cond.npy", cond)
    np.save(tmp_path / "expert_number.npy", target)
    r = subprocess.run([sys.executable, os.path.join(REPO, "cli.py"), "-o", "model.architecture=neutron",
                        "dataset.input_image_shape=[44,44]", f"model.n_experts={E}", "model.router.diff_strength=1e-6",
                        "train.precision=fp32", "--diagnose", "--checkpoint", str(models), "--conditions",
                        str(tmp_path / "cond.npy"), "--out", str(tmp_path / "diag.npz"), "--seed", "3",
                        "--expert-number", str(tmp_path / "expert_number.npy")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(tmp_path / "diag.npz")
    expert = moe.simulate(torch.from_numpy(cond.astype(np.float32)).to(DEV), seed=3, domain="photons")["expert"]
    got = {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith("router_agreement.")}
    assert set(got) == {"confusion", "invalid", "accuracy", "precision", "recall", "f1", "adjusted_rand",
                        "matched_accuracy"}
    _check_agreement({k: (v if k == "confusion" else v.item()) for k, v in got.items()}, expert.cpu().numpy(), target, E)
