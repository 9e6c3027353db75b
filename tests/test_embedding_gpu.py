"""es_pca_project / es_tsne_affinities / es_tsne_gradient / es_tsne_run on the device against tests/embed_refs.py
and tests/golden/tsne_sklearn.npz, and MoEWrapper.diagnose(embedding=True) / loop.evaluate_epoch
(train.eval_embedding) end to end.

Bounds (tests/embed_refs.py has the derivations): mean, dmin bitwise; PCA residual within 40 cols 2^-52 lambda_1,
components within Davis-Kahan of it; entropy within 1e-5 + H_SLACK; gradient, Z and KL within grad_bounds();
the 10-iteration trajectory within 8 times the restatement's own fp32-gradient sensitivity; the golden's final KL
within sklearn's own spread over inits.  Every test prints its worst error / bound ratio before it asserts.

Worst error / bound seen on an MI355X (one run): PCA residual 0.022, components 0.002; entropy 0.9987 (the search
stops just inside its 1e-5); gradient 0.069 (4097 rows: 0.044), Z 0.018, KL 0.0046; trajectory 7.0 of the allowed
8 (device 8.3e-7, the restatement's own fp32-gradient deviation 1.2e-7); the golden's final KL 1.13250 against
sklearn's 1.13505 (limit 1.14987), purity 1.0."""
import functools

import numpy as np
import pytest
import torch

import embed_refs as ER

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _clusters(n, cols, seed, dup=None):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, 4.0, (3, cols))
    x = (centres[rng.integers(0, 3, n)] + rng.normal(0.0, 1.0, (n, cols))).astype(np.float32)
    if dup is not None:
        x[dup[0]:dup[1]] = x[dup[0]]
    return x


# ------------------------------------------------------------------------------------------ PCA
def _pca_data(rows, cols, dtype, seed, const=None):
    """Independent columns of standard deviation 4 * 0.7^c, mixed by a random rotation: well-separated leading
    eigenvalues.  const: that column is constant afterwards."""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.0, 1.0, (rows, cols)) * (4.0 * 0.7 ** np.arange(cols))
    q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (cols, cols)))
    x = (z @ q.T + rng.normal(0.0, 3.0, cols)).astype(dtype)
    if const is not None:
        x[:, const] = 0.375
    return x


PCA_CASES = {"f32_257x9": (257, 9, np.float32, 0, None), "f64_1000x9_ld12": (1000, 9, np.float64, 3, None),
             "f32_300x1": (300, 1, np.float32, 0, None), "f64_300x64": (300, 64, np.float64, 0, None),
             "f32_257x9_const": (257, 9, np.float32, 2, 4)}


@pytest.mark.parametrize("case", list(PCA_CASES))
def test_pca_project(case):
    from expertsim.train.embedding import pca_project
    rows, cols, dtype, pad, const = PCA_CASES[case]
    k = min(3, cols)
    x = _pca_data(rows, cols, dtype, 11, const)
    full = torch.full((rows, cols + pad), float("nan"), device=DEV, dtype=torch.float64 if dtype == np.float64
                      else torch.float32)
    full[:, :cols] = _dev(x)
    xd = full[:, :cols]
    out = pca_project(xd, k)
    again = pca_project(xd, k)
    got = {n: v.cpu().numpy() for n, v in out.items()}
    for n in out:                                              # a rerun is bit-equal
        assert torch.equal(out[n].view(torch.int64), again[n].view(torch.int64)), n
    ref = ER.pca_ref(x, k)
    assert np.array_equal(got["mean"], ref["mean"])            # the fixed order of the header, bit for bit
    lam1 = ref["eigenvalues"][0]
    bound = ER.pca_residual_bound(cols, lam1)
    wide = x.astype(np.float64)
    worst_res = worst_dk = 0.0
    for m in range(k):
        v, lam = got["components"][m], got["explained_variance"][m]
        res = np.linalg.norm(ref["cov"] @ v - lam * v)
        worst_res = max(worst_res, res / bound)
        assert abs(np.linalg.norm(v) - 1.0) <= 8 * cols * ER.U
        assert v[np.argmax(np.abs(v))] > 0                     # the sign rule
        others = np.delete(ref["eigenvalues"], m)
        gap = np.abs(others - ref["eigenvalues"][m]).min() if others.size else np.inf
        dk = max(4.0 * bound / gap, 1e-300)
        err = np.abs(v - ref["components"][m]).max()
        worst_dk = max(worst_dk, err / dk)
        assert abs(lam - ref["explained_variance"][m]) <= bound
        if const is not None:
            assert abs(v[const]) <= dk
    print(f"{case}: residual / bound {worst_res:.3f}, component error / Davis-Kahan {worst_dk:.3f}")
    assert worst_res <= 1.0 and worst_dk <= 1.0
    trace = np.trace(ref["cov"])
    assert np.abs(got["explained_variance_ratio"] - got["explained_variance"] / trace).max() <= 8 * cols * ER.U
    # scores: the device's own components to rounding, the restatement's within the components' bound
    centred = wide - got["mean"]
    own = centred @ got["components"].T
    rounding = (cols + 2) * ER.U * (np.abs(centred) @ np.abs(got["components"]).T) + 1e-300
    assert (np.abs(got["scores"] - own) <= rounding).all()
    for m in range(k):
        others = np.delete(ref["eigenvalues"], m)
        dk = 4.0 * bound / np.abs(others - ref["eigenvalues"][m]).min() if others.size else 0.0
        slack = np.linalg.norm(centred, axis=1) * dk * np.sqrt(cols) + rounding[:, m]
        assert (np.abs(got["scores"][:, m] - ref["scores"][:, m]) <= slack).all()


# ------------------------------------------------------------------------------------------ affinities
@functools.lru_cache(maxsize=None)
def _aff_case(rows):
    x = _clusters(rows, 9, 20 + rows, dup=(10, 50) if rows == 300 else None)
    return x, ER.affinities_ref(x, 30.0)


def _device_affinities(x, perplexity=30.0, pad=0):
    from expertsim.train.embedding import tsne_affinities
    full = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=DEV, dtype=torch.float32)
    full[:, :x.shape[1]] = _dev(x)
    xd = full[:, :x.shape[1]]
    return xd, tsne_affinities(xd, perplexity)


@pytest.mark.parametrize("rows", [255, 256, 257, 300])
def test_tsne_affinities(rows):
    x, ref = _aff_case(rows)
    _, aff = _device_affinities(x, pad=rows % 2)
    got = {k: v.cpu().numpy() for k, v in aff.items()}
    assert np.array_equal(got["dmin"].view(np.int32), ref["dmin"].view(np.int32))          # bitwise
    assert np.isfinite(got["beta"]).all() and np.isfinite(got["log_s"]).all()
    d, target, slack = ref["d"], np.log(30.0), ER.h_slack(rows)
    worst = 0.0
    for i in np.flatnonzero(ref["converged"]):
        dd = np.delete(d[i].astype(np.float64) - np.float64(got["dmin"][i]), i)
        H, lS = ER.entropy(got["beta"][i], dd)
        worst = max(worst, abs(H - target) / (1e-5 + slack))
        assert abs(lS - got["log_s"][i]) <= slack
        assert got["steps"][i] == ref["steps"][i] or got["steps"][i] < 100
    print(f"rows {rows}: worst |H - log 30| / (1e-5 + slack) {worst:.4f} over {int(ref['converged'].sum())} rows")
    assert worst <= 1.0
    stuck = np.flatnonzero(~ref["converged"])
    if rows == 300:
        assert set(range(10, 50)) <= set(stuck.tolist())
    else:
        assert stuck.size == 0
    cond = ER.conditional_P(got["beta"], got["log_s"], got["dmin"], d)
    for i in stuck:                                            # unreachable on the device too
        assert got["steps"][i] == 100 and np.isfinite(got["beta"][i])
        near = np.flatnonzero((d[i] == got["dmin"][i]) & (np.arange(rows) != i))
        assert near.size >= 30
        assert np.abs(cond[i, near] - 1.0 / near.size).max() <= 1e-12
    again = _device_affinities(x, pad=rows % 2)[1]
    assert all(torch.equal(aff[k], again[k]) for k in aff)


def test_tsne_affinities_largest_perplexity():
    x = _clusters(64, 9, 3)
    _, aff = _device_affinities(x, perplexity=63.0)
    assert all(bool(torch.isfinite(aff[k].double()).all()) for k in ("beta", "log_s", "dmin"))
    assert int(aff["steps"].min()) >= 1 and int(aff["steps"].max()) <= 100 and float(aff["beta"].min()) > 0


# ------------------------------------------------------------------------------------------ gradient
@functools.lru_cache(maxsize=None)
def _grad_case(rows, cols):
    """x, the device's affinities (host copies) and the dense fp64 P they define."""
    x = _clusters(rows, cols, 40 + rows + cols, dup=(10, 50) if rows == 300 else None)
    xd, aff = _device_affinities(x)
    host = {k: v.cpu().numpy() for k, v in aff.items()}
    d = ER.dist32(x)
    return x, host, d, ER.joint_P(host["beta"], host["log_s"], host["dmin"], d)


GRAD_CASES = [(rows, 9, a, scale) for rows in (257, 300) for a in (12.0, 1.0) for scale in (1e-4, 5.0, 50.0)]
GRAD_CASES += [(257, cols, 12.0, 5.0) for cols in (5, 20, 40)]           # the other column widths of the pair pass


@pytest.mark.parametrize("rows,cols,a,scale", GRAD_CASES)
def test_tsne_gradient(rows, cols, a, scale):
    """rows 257: the second j split holds one column; rows 300: its last tile holds 12 of 32 (ragged tile and
    split), and rows 10..49 are duplicates."""
    from expertsim.train.embedding import tsne_gradient
    x, host, d, P = _grad_case(rows, cols)
    y = np.random.default_rng(int(rows + cols + 10 * a)).normal(0.0, scale, (rows, 2)).astype(np.float32)
    aff = {k: _dev(v) for k, v in host.items()}
    g, zkl = tsne_gradient(_dev(x), aff, _dev(y), a)
    g2, zkl2 = tsne_gradient(_dev(x), aff, _dev(y), a)
    assert torch.equal(g, g2) and torch.equal(zkl, zkl2)
    g, zkl = g.cpu().numpy(), zkl.cpu().numpy()
    g_ref, Z_ref, KL_ref = ER.gradient_ref(P, y, a)
    gb, zb, kb = ER.grad_bounds(P, y, a, host["beta"], host["log_s"], host["dmin"], d)
    rg = float((np.abs(g - g_ref) / gb).max())
    rz, rk = abs(zkl[0] - Z_ref) / zb, abs(zkl[1] - KL_ref) / kb
    print(f"rows {rows} cols {cols} a {a} scale {scale}: error / bound  g {rg:.4f}  Z {rz:.4f}  KL {rk:.4f}"
          f"  (|g| max {np.abs(g_ref).max():.3e}, relative error {np.abs(g - g_ref).max() / np.abs(g_ref).max():.2e})")
    assert np.isfinite(g).all() and rg <= 1.0 and rz <= 1.0 and rk <= 1.0


def test_tsne_gradient_sixteen_splits():
    """4097 rows: the most j splits (16 of 384 columns; the last five are empty, the eleventh ragged) and 17 row
    tiles.  g of 48 rows (the first, the last and rows of the ragged row tile among them) and Z against the
    restatement's row form; same bound as above."""
    from expertsim.train.embedding import tsne_affinities, tsne_gradient
    rows, a = 4097, 12.0
    x = _clusters(rows, 9, 91)
    y = np.random.default_rng(92).normal(0.0, 5.0, (rows, 2)).astype(np.float32)
    aff = tsne_affinities(_dev(x), 30.0)
    host = {k: v.cpu().numpy() for k, v in aff.items()}
    g, zkl = tsne_gradient(_dev(x), aff, _dev(y), a)
    g, zkl = g.cpu().numpy(), zkl.cpu().numpy()
    idx = np.unique(np.concatenate([[0, 1, 255, 256, 4095, 4096], np.random.default_rng(93).integers(0, rows, 42)]))
    g_ref, Z_ref, gb, zb = ER.gradient_rows_ref(idx, x, y, a, host["beta"], host["log_s"], host["dmin"])
    rg, rz = float((np.abs(g[idx] - g_ref) / gb).max()), abs(zkl[0] - Z_ref) / zb
    print(f"rows {rows}: error / bound  g {rg:.4f}  Z {rz:.4f}")
    assert np.isfinite(g).all() and np.isfinite(zkl).all() and rg <= 1.0 and rz <= 1.0


# ------------------------------------------------------------------------------------------ trajectory
def _run_device(x, host, y0, n_iter, iter0=0, state=None, log=None, **kw):
    from expertsim.train.embedding import tsne_run
    aff = {k: _dev(v) for k, v in host.items()}
    if state is None:
        y = _dev(y0).clone()
        upd = torch.zeros(len(y0), 2, dtype=torch.float64, device=DEV)
        gains = torch.ones(len(y0), 2, dtype=torch.float64, device=DEV)
    else:
        y, upd, gains = state
    log = tsne_run(_dev(x), aff, y, upd, gains, n_iter, iter0, log, **kw)
    return (y, upd, gains), log


def test_tsne_run_trajectory():
    """10 iterations across both schedule switches (exaggeration_iters = 4, check_every = 5) from the
    restatement's y0.  Yardstick: the restatement against itself with every gradient rounded to fp32."""
    rows = 300
    x, host, d, P = _grad_case(rows, 9)
    y0 = np.random.default_rng(77).normal(0.0, 1e-4, (rows, 2)).astype(np.float32)
    kw = dict(exaggeration_iters=4, check_every=5)
    y_ref, _, _, log_ref = ER.run_ref(P, y0, 10, **kw)
    y_r32, _, _, _ = ER.run_ref(P, y0, 10, round_grad=True, **kw)
    state, log = _run_device(x, host, y0, 10, **kw)
    y = state[0].cpu().numpy()
    own = np.abs(y_ref.astype(np.float64) - y_r32).max()
    dev = np.abs(y.astype(np.float64) - y_ref).max()
    print(f"trajectory: device deviation {dev:.3e}, restatement's fp32-gradient deviation {own:.3e}, ratio "
          f"{dev / own if own > 0 else float('inf'):.3f} (|y| max {np.abs(y_ref).max():.3e})")
    log = log.cpu().numpy()
    assert log.shape == (2, 2) and np.isfinite(log).all()
    for r in (0, 1):                                           # the log rows: iterations 4 and 9 (loose: y has moved)
        assert abs(log[r, 0] - log_ref[r][0]) <= 1e-3 * abs(log_ref[r][0])
        assert abs(log[r, 1] - log_ref[r][1]) <= 1e-3 * abs(log_ref[r][1])
    # one call of 10 == two calls of 5, and a rerun, bit for bit
    again, log_again = _run_device(x, host, y0, 10, **kw)
    half, log_half = _run_device(x, host, y0, 5, **kw)
    half, log_half = _run_device(x, host, y0, 5, iter0=5, state=half, log=log_half, **kw)
    for a, b, c in zip(state, again, half):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(log_again, _dev(log)) and torch.equal(log_half, _dev(log))
    assert dev <= 8.0 * own


# ------------------------------------------------------------------------------------------ end to end
def test_tsne_embed_on_the_golden():
    """tsne_embed(X), 1000 iterations, init='pca', against scikit-learn's exact t-SNE on the same data."""
    from expertsim.train.embedding import tsne_embed
    g = ER.golden()
    out = tsne_embed(_dev(g["X"]))
    y, log = out["y"].cpu().numpy(), out["kl_log"].cpu().numpy()
    kls = np.concatenate([[float(g["kl_pca"])], g["kl_random"]])
    spread = (kls.max() - kls.min()) / kls.min()
    purity = ER.knn_purity(y, g["labels"])
    floor = min(float(g["purity_pca"]), float(g["purity_random"].min()))
    print(f"golden: final KL {log[-1, 0]:.6f} vs sklearn pca-init {float(g['kl_pca']):.6f} (spread over six inits "
          f"{spread:.4f}: limit {float(g['kl_pca']) * (1 + spread):.6f}); purity {purity:.4f} vs floor {floor:.4f}")
    print("KL log:", np.array2string(log[:, 0], precision=4))
    assert log.shape == (20, 2) and np.isfinite(log).all() and np.isfinite(y).all()
    assert int(out["steps"].max()) < 100
    assert log[-1, 0] <= float(g["kl_pca"]) * (1.0 + spread)
    assert purity >= floor
    after = log[5:, 0]                                         # iterations 299, 349, .., 999: exaggeration is over
    assert (np.diff(after) <= 1e-9 * after[:-1]).all()


# ------------------------------------------------------------------------------------------ wiring
def _moe(E, extra=()):
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", "train.precision=fp32", "model.router.diff_strength=1e-6",
                                 *extra])
    torch.manual_seed(4)
    moe = setup_moe_system(cfg, torch.device(DEV))
    moe.eval()
    moe.eval_batch_size = 128
    return moe, cfg


def _batch(n):
    from expertsim.utils.synthetic import make_batch
    return make_batch(n, "neutron", seed=11)


def test_diagnose_with_embedding():
    from expertsim.train.diagnostics import DIAGNOSTIC_KEYS
    from expertsim.train.embedding import EMBEDDING_KEYS, pca_project
    N, E, seed = 600, 3, 13
    moe, _ = _moe(E)
    cond_host = _batch(N)["cond"].astype(np.float32)
    cond = _dev(cond_host)
    C = cond_host.shape[1]
    plain = moe.diagnose(cond, seed=seed, names=[f"v{i}" for i in range(C)])
    assert set(plain) == set(DIAGNOSTIC_KEYS) | {"cond_names"}
    assert set(moe.diagnose(cond, seed=seed)) == set(DIAGNOSTIC_KEYS)
    diag = moe.diagnose(cond, seed=seed, embedding=True, embedding_iters=60)
    assert set(diag) == set(DIAGNOSTIC_KEYS) | set(EMBEDDING_KEYS)
    shapes = {"embed_rows": (N,), "embed_expert": (N,), "pca": (N, 2), "pca_components": (2, C),
              "pca_explained_variance": (2,), "pca_explained_variance_ratio": (2,), "tsne": (N, 2), "tsne_kl": (2,)}
    assert {k: diag[k].shape for k in shapes} == shapes
    assert all(np.array_equal(diag[k], plain[k], equal_nan=True) for k in DIAGNOSTIC_KEYS)
    expert = moe.simulate(cond, seed=seed, domain="photons")["expert"].cpu().numpy()
    assert np.array_equal(diag["embed_rows"], np.arange(N)) and np.array_equal(diag["embed_expert"], expert)
    pca = pca_project(cond, 2)
    assert np.array_equal(diag["pca"], pca["scores"].cpu().numpy())
    assert np.array_equal(diag["pca_components"], pca["components"].cpu().numpy())
    assert np.isfinite(diag["tsne"]).all() and np.isfinite(diag["tsne_kl"]).all() and diag["tsne"].std() > 0


def test_evaluate_epoch_with_eval_embedding(tmp_path):
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.embedding import EMBEDDING_KEYS
    from expertsim.train.loop import evaluate_epoch
    N = 257
    b = _batch(N)
    x = torch.from_numpy(b["real_images"])
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    moe, cfg = _moe(3, extra=("train.eval_on_device=true", "train.eval_diagnostics=true", "train.eval_embedding=true",
                              "train.eval_embedding_iters=20", "train.eval_embedding_max=100",
                              "train.save_experiment_data=true"))
    cfg.train.dir_info = str(tmp_path / "info")
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=200), epoch=2, cfg=cfg, device=torch.device(DEV))
    diag = out["expert_diagnostics"]
    z = np.load(tmp_path / "info" / "diagnostics_epoch_2.npz")
    assert set(EMBEDDING_KEYS) <= set(diag) and set(z.files) == set(diag)
    assert np.array_equal(diag["embed_rows"], np.arange(0, N, 3)) and diag["tsne"].shape == (86, 2)
    assert all(np.array_equal(z[k], diag[k], equal_nan=True) for k in diag)


def test_cond_embedding_stride_subsample():
    from expertsim.train.embedding import cond_embedding, pca_project
    max_rows = 150
    N = 2 * max_rows + 1
    cond = _clusters(N, 9, 9)
    expert = (np.arange(N) % 3).astype(np.int32)
    out = cond_embedding(_dev(cond), _dev(expert), 3, max_rows=max_rows, n_iter=20)
    keep = np.arange(0, N, 3)
    assert np.array_equal(out["embed_rows"], keep) and np.array_equal(out["embed_expert"], expert[keep])
    assert out["pca"].shape == (len(keep), 2) and out["tsne"].shape == (len(keep), 2) and out["tsne_kl"].shape == (1,)
    assert np.array_equal(out["pca"], pca_project(_dev(cond[keep]), 2)["scores"].cpu().numpy())
    assert np.isfinite(out["tsne"]).all()
