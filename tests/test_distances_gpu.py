"""es_segment_moments / es_frechet / es_mmd_poly on the device against numpy (np.mean / np.cov), the record of
scipy and scikit-learn (tests/golden/distances_scipy.npz) and the numpy restatement (tests/distance_refs.py), and
expertsim.train.distances / MoEWrapper.evaluate_device(distances=True) / loop.evaluate_epoch(train.eval_distances)
/ ``cli.py --simulate --real --distances`` end to end.

Bounds (derived in tests/distance_refs.py, u = 2^-53): a mean within (n + 1) u sum|x| / n, a covariance entry within
(n + 4) 2 u sum|d_i||d_j| / (n - 1), a kernel sum of T terms within (T - 1 + cols + degree + 2) u sum|k|, and the
Frechet numbers within 8 max(D, 1) U of the symmetric eigh form on identical moments, U = 2^-52 cols (tr A + tr B +
|dmu|^2) and D the record's own disagreement between scipy's sqrtm form and the eigh form.  Every test prints the
worst observed error-to-bound ratio before it asserts."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distance_refs as R
import segment_refs as S
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


# ------------------------------------------------------------------------------------------ 1. moments
MOM_ROWS = 1100
# lengths 0, 1, 2, 63, 64, 65, 257, 1000, then an empty entry, one clamped at the end (1000 .. 1100), one clamped at
# the start (0 .. 3) and one with e < b (empty)
MOM_SEG = np.array([[0, 0], [5, 6], [10, 12], [20, 83], [100, 164], [200, 265], [300, 557], [50, 1050], [700, 700],
                    [1000, 5000], [-5, 3], [900, 800]], dtype=np.int32)


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("cols", [1, 3, 10, 32])
def test_moments_against_numpy(cols, f64):
    from expertsim.train.distances import segment_moments
    rs = np.random.RandomState(100 + cols)
    full = (rs.randn(MOM_ROWS, cols + 3) * (1.0 + 5.0 * rs.rand(cols + 3)) + 3.0 * rs.randn(cols + 3))
    full = full.astype(np.float64 if f64 else np.float32)
    xd = _dev(full)[:, :cols]                                               # ld = cols + 3 > cols
    assert xd.stride(0) == cols + 3
    x = full[:, :cols].astype(np.float64)
    n_seg, worst_m, worst_c = len(MOM_SEG), 0.0, 0.0
    for idx in (None, rs.permutation(MOM_ROWS).astype(np.int32)):
        count = torch.full((n_seg + 2,), -7, dtype=torch.int32, device=DEV)
        mean = torch.full((n_seg + 2, cols), -7.0, dtype=torch.float64, device=DEV)
        cov = torch.full((n_seg + 2, cols, cols), -7.0, dtype=torch.float64, device=DEV)
        segment_moments(xd, None if idx is None else _dev(idx), _dev(MOM_SEG), out=(count, mean, cov))
        count, mean, cov = count.cpu().numpy(), mean.cpu().numpy(), cov.cpu().numpy()
        assert (count[n_seg:] == -7).all() and (mean[n_seg:] == -7).all() and (cov[n_seg:] == -7).all()
        members = S.members(MOM_ROWS, idx, MOM_SEG)
        assert [len(m) for m in members] == [0, 1, 2, 63, 64, 65, 257, 1000, 0, 100, 3, 0]
        for s, m in enumerate(members):
            n, ref_mean, ref_cov = R.moments(x[m])
            assert count[s] == n, s
            assert np.array_equal(cov[s].view(np.int64), cov[s].T.copy().view(np.int64)), s     # symmetric bitwise
            if n == 0:
                assert np.isnan(mean[s]).all() and np.isnan(cov[s]).all(), s
                continue
            if n == 1:
                assert np.array_equal(mean[s], x[m][0]) and np.isnan(cov[s]).all(), s
                continue
            mb, cb = R.moment_bounds(x[m])
            em, ec = np.abs(mean[s] - ref_mean), np.abs(cov[s] - ref_cov)
            worst_m = max(worst_m, float((em / np.where(mb > 0, mb, 1.0)).max()))
            worst_c = max(worst_c, float((ec / np.where(cb > 0, cb, 1.0)).max()))
            assert (em <= mb).all() and (ec <= cb).all(), (s, n, (em / mb).max(), (ec / cb).max())
    print(f"moments cols={cols} f64={f64}: worst error / bound: mean {worst_m:.3g}, cov {worst_c:.3g}")


def test_moments_rerun_is_bit_equal():
    from expertsim.train.distances import segment_moments
    rs = np.random.RandomState(7)
    x = _dev(rs.randn(MOM_ROWS, 10))
    idx, seg = _dev(rs.permutation(MOM_ROWS).astype(np.int32)), _dev(MOM_SEG)
    first, again = segment_moments(x, idx, seg), segment_moments(x, idx, seg)
    torch.cuda.synchronize()
    assert all(torch.equal(_bytes(a), _bytes(b)) for a, b in zip(first, again))


# ------------------------------------------------------------------------------------------ 2. Frechet
@pytest.mark.parametrize("cols", [1, 2, 10, 32])
def test_frechet_against_the_record(golden, cols):
    """Problems: gauss, a NaN problem, obs, then A = B with dmu = 0 for both kinds."""
    from expertsim.train.distances import frechet
    g = {kind: [golden[f"fr_{kind}_{cols}_{n}"] for n in ("mean_a", "cov_a", "mean_b", "cov_b")]
         for kind in ("gauss", "obs")}
    nan = [a.copy() for a in g["gauss"]]
    nan[3][cols - 1, 0] = nan[3][0, cols - 1] = np.nan
    probs = [g["gauss"], nan, g["obs"], [g["gauss"][0], g["gauss"][1]] * 2, [g["obs"][0], g["obs"][1]] * 2]
    out = torch.full((len(probs) + 1, 4), -7.0, dtype=torch.float64, device=DEV)
    frechet(*[_dev(np.stack([p[i] for p in probs])) for i in range(4)], out=out)
    out = out.cpu().numpy()
    assert (out[len(probs)] == -7).all()
    assert np.isnan(out[1]).all()
    worst = 0.0
    for row, kind in ((0, "gauss"), (2, "obs")):
        unit = R.frechet_unit(*g[kind])
        D = float(golden[f"fr_{kind}_{cols}_D"])
        err = np.abs(out[row] - golden[f"fr_{kind}_{cols}_eigh"]) / unit
        worst = max(worst, float(err.max()))
        print(f"frechet {kind} cols={cols}: |device - eigh| / U = {err}  (D = {D:.3g} U, limit {8 * max(D, 1.0):.3g} U)")
        assert (err <= 8 * max(D, 1.0)).all(), (kind, err, D)
    for row, kind in ((3, "gauss"), (4, "obs")):
        unit = R.frechet_unit(g[kind][0], g[kind][1], g[kind][0], g[kind][1])
        print(f"frechet {kind} cols={cols} A = B: d2 / U = {out[row, 0] / unit:.3g}")
        assert abs(out[row, 0]) <= 8 * unit and out[row, 1] == 0.0
        worst = max(worst, abs(out[row, 0]) / unit)
    print(f"frechet cols={cols}: worst ratio to U {worst:.3g}")


# ------------------------------------------------------------------------------------------ 3. kernel sums
MMD_ROWS = 600
# (real b, e), (generated b, e): m, n from 1, 2, 63, 64, 65, 257, unequal; an empty real segment; then ten equal
# blocks of 25 and the whole 257
MMD_SEG = [((0, 1), (0, 2)), ((3, 5), (7, 8)), ((10, 73), (20, 84)), ((100, 164), (100, 165)),
           ((200, 265), (300, 557)), ((300, 557), (10, 73)), ((50, 50), (0, 5))]
MMD_SEG += [((300 + 25 * t, 325 + 25 * t), (300 + 25 * t, 325 + 25 * t)) for t in range(10)] + [((300, 557), (300, 557))]


@pytest.mark.parametrize("cols", [1, 3, 10, 16, 64])
def test_mmd_poly_against_the_restatement(cols):
    from expertsim.train.distances import mmd_poly_sums
    rs = np.random.RandomState(200 + cols)
    real_full = np.concatenate([R.observable_rows(rs, MMD_ROWS, cols), rs.rand(MMD_ROWS, 2)], 1).astype(np.float32)
    fake_full = np.concatenate([0.95 * R.observable_rows(rs, MMD_ROWS, cols) + 0.03, rs.rand(MMD_ROWS, 2)],
                               1).astype(np.float32)
    rd, fd = _dev(real_full)[:, :cols], _dev(fake_full)[:, :cols]           # ld = cols + 2 > cols
    real, fake = real_full[:, :cols], fake_full[:, :cols]
    r_idx, f_idx = rs.permutation(MMD_ROWS).astype(np.int32), rs.permutation(MMD_ROWS).astype(np.int32)
    r_seg = np.array([a for a, _ in MMD_SEG], dtype=np.int32)
    f_seg = np.array([b for _, b in MMD_SEG], dtype=np.int32)
    m_r, m_f = S.members(MMD_ROWS, r_idx, r_seg), S.members(MMD_ROWS, f_idx, f_seg)
    n_seg = len(MMD_SEG)
    for degree in (1, 2, 4):
        def run():
            out = (torch.full((n_seg + 1, 4), -7.0, dtype=torch.float64, device=DEV),
                   torch.full((n_seg + 1, 2), -7, dtype=torch.int32, device=DEV))
            return mmd_poly_sums(rd, fd, degree=degree, r_idx=_dev(r_idx), r_seg=_dev(r_seg), f_idx=_dev(f_idx),
                                 f_seg=_dev(f_seg), out=out)
        (sums_d, counts_d), (sums_2, counts_2) = run(), run()
        torch.cuda.synchronize()
        assert torch.equal(_bytes(sums_d), _bytes(sums_2)) and torch.equal(counts_d, counts_2)   # rerun: bit-equal
        sums, counts = sums_d.cpu().numpy(), counts_d.cpu().numpy()
        assert (sums[n_seg] == -7).all() and (counts[n_seg] == -7).all() and (sums[:n_seg, 3] == 0).all()
        worst = 0.0
        for s, (ir, jf) in enumerate(zip(m_r, m_f)):
            m, n = len(ir), len(jf)
            assert counts[s].tolist() == [m, n], s
            ref, absum = R.poly_sums(real[ir], fake[jf], degree)
            bound = R.poly_bound(m, n, cols, degree, absum)
            err = np.abs(sums[s, :3] - ref)
            worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
            assert (err <= bound).all(), (s, m, n, degree, err, bound)
            if m == 1:
                assert sums[s, 0] == 0.0                                     # one row: no pair, exactly
            if m == 0:
                assert sums[s, 0] == 0.0 and sums[s, 2] == 0.0
        print(f"mmd_poly cols={cols} degree={degree}: worst error / bound {worst:.3g}")


def test_mmd_poly_against_sklearn_and_the_diagonal(golden):
    from expertsim.train.distances import mmd_poly_sums
    worst = 0.0
    for i, (cols, m, n, degree) in enumerate(R.MMD_CASES):
        x, y = golden[f"mmd_{i}_x"], golden[f"mmd_{i}_y"]
        sums, counts = mmd_poly_sums(_dev(x), _dev(y), degree=degree)
        assert counts.cpu().numpy().tolist() == [[m, n]]
        _, absum = R.poly_sums(x, y, degree)
        bound = R.poly_bound(m, n, cols, degree, absum)
        err = np.abs(sums.cpu().numpy()[0, :3] - golden[f"mmd_{i}_sums"])
        worst = max(worst, float((err / np.where(bound > 0, bound, 1.0)).max()))
        assert (err <= bound).all(), (i, err, bound)
    print(f"mmd_poly against scikit-learn: worst error / bound {worst:.3g}")
    # two identical rows: S_xx = 2 k(x, x), nothing of the diagonal
    x = golden["mmd_2_x"][:1]
    two = np.repeat(x, 2, axis=0)
    sums, _ = mmd_poly_sums(_dev(two), _dev(x), degree=4, gamma=0.25, coef0=0.5)
    ref, absum = R.poly_sums(two, x, 4, 0.25, 0.5)
    k = (0.25 * float(np.dot(x[0].astype(np.float64), x[0].astype(np.float64))) + 0.5) ** 4
    bound = R.poly_bound(2, 1, x.shape[1], 4, absum)
    got = sums.cpu().numpy()[0]
    assert abs(got[0] - 2 * k) <= bound[0] + 8 * R.U * 2 * k and got[1] == 0.0 and abs(got[2] - ref[2]) <= bound[2]


# ------------------------------------------------------------------------------------------ 4. fpd / kpd
def test_fpd_kpd_over_experts(golden):
    """Three experts, one empty and one of 7 <= cols rows: those and only those segments are NaN.  Tolerances: the
    Frechet numbers move by the moments' rounding ((n + 4) 2 u relative to sum|d_i||d_j|, about 1e-13 here) times
    the condition of the matrix square root (below 1e3 by the record) and the extrapolation's leverage (the
    intercept is a combination of the FD_j with coefficients below 20): 1e-8 of fd_full covers it a hundredfold.
    Each block's MMD^2 is within the sum of its three kernel sums' bounds over their term counts, and a median or
    percentile moves by no more than the largest of them."""
    from expertsim.train.distances import distances, fpd, kpd
    real, fake, expert = golden["ex_real"], golden["ex_fake"], golden["ex_expert"]
    rd, fd, ed = _dev(real), _dev(fake), _dev(expert)
    f = fpd(rd, fd, ed, R.EXPERT_E, details=True)
    k = kpd(rd, fd, ed, R.EXPERT_E, details=True)
    both = distances(rd, fd, ed, R.EXPERT_E)
    assert all(both[key] == v or (np.isnan(both[key]) and np.isnan(v))
               for key, v in {**f, **k}.items() if isinstance(v, float))
    assert tuple(f["table"].shape) == (4, 10, 3) and tuple(k["table"].shape) == (4, 11, 5)
    names = ["", "_0", "_1", "_2"]
    for s, suffix in enumerate(names):
        fv = np.array([f[f"{n}{suffix}"] for n in ("fpd", "fpd_err", "fd_full")])
        kv = np.array([k[f"{n}{suffix}"] for n in ("kpd", "kpd_err", "mmd_full")])
        assert np.isnan(fv).all() == bool(golden["ex_fpd_nan"][s]) and np.isnan(fv).any() == np.isnan(fv).all()
        assert np.isnan(kv).all() == bool(golden["ex_kpd_nan"][s]) and np.isnan(kv).any() == np.isnan(kv).all()
        if golden["ex_fpd_nan"][s]:
            continue
        want_f, want_k = golden[f"ex_s{s}_fpd"], golden[f"ex_s{s}_kpd"]
        print(f"segment {s}: fpd {fv} vs {want_f}; kpd {kv} vs {want_k}")
        assert (np.abs(fv - want_f) <= 1e-8 * want_f[2]).all(), (s, fv, want_f)
        kt = golden[f"ex_s{s}_kpd_table"]
        tol = 0.0
        ix = np.arange(len(real)) if s == 0 else np.where(expert == s - 1)[0]
        m = len(ix) // 10
        for t in range(11):
            lo, hi = (t * m, (t + 1) * m) if t < 10 else (0, len(ix))
            _, absum = R.poly_sums(real[ix][lo:hi].astype(np.float32), fake[ix][lo:hi].astype(np.float32), 4)
            b = R.poly_bound(hi - lo, hi - lo, R.EXPERT_COLS, 4, absum) / R.poly_terms(hi - lo, hi - lo)
            tol = max(tol, 2 * float(b[0] + b[1] + 2 * b[2]))              # the record's sums carry a bound as well
        assert kt.shape == (11, 5) and (np.abs(kv - want_k) <= tol).all(), (s, kv, want_k, tol)


def test_shift_grows_both_distances(golden):
    from expertsim.train.distances import fpd, kpd
    real = golden["ex_real"]
    fd_full, mmd_full = [], []
    for shift in (0.05, 0.1, 0.2):
        fake = real.copy()
        fake[:, 3] += shift
        fd_full.append(fpd(_dev(real), _dev(fake))["fd_full"])
        mmd_full.append(kpd(_dev(real), _dev(fake))["mmd_full"])
    print("fd_full", fd_full, "mmd_full", mmd_full)
    assert fd_full[0] < fd_full[1] < fd_full[2] and mmd_full[0] < mmd_full[1] < mmd_full[2]
    assert all(v > 0 for v in fd_full + mmd_full)


# ------------------------------------------------------------------------------------------ 5. wiring
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


def _dist_keys(E):
    from expertsim.train.distances import KEYS
    return {f"dist_{n}" for n in KEYS} | {f"dist_{n}_{e}" for n in KEYS for e in range(E)}


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_evaluate_device_distances():
    from expertsim.train import distances as D
    from expertsim.train.distances import KEYS
    E, N, seed = 3, 96, 17
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, distances=True)
    extra = {"dist_obs_real", "dist_obs_gen", "dist_scale", "dist_fpd_table", "dist_fpd_frechet", "dist_kpd_table"}
    assert set(det) == set(plain) | _dist_keys(E) | extra
    for key, v in plain.items():                                                   # bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(_bytes(det[key]), _bytes(v)), key
        else:
            assert det[key] == v, key
    assert all(np.isfinite(det[f"dist_{n}"]) for n in KEYS), {n: det[f"dist_{n}"] for n in KEYS}
    assert det["dist_fd_full"] > 0 and det["dist_obs_real"].shape == (N, 10) and det["dist_obs_real"].dtype == torch.float64
    assert float(det["dist_obs_real"].abs().max()) == 1.0
    again = moe.evaluate_device(5, cond, x, cfg, seed=seed, distances=True)
    assert set(again) == {k for k, v in plain.items() if not isinstance(v, torch.Tensor)} | _dist_keys(E)
    assert all(_same_float(again[k], det[k]) for k in again)
    # the same numbers from the public pieces, and with the features of the simulate call reused
    want = D.distances(det["dist_obs_real"], det["dist_obs_gen"], det["expert"], E)
    assert all(_same_float(det[f"dist_{k}"], v) for k, v in want.items())
    feats = moe.evaluate_device(5, cond, x, cfg, seed=seed, features=True, distances=True)
    assert all(_same_float(feats[k], det[k]) for k in _dist_keys(E))


def test_evaluate_epoch_averages_over_the_finite_batches():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    E, N, bs = 3, 106, 48                            # batches of 48, 48 and 10 rows: the last is too short for both
    moe, cfg = _moe(E, extra=("train.eval_on_device=true", "train.eval_distances=true"))
    b, x, cond = _batch(N)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg, device=torch.device(DEV))
    cfg_off = _cfg(E, extra=("train.eval_on_device=true",))
    off = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_off, device=torch.device(DEV))
    assert set(out) == set(off) | _dist_keys(E) and all(out[key] == off[key] for key in off)
    per = [moe.evaluate_device(0, cond[i:i + bs], x[i:i + bs], cfg, seed=int(cfg.train.rng_seed), sample_offset=i,
                               distances=True) for i in range(0, N, bs)]
    assert all(np.isnan(per[2][key]) for key in _dist_keys(E))                      # 10 rows: n_0 = 5, m = 1
    assert all(np.isfinite(per[i]["dist_fpd"]) and np.isfinite(per[i]["dist_kpd"]) for i in (0, 1))
    for key in _dist_keys(E):
        finite = [m[key] for m in per if np.isfinite(m[key])]
        if finite:
            assert out[key] == sum(finite) / len(finite), key
        else:
            assert np.isnan(out[key]), key
    cfg_bad = _cfg(E, extra=("train.eval_distances=true",))
    with pytest.raises(ValueError, match="eval_on_device"):
        evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_bad, device=torch.device(DEV))


def test_cli_simulate_real_distances(tmp_path):
    from expertsim.train import distances as D
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    E, N, k = 3, 64, 3
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
                        "--sim-batch-size", "16", "--real", str(tmp_path / "real.npy"), "--prdc-k", str(k),
                        "--distances", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert _dist_keys(E) <= set(z.files) and "prdc_precision" in z.files
    images, expert = torch.from_numpy(z["images"]).to(DEV), torch.from_numpy(z["expert"]).to(DEV)
    obs_real = D.observables(x.to(DEV), log_domain=True)
    obs_gen = D.observables(images, log_domain=False, sums=torch.from_numpy(z["sums"]).to(DEV))
    obs_real, obs_gen, _ = D.normalise(obs_real, obs_gen)
    want = D.distances(obs_real, obs_gen, expert, E)
    for key in _dist_keys(E):
        assert z[key].dtype == np.float64 and _same_float(float(z[key]), want[key[5:]]), key
        assert f"{key} = " in r.stdout
    assert np.isfinite(float(z["dist_fpd"])) and np.isfinite(float(z["dist_kpd"]))
