"""Sliced Wasserstein distance of whole images on the device (csrc/sliced.hip, expertsim/train/sliced.py; DESIGN.md
§7k) against the numpy / scipy restatement of tests/sliced_refs.py and the committed record
tests/golden/sliced_numpy.npz.

Every bound is derived in sliced_refs (u = 2^-53): a projection within (D + 1) u sum |x| |theta|, a direction within
(D / 2 + 3) u |ref|, a distance on the device's own projections within 2 m 2^-52 ref, a distance end to end within
that plus the largest projection bound of either side.  Every test prints its worst observed error-to-bound ratio
before it asserts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sliced_refs as R
from conftest import REPO

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).to(DEV)                        # a copy: the seeded inputs are read-only
    return t if dtype is None else t.to(dtype)


def _ratio(err, bound):
    return float((err / np.where(bound > 0, bound, 1.0)).max())


def _raw_project(view_dims, strides, x, theta, theta_ld, n_proj, out, out_ld, dt=0):
    from expertsim import hip
    view = hip.make_view(view_dims, strides)
    return hip.call("es_sliced_project", C.byref(view), dt, hip.ptr(x), hip.ptr(theta), theta_ld, n_proj, hip.ptr(out),
                    out_ld, hip.stream_ptr())


# ------------------------------------------------------------------------------------------ 1. layout
def test_exact_integer_layout():
    """Integer images against an ASYMMETRIC integer theta: every product and sum is exact, so the output is the int64
    product -- a row / column swap or the f32 row map of the C/D fragment cannot pass."""
    from expertsim.train.sliced import project
    N, P, h, w = 33, 19, 3, 7
    D = h * w
    b, p, d = np.arange(N)[:, None], np.arange(P)[:, None], np.arange(D)[None, :]
    x = ((5 * b + 2 * d) % 13 - 6).astype(np.int64)
    theta = ((3 * p + 7 * d) % 11 - 5).astype(np.int64)
    want = x @ theta.T
    assert not np.array_equal(want[:19, :19], want[:19, :19].T)
    got = project(_dev(x.reshape(N, h, w).astype(np.float32)), _dev(theta.astype(np.float64))).cpu().numpy()
    assert got.shape == (N, P) and got.dtype == np.float64
    assert np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)[:8]


# ------------------------------------------------------------------------------------------ 2. projection
# every N of {1, 15, 16, 17, 65, 257}, every shape and every P of {1, 15, 16, 17, 64, 80} at least once
PROJECT_CASES = [
    (1, (1, 1), 1, "f32", "plain"),
    (15, (1, 3), 15, "f32", "plain"),
    (16, (2, 2), 16, "bf16", "plain"),
    (17, (1, 5), 17, "f32", "strided"),
    (65, (6, 5), 64, "f32", "ld"),
    (257, (56, 30), 80, "f32", "plain"),
    (17, (44, 44), 17, "bf16", "strided"),
    (65, (64, 64), 15, "f32", "plain"),
    (257, (44, 44), 80, "f32", "plain"),
    (16, (56, 30), 1, "f32", "ld"),
    (33, (6, 5), 16, "bf16", "ld"),
    (15, (64, 64), 64, "f32", "strided"),
]


@pytest.mark.parametrize("N,shape,P,dtype,mode", PROJECT_CASES)
def test_projection_against_the_restatement(N, shape, P, dtype, mode):
    from expertsim.train.sliced import project
    h, w = shape
    D = h * w
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    x = _dev(R.images(h, w, N)).to(tdt)
    theta_host = R.normal_theta(P, D)
    ref, absum = R.project_ref(x.float().cpu().numpy(), theta_host)
    bound = R.project_bound(D, absum)
    theta = _dev(theta_host)
    if mode == "strided":            # a batch slice with a step, inside a wider tensor full of NaN
        big = torch.full((2 * N + 1, 1, h + 2, w + 3), float("nan"), dtype=tdt, device=DEV)
        xv = big[1::2, :, 1:h + 1, 2:w + 2]
        xv.copy_(x[:, None])
        assert not xv.is_contiguous()
        got = project(xv, theta)
    elif mode == "ld":               # out_ld > P and theta_ld > D; the sentinel columns and rows stay
        tbuf = torch.full((P, D + 3), float("nan"), dtype=torch.float64, device=DEV)
        tbuf[:, :D] = theta
        obuf = torch.full((N + 2, P + 5), -7.5, dtype=torch.float64, device=DEV)
        got = project(x, tbuf[:, :D], out=obuf)
        assert got.data_ptr() == obuf.data_ptr() and tuple(got.shape) == (N, P)
        assert bool((obuf[N:] == -7.5).all()) and bool((obuf[:, P:] == -7.5).all())
    else:
        got = project(x, theta)
    got = got.cpu().numpy()
    err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
    print(f"project N={N} {shape} P={P} {dtype} {mode}: worst error / bound {_ratio(err, bound):.3g}")
    assert np.isfinite(got).all() and (err <= bound).all()


# ------------------------------------------------------------------------------------------ 3. independence
def test_projection_is_independent_of_batch_and_direction_position():
    from expertsim.train.sliced import project
    h, w, N, P = 44, 44, 257, 80
    x, theta = _dev(R.images(h, w, N)), _dev(R.normal_theta(P, h * w))
    full = project(x, theta)
    assert torch.equal(_bytes(project(x, theta)), _bytes(full))                    # a rerun
    assert torch.equal(_bytes(project(x[3:20], theta)), _bytes(full[3:20]))        # rows 3 .. 20 alone
    assert torch.equal(_bytes(project(x, theta[:17])), _bytes(full[:, :17]))       # the first 17 directions alone
    assert torch.equal(_bytes(project(x[200:], theta[64:])), _bytes(full[200:, 64:]))


# ------------------------------------------------------------------------------------------ 4. directions
@pytest.mark.parametrize("d", [1, 5, 30, 1936])
def test_directions(d):
    from expertsim import hip
    from expertsim.train import sliced as S
    P, seed = 19, 77
    D2 = d + d % 2
    theta = S.directions(P, d, seed=seed)
    assert tuple(theta.shape) == (P, d) and theta.dtype == torch.float64
    draws = torch.empty(P * D2, dtype=torch.float32, device=DEV)
    hip.call("es_randn", hip.ptr(draws), P * D2, seed, S.SLICED_STREAM, hip.stream_ptr())
    ref = R.directions_ref(draws.reshape(P, D2).cpu().numpy(), d)
    got = theta.cpu().numpy()
    err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
    bound = R.direction_bound(d, ref)
    norm = np.abs(np.sqrt((got.astype(np.longdouble) ** 2).sum(axis=1)) - 1).astype(np.float64)
    print(f"directions d={d}: worst error / bound {_ratio(err, bound):.3g}, worst |norm - 1| / ((D + 4) u) "
          f"{norm.max() / ((d + 4) * R.U):.3g}")
    assert (err <= bound).all()
    assert (norm <= (d + 4) * R.U).all()
    assert torch.equal(_bytes(S.directions(P, d, seed=seed)), _bytes(theta))       # equal seed, equal bits
    other_seed = S.directions(P, d, seed=seed + 1)
    other_stream = torch.empty_like(theta)
    hip.call("es_sliced_directions", hip.ptr(other_stream), d, P, d, seed, S.SLICED_STREAM + 1, hip.stream_ptr())
    if d > 1:                                                                      # d = 1: every row is +-1
        assert all(not torch.equal(o[p], theta[p]) for o in (other_seed, other_stream) for p in range(P))
    else:
        assert bool((theta.abs() == 1.0).all())
    if d == 30:                                                                    # theta_ld > d: the rest stays
        buf = torch.full((P, d + 2), -7.5, dtype=torch.float64, device=DEV)
        hip.call("es_sliced_directions", hip.ptr(buf), d + 2, P, d, seed, S.SLICED_STREAM, hip.stream_ptr())
        assert torch.equal(_bytes(buf[:, :d]), _bytes(theta)) and bool((buf[:, d:] == -7.5).all())


# ------------------------------------------------------------------------------------------ 5. arguments
def test_arguments():
    from expertsim import hip
    from expertsim.train import sliced as S
    x = torch.ones(4, 1, 64, 65, dtype=torch.float32, device=DEV)
    theta = torch.ones(1025, 4160, dtype=torch.float64, device=DEV)
    out = torch.full((4, 1030), -7.5, dtype=torch.float64, device=DEV)
    s = (64 * 65, 64 * 65, 65, 1)
    ok = dict(view_dims=(4, 1, 6, 5), strides=s, x=x, theta=theta, theta_ld=4160, n_proj=16, out=out, out_ld=1030)
    bad = [dict(view_dims=(4, 1, 1, 4097)),                 # D = 4097
           dict(view_dims=(4, 1, 64, 65)),                  # D = 4160
           dict(n_proj=1025), dict(n_proj=0),
           dict(view_dims=(4, 2, 6, 5)),                    # c = 2
           dict(out_ld=15), dict(theta_ld=29),
           dict(x=None), dict(theta=None), dict(out=None),
           dict(view_dims=((1 << 20) + 1, 1, 6, 5))]
    for change in bad:
        with pytest.raises(hip.HipError, match=r"es_sliced_project failed \(1\)"):
            _raw_project(**{**ok, **change})
    assert _raw_project(**{**ok, "view_dims": (0, 1, 6, 5)}) == 0                   # n = 0: fine, no launch
    assert bool((out == -7.5).all())
    assert _raw_project(**ok) == 0
    assert bool((out[:, :16] == 30.0).all()) and bool((out[:, 16:] == -7.5).all())
    for args in [(None, 30, 4, 30), (theta, 29, 4, 30), (theta, 4160, 1025, 30), (theta, 4160, 4, 4097),
                 (theta, 4160, 0, 30), (theta, 4160, 4, 0)]:
        with pytest.raises(hip.HipError, match=r"es_sliced_directions failed \(1\)"):
            hip.call("es_sliced_directions", hip.ptr(args[0]), args[1], args[2], args[3], 0, S.SLICED_STREAM,
                     hip.stream_ptr())
    assert bool((theta == 1.0).all())
    img = torch.zeros(8, 6, 5, device=DEV)
    assert tuple(S.project(img[:0], theta[:3, :30]).shape) == (0, 3)
    before = out.clone()
    with pytest.raises(ValueError, match="65535"):                                # before any launch
        S.sliced(img, img, torch.zeros(8, dtype=torch.int32, device=DEV), n_experts=63, n_proj=1024)
    assert torch.equal(out, before)


# ------------------------------------------------------------------------------------------ 6. distances
@pytest.mark.parametrize("shape", [(6, 5), (44, 44)])
def test_distances_on_the_device_projections_against_scipy(shape):
    from expertsim.train.sliced import sliced_device
    from expertsim.train.utils import wasserstein_1d_device
    h, w = shape
    real, fake = R.images(h, w, 300, seed=1), R.images(h, w, 257, seed=2, shift=0.25)
    raw = sliced_device(_dev(real), _dev(fake), directions=_dev(R.normal_theta(64, h * w)))
    pr, pf = raw["proj_real"].cpu().numpy(), raw["proj_fake"].cpu().numpy()
    ref = R.w_table(pr, pf, [np.arange(300)], [np.arange(257)])
    bound = R.ws_bound(557, ref)
    got = raw["w"].cpu().numpy()
    assert got.shape == (1, 64) and (ref > 0).all()
    err = np.abs(got - ref)
    rng = np.random.default_rng(9)
    perm_r, perm_f = (_dev(rng.permutation(n).astype(np.int32)) for n in (300, 257))
    permuted = wasserstein_1d_device(raw["proj_real"], raw["proj_fake"], u_idx=perm_r, v_idx=perm_f).cpu().numpy()
    err_p = np.abs(permuted - ref)
    print(f"distances {shape}: worst error / bound {_ratio(err, bound):.3g}, permuted {_ratio(err_p, bound):.3g}")
    assert (err <= bound).all() and (err_p <= bound).all()
    assert raw["counts"].cpu().tolist() == [[300, 257]]
    assert float(raw["maxima"][0]) == got.max()


# ------------------------------------------------------------------------------------------ 7. end to end
@pytest.mark.parametrize("shape", R.RECORD_SHAPES)
def test_end_to_end_against_the_record(shape):
    from expertsim.train.sliced import sliced
    h, w = shape
    g, key = R.golden(), f"c{shape[0]}x{shape[1]}"
    real, fake, expert = R.record_inputs(h, w)
    theta = g[f"{key}_theta16"].astype(np.float64)
    out = sliced(_dev(real), _dev(fake), _dev(expert), R.RECORD_E, directions=_dev(theta), details=True)
    _, _, _, counts, proj_bound = R.record_case(h, w)
    ref = g[f"{key}_w"]
    assert np.array_equal(g[f"{key}_counts"], counts) and out["counts"].cpu().tolist() == counts.tolist()
    entry = R.ws_bound(counts.sum(axis=1)[:, None], ref) + proj_bound[None, :]
    got = out["w"].cpu().numpy()
    err = np.abs(got - ref)
    print(f"record {shape}: table worst error / bound {_ratio(err, entry):.3g}")
    assert got.shape == (R.RECORD_E + 1, R.RECORD_P) and (err <= entry).all()
    assert (got[2] == 0).all()                                                     # the kernel's value for the empty expert
    want, sb = g[f"{key}_summary"], R.summary_bounds(ref, entry)
    worst = 0.0
    for i, name in enumerate(("swd", "swd_err", "swd_max")):
        for s, suffix in enumerate(("", "_0", "_1", "_2")):
            v = out[name + suffix]
            if s == 2:
                assert np.isnan(v) and np.isnan(want[i, s]), (name, suffix, v)     # the empty expert
                continue
            worst = max(worst, abs(v - want[i, s]) / sb[i, s])
            assert abs(v - want[i, s]) <= sb[i, s], (name, suffix, v, want[i, s], sb[i, s])
    print(f"record {shape}: summary worst error / bound {worst:.3g}")
    assert out["swd_2"] > 0 and np.isfinite(out["swd_err_2"])                      # the one-row expert


# ------------------------------------------------------------------------------------------ 8. properties
@pytest.mark.parametrize("shape", [(6, 5), (44, 44)])
def test_properties(shape):
    from expertsim.train.sliced import sliced
    h, w = shape
    N = 257
    real = _dev(R.images(h, w, N, seed=1))
    theta = _dev(R.normal_theta(64, h * w))
    same = sliced(real, real, directions=theta, details=True)
    assert bool((same["w"] == 0.0).all()) and same["swd"] == 0.0 and same["swd_max"] == 0.0 and same["swd_err"] == 0.0
    shuffled = real[_dev(np.random.default_rng(2).permutation(N))]
    perm = sliced(real, shuffled, directions=theta, details=True)
    assert bool((perm["w"] == 0.0).all()) and perm["swd"] == 0.0
    plain = sliced(real, _dev(R.images(h, w, N, seed=3)), directions=theta)
    shifted = sliced(real, _dev(R.images(h, w, N, seed=2, shift=0.25)), directions=theta)
    print(f"properties {shape}: swd unshifted {plain['swd']:.4g} +- {plain['swd_err']:.2g}, shifted by 0.25 "
          f"{shifted['swd']:.4g} +- {shifted['swd_err']:.2g}")
    assert shifted["swd"] > plain["swd"] > 0
    assert set(plain) == {"swd", "swd_err", "swd_max"}


# ------------------------------------------------------------------------------------------ 9. workspace path
def test_past_the_lds_limit_of_the_wasserstein_kernel():
    from expertsim import hip
    from expertsim.train.sliced import sliced_device
    h, w, N, P = 6, 5, 4200, 16
    assert 2 * N > hip.WS_LDS_MAX
    raw = sliced_device(_dev(R.images(h, w, N, seed=1)), _dev(R.images(h, w, N, seed=2, shift=0.25)),
                        directions=_dev(R.normal_theta(P, h * w)))
    pr, pf = raw["proj_real"].cpu().numpy(), raw["proj_fake"].cpu().numpy()
    ref = R.w_table(pr, pf, [np.arange(N)])
    bound = R.ws_bound(2 * N, ref)
    err = np.abs(raw["w"].cpu().numpy() - ref)
    print(f"workspace path N={N} P={P}: worst error / bound {_ratio(err, bound):.3g}")
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------ 10. wiring
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


def _swd_keys(E):
    from expertsim.train.sliced import KEYS
    return set(KEYS) | {f"{n}_{e}" for n in KEYS for e in range(E)}


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_evaluate_device_sliced():
    from expertsim.train import sliced as S
    E, N, seed, P = 3, 64, 17, 64
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, sliced=True, sliced_proj=P)
    extra = {"swd_real", "swd_gen", "swd_theta", "swd_w", "swd_proj_real", "swd_proj_gen"}
    assert set(det) == set(plain) | _swd_keys(E) | extra
    for key, v in plain.items():                                                   # bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(_bytes(det[key]), _bytes(v)), key
        else:
            assert det[key] == v, key
    assert all(np.isfinite(det[n]) for n in S.KEYS), {n: det[n] for n in S.KEYS}
    assert det["swd_max"] >= det["swd"] > 0 and tuple(det["swd_w"].shape) == (E + 1, P)
    assert tuple(det["swd_theta"].shape) == (P, 44 * 44)
    assert torch.equal(_bytes(det["swd_theta"]), _bytes(S.directions(P, 44 * 44, seed=seed)))
    assert torch.equal(_bytes(det["swd_real"]), _bytes(x.to(DEV)))                 # the stored log1p domain
    again = moe.evaluate_device(5, cond, x, cfg, seed=seed, sliced=True, sliced_proj=P)
    assert set(again) == {k for k, v in plain.items() if not isinstance(v, torch.Tensor)} | _swd_keys(E)
    assert all(_same_float(again[k], det[k]) for k in again)
    want = S.sliced(det["swd_real"], det["swd_gen"], det["expert"], E, n_proj=P, seed=seed)
    assert set(want) == _swd_keys(E) and all(_same_float(det[k], v) for k, v in want.items())
    other = moe.evaluate_device(5, cond, x, cfg, seed=seed, sliced=True, sliced_proj=P // 2)
    assert other["swd"] != det["swd"] and other["ws_mean"] == det["ws_mean"]
    both = moe.evaluate_device(5, cond, x, cfg, seed=seed, sliced=True, sliced_proj=P, prdc=True, distances=True)
    alone = moe.evaluate_device(5, cond, x, cfg, seed=seed, prdc=True, distances=True)
    assert set(both) == set(alone) | _swd_keys(E)
    assert all(_same_float(both[k], alone[k]) for k in alone) and all(_same_float(both[k], det[k]) for k in _swd_keys(E))


def test_evaluate_epoch_averages_sliced():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    E, N, bs, P = 3, 106, 48, 32
    on = ("train.eval_on_device=true", "train.eval_sliced=true", f"train.eval_sliced_proj={P}")
    moe, cfg = _moe(E, extra=on)
    b, x, cond = _batch(N)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg, device=torch.device(DEV))
    cfg_off = _cfg(E, extra=("train.eval_on_device=true",))
    off = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_off, device=torch.device(DEV))
    assert set(out) == set(off) | _swd_keys(E) and all(out[key] == off[key] for key in off)
    per = [moe.evaluate_device(0, cond[i:i + bs], x[i:i + bs], cfg, seed=int(cfg.train.rng_seed), sample_offset=i,
                               sliced=True, sliced_proj=P) for i in range(0, N, bs)]
    assert all(np.isfinite(m["swd"]) for m in per) and np.isfinite(out["swd"])
    for key in _swd_keys(E):
        finite = [m[key] for m in per if np.isfinite(m[key])]
        if finite:
            assert out[key] == sum(finite) / len(finite), key
        else:
            assert np.isnan(out[key]), key
    cfg_bad = _cfg(E, extra=("train.eval_sliced=true",))
    with pytest.raises(ValueError, match="train.eval_sliced needs train.eval_on_device"):
        evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_bad, device=torch.device(DEV))


def test_cli_simulate_real_sliced(tmp_path):
    from expertsim.train import sliced as S
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    E, N, P = 3, 64, 48
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
                        "--sim-batch-size", "16", "--real", str(tmp_path / "real.npy"), "--sliced", "--sliced-proj",
                        str(P), "--seed", "5", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert _swd_keys(E) <= set(z.files) and int(z["swd_proj"]) == P
    images, expert = torch.from_numpy(z["images"]).to(DEV), torch.from_numpy(z["expert"]).to(DEV)
    want = S.sliced(x.to(DEV), torch.log1p(images), expert, E, n_proj=P, seed=5)
    for key in _swd_keys(E):
        assert z[key].dtype == np.float64 and _same_float(float(z[key]), want[key]), key
        assert f"{key} = " in r.stdout
    assert np.isfinite(float(z["swd"])) and float(z["swd"]) > 0
