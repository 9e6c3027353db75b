"""Shower-shape observables on the GPU: es_image_features against its fp64 restatement
(tests/feature_refs.py, bit for bit) and the reference's record (tests/golden/image_features.npz), and the
feature outputs of MoEWrapper.simulate, MoEWrapper.evaluate_device, loop.evaluate_epoch and
``cli.py --simulate --features``.

Tolerances: the kernel's arithmetic order is fixed (include/expertsim_hip.h), so feat is compared bitwise
and peak exactly with the restatement; against the reference's float32 sums max_x / max_y hold the float32
summation bound of feature_refs.max_sum_bounds and the rest is exact; fp64 sums of fp32 data against numpy's
expm1 <= 1e-6 relative (tests/test_eval_gpu.py); every device Wasserstein distance within
2 (nu + nv) 2^-52 relative of scipy's (tests/test_wasserstein_gpu.py), and a mean of non-negative numbers
inherits the largest relative error of its terms (tests/test_eval_device_gpu.py), the std 1e-12 x the
mean absolute."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import feature_refs as FR
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"
NS = (1, 5, 9)          # 9 = two full blocks of four images and one with a single image (64x64: 4 + 1)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _check(x_dev, feat_ref, peak_ref, what):
    from expertsim.train.utils import image_features
    feat, peak = image_features(x_dev)
    assert feat.dtype == torch.float64 and peak.dtype == torch.int32 and feat.is_cuda and peak.is_cuda
    assert feat.shape == feat_ref.shape and peak.shape == peak_ref.shape
    f, p = feat.cpu().numpy(), peak.cpu().numpy()
    assert np.array_equal(f.view(np.int64), feat_ref.view(np.int64)), (what, f, feat_ref)
    assert np.array_equal(p, peak_ref), (what, p, peak_ref)


# ------------------------------------------------------------------------ 1. kernel = restatement
@pytest.mark.parametrize("layout", ["dense", "slice", "transposed", "bf16"])
@pytest.mark.parametrize("shape", FR.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_restatement(shape, layout):
    h, w = shape
    for n in NS:
        x, feat_ref, peak_ref = FR.case(h, w, n)
        t = torch.from_numpy(x.copy())
        if layout == "dense":
            xd = t.to(DEV)
        elif layout == "slice":        # a window of a wider buffer; the rest would dominate every result
            buf = torch.full((n, h + 3, w + 5), 1e30, dtype=torch.float32, device=DEV)
            xd = buf[:, 1:1 + h, 2:2 + w]
            xd.copy_(t)
            assert not xd.is_contiguous() or h * w == 1
        elif layout == "transposed":   # an [n,w,h] buffer viewed as [n,h,w]
            buf = t.transpose(1, 2).contiguous().to(DEV)
            xd = buf.transpose(1, 2)
            assert xd.shape == (n, h, w) and xd.stride() == (h * w, 1, h)
        else:                          # bf16: the restatement sees the rounded values
            xd = t.to(DEV).to(torch.bfloat16)
            feat_ref, peak_ref = FR.image_features_ref(xd.float().cpu().numpy())
        _check(xd, feat_ref, peak_ref, (shape, layout, n))


def test_result_does_not_depend_on_batch_or_position():
    from expertsim.train.utils import image_features
    x, _, _ = FR.case(44, 44, 9)
    t = torch.from_numpy(x.copy()).to(DEV)
    feat, peak = image_features(t)
    rev_f, rev_p = image_features(t.flip(0))
    one_f, one_p = image_features(t[6:7])
    assert _same(rev_f.flip(0), feat) and torch.equal(rev_p.flip(0), peak)
    assert _same(one_f, feat[6:7]) and torch.equal(one_p, peak[6:7])


@pytest.mark.parametrize("shape", FR.GOLDEN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_the_reference_record(shape):
    from expertsim.train.utils import calculate_image_features, image_features
    images, gfeat, _ = FR.golden()[shape]
    feat, peak = image_features(torch.from_numpy(images.copy()))          # host input: copied to the device
    FR.assert_matches_golden(feat.cpu().numpy(), peak.cpu().numpy(), shape)
    ref_api = calculate_image_features(images.copy())                     # the reference's [5, N] convention
    assert ref_api.shape == gfeat.shape and ref_api.dtype == np.float64
    assert np.array_equal(ref_api, feat.cpu().numpy().T)


# ------------------------------------------------------------------------------------ 2. edges
def _raw(x, feat, peak, dims=None, log_domain=0):
    from expertsim import hip
    n, h, w = x.shape
    v = hip.make_view(dims or (n, 1, h, w), (x.stride(0), h * w, x.stride(1), x.stride(2)), False)
    return hip.call("es_image_features", C.byref(v), hip.dt_of(x), hip.ptr(x), log_domain, hip.ptr(feat),
                    hip.ptr(peak), hip.stream_ptr())


def test_empty_batch_and_argument_errors():
    from expertsim import hip
    from expertsim.train.utils import image_features
    feat, peak = image_features(torch.empty(0, 4, 4, device=DEV))
    assert feat.shape == (0, 5) and peak.shape == (0, 2) and feat.dtype == torch.float64 and peak.dtype == torch.int32
    x = torch.zeros(2, 70, 70, device=DEV)
    f = torch.full((2, 5), -7.0, dtype=torch.float64, device=DEV)
    p = torch.full((2, 2), -7, dtype=torch.int32, device=DEV)
    assert _raw(x[:, :4, :4], f, p, dims=(0, 1, 4, 4)) == 0     # n = 0: ES_OK, nothing launched
    for bad in (x[:, :65, :4], x[:, :4, :65]):
        with pytest.raises(hip.HipError, match="es_image_features failed"):
            _raw(bad, f, p)
    with pytest.raises(hip.HipError, match="one channel"):
        _raw(x[:, :4, :4], f, p, dims=(2, 2, 4, 4))
    with pytest.raises(hip.HipError, match="both outputs"):
        _raw(x[:, :4, :4], None, None)
    torch.cuda.synchronize()
    assert bool((f == -7.0).all()) and bool((p == -7).all())    # none of them wrote anything


def test_either_output_alone():
    x, feat_ref, peak_ref = FR.case(7, 5, 5)
    xd = torch.from_numpy(x.copy()).to(DEV)
    f = torch.full((5, 5), -7.0, dtype=torch.float64, device=DEV)
    p = torch.full((5, 2), -7, dtype=torch.int32, device=DEV)
    _raw(xd, f, None)
    assert np.array_equal(f.cpu().numpy().view(np.int64), feat_ref.view(np.int64)) and bool((p == -7).all())
    f.fill_(-7.0)
    _raw(xd, None, p)
    assert np.array_equal(p.cpu().numpy(), peak_ref) and bool((f == -7.0).all())


# ------------------------------------------------------------------------------------ 3. models
def running_stats(n, expert):
    i = np.arange(n, dtype=np.float64)
    return ((0.1 * np.sin(0.37 * i + expert)).astype(np.float32),
            (0.75 + 0.25 * np.cos(0.11 * i + 2 * expert)).astype(np.float32))


def _moe(E, precision="fp32", extra=(), seed=4):   # seed 4: dense, non-zero generator images
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", f"train.precision={precision}",
                                 "model.router.diff_strength=1e-6", *extra])
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


def test_log_domain_is_the_photon_images():
    from expertsim.train.utils import image_features
    moe, _ = _moe(1)
    _, _, cond = _batch(8)
    L = moe.simulate(cond, seed=21, domain="log")["images"]
    P = moe.simulate(cond, seed=21, domain="photons")["images"]
    fl, pl = image_features(L, log_domain=True)
    fp, pp = image_features(P)
    assert _same(fl, fp) and torch.equal(pl, pp)
    # numpy's float32 expm1 may differ from the device's in the last bits: sums to 1e-6 relative, and the
    # rest exactly where the peak is separated from the runner-up by more than 1e-3 relative
    host = np.expm1(L.cpu().numpy())
    assert host.dtype == np.float32
    ref_f, ref_p = FR.image_features_ref(host)
    got_f, got_p = fl.cpu().numpy(), pl.cpu().numpy()
    top2 = np.sort(host.reshape(8, -1), axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * np.abs(top2[:, 1])
    rel = np.abs(got_f[:, :2] - ref_f[:, :2]) / np.maximum(np.abs(ref_f[:, :2]), 1e-300)
    print(f"log_domain vs numpy expm1: max-sum rel {rel.max():.2e}; {int(clear.sum())} of 8 peaks separated")
    assert (rel <= 1e-6).all()
    assert clear.any()
    assert np.array_equal(got_f[clear, 2:], ref_f[clear, 2:]) and np.array_equal(got_p[clear], ref_p[clear])


@pytest.mark.parametrize("E", [1, 3])
def test_simulate_features(E):
    from expertsim.train.utils import image_features
    moe, _ = _moe(E)
    _, _, cond = _batch(40)
    kw = dict(seed=5, batch_size=16, sums=True)                       # chunks 16, 16, 8
    old = ("images", "sums", "expert", "noise")
    plain = {k: v.clone() for k, v in moe.simulate(cond, graph=True, **kw).items()}
    assert set(plain) == set(old)
    cap0, rep0 = moe.sim_captures, moe.sim_replays
    g = {k: v.clone() for k, v in moe.simulate(cond, graph=True, features=True, **kw).items()}
    assert (moe.sim_captures - cap0, moe.sim_replays - rep0) == (2, 1)   # the 16- and the 8-row program
    assert set(g) == set(old) | {"features", "peak"}
    assert g["features"].shape == (40, 5) and g["features"].dtype == torch.float64
    assert g["peak"].shape == (40, 2) and g["peak"].dtype == torch.int32
    for k in old:                                                     # the flag changes nothing else
        assert torch.equal(g[k].view(torch.uint8), plain[k].view(torch.uint8)), k
    feat, peak = image_features(g["images"])
    assert _same(g["features"], feat) and torch.equal(g["peak"], peak)
    # a second call replays every chunk and captures nothing
    cap1, rep1 = moe.sim_captures, moe.sim_replays
    g2 = moe.simulate(cond, graph=True, features=True, **kw)
    assert (moe.sim_captures - cap1, moe.sim_replays - rep1) == (0, 3)
    for k in g:
        assert torch.equal(g2[k].view(torch.uint8), g[k].view(torch.uint8)), k
    # graph replay = eager, with and without the flag
    e = moe.simulate(cond, graph=False, features=True, **kw)
    for k in g:
        assert torch.equal(e[k].view(torch.uint8), g[k].view(torch.uint8)), k
    e0 = moe.simulate(cond, graph=False, **kw)
    assert set(e0) == set(old)
    for k in old:
        assert torch.equal(e0[k].view(torch.uint8), plain[k].view(torch.uint8)), k
    # the observables describe the images as returned
    lg = moe.simulate(cond, graph=False, features=True, domain="log", **kw)
    feat, peak = image_features(lg["images"])
    assert _same(lg["features"], feat) and torch.equal(lg["peak"], peak)
    assert not torch.equal(lg["features"][:, :2], g["features"][:, :2])
    assert (moe.sim_captures, moe.sim_replays) == (cap1, rep1 + 3)


def _old_keys(E):
    return {"ws_mean", "ws_std", *[f"ws_mean_{i}" for i in range(E)], *[f"ws_std_{i}" for i in range(E)], "epoch"}


def _new_keys(E):
    from expertsim.train.utils import FEATURE_NAMES
    return {k for n in FEATURE_NAMES for k in (f"ws_feat_{n}", f"ws_feat_std_{n}", *[f"ws_feat_{n}_{e}" for e in range(E)])}


def test_evaluate_device_features():
    from scipy.stats import wasserstein_distance

    from expertsim.train.utils import FEATURE_NAMES, image_features
    E, N, seed = 3, 40, 17
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)          # R = 2
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, features=True)
    tensors = {"sums_real", "sums_gen", "expert", "ws"}
    assert set(plain) == _old_keys(E) | tensors
    assert set(det) == _old_keys(E) | tensors | _new_keys(E) | {"feat_real", "feat_gen", "ws_feat"}
    assert all(det[k] == plain[k] for k in _old_keys(E))                           # bit for bit
    assert all(torch.equal(det[k].view(torch.uint8), plain[k].view(torch.uint8)) for k in tensors)
    short = moe.evaluate_device(5, cond, x, cfg, seed=seed, features=True)
    assert set(short) == _old_keys(E) | _new_keys(E) and all(short[k] == det[k] for k in short)
    assert det["feat_real"].shape == (N, 5) and det["feat_gen"].shape == (2, N, 5) and det["ws_feat"].shape == (2, E + 1, 5)
    fr, _ = image_features(x.to(DEV), log_domain=True)
    assert _same(det["feat_real"], fr)
    sim0 = moe.simulate(cond, seed=seed, sums=True, features=True)
    assert _same(det["feat_gen"][0], sim0["features"])
    # scipy on the host copies, per repetition, segment and feature
    real, gen, expert = (det[k].cpu().numpy() for k in ("feat_real", "feat_gen", "expert"))
    ws_dev = det["ws_feat"].cpu().numpy()
    ref = np.zeros((2, E + 1, 5))
    worst = 0.0
    for j in range(2):
        for s in range(E + 1):
            ix = np.arange(N) if s == 0 else np.where(expert == s - 1)[0]
            if len(ix) == 0:
                continue
            for k in range(5):
                ref[j, s, k] = wasserstein_distance(real[ix, k], gen[j][ix, k])
                bound = 2 * (2 * len(ix)) * 2.0 ** -52 * ref[j, s, k]
                err = abs(ws_dev[j, s, k] - ref[j, s, k])
                worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else np.inf))
                assert err <= bound, (j, s, k, ws_dev[j, s, k], ref[j, s, k])
    print(f"evaluate_device features: worst distance error / bound {worst:.3f}; counts "
          f"{np.bincount(expert, minlength=E).tolist()}; joint {dict(zip(FEATURE_NAMES, ref[:, 0].mean(axis=0)))}")
    rel = 2 * (2 * N) * 2.0 ** -52
    for k, name in enumerate(FEATURE_NAMES):
        m, s = ref[:, 0, k].mean(), ref[:, 0, k].std()
        assert abs(det[f"ws_feat_{name}"] - m) <= rel * m
        assert abs(det[f"ws_feat_std_{name}"] - s) <= 1e-12 * m
        for e in range(E):
            me = ref[:, 1 + e, k].mean()
            assert abs(det[f"ws_feat_{name}_{e}"] - me) <= rel * me
    assert det["ws_feat_max_x"] > 0 and det["ws_feat_center_x"] > 0
    again = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, features=True)
    assert all(again[k] == det[k] for k in _old_keys(E) | _new_keys(E))
    assert all(torch.equal(again[k].view(torch.uint8), det[k].view(torch.uint8))
               for k in tensors | {"feat_real", "feat_gen", "ws_feat"})


def test_evaluate_epoch_with_eval_features():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    moe, cfg = _moe(3, extra=("train.eval_on_device=true", "train.eval_features=true"))
    b, x, cond = _batch(40)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=40), epoch=5, cfg=cfg, device=torch.device(DEV))
    assert set(out) == (_old_keys(3) | _new_keys(3)) - {"epoch"}
    one = moe.evaluate_device(5, cond, x, cfg, seed=int(cfg.train.rng_seed), features=True)
    assert all(out[k] == float(one[k]) for k in out)                  # one batch: its own metrics


def test_cli_simulate_features(tmp_path):
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    import cli
    moe, cfg = _moe(3)
    models = tmp_path / "models"
    models.mkdir()
    save_checkpoint(str(models), 0, moe, *setup_optimizers(moe, cfg))
    common = ["-o", "model.architecture=neutron", "dataset.input_image_shape=[44,44]", "model.n_experts=3",
              "model.router.diff_strength=1e-6", "--simulate", "--checkpoint", str(models), "--num-samples", "40",
              "--sim-batch-size", "16"]
    out = tmp_path / "sim_features.npz"
    r = subprocess.run([sys.executable, os.path.join(REPO, "cli.py"), *common, "--out", str(out), "--features"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert set(z.files) == {"images", "expert", "sums", "cond", "features", "peak"}
    assert z["features"].shape == (40, 5) and z["features"].dtype == np.float64
    assert z["peak"].shape == (40, 2) and z["peak"].dtype == np.int32
    ref_f, ref_p = FR.image_features_ref(z["images"])
    assert np.array_equal(z["features"].view(np.int64), ref_f.view(np.int64)) and np.array_equal(z["peak"], ref_p)
    # without the flag (the same entry point, in this process) the file is what it was
    plain = tmp_path / "sim.npz"
    cli.simulate(cli.parse_args([*common, "--out", str(plain)]))
    zp = np.load(plain)
    assert set(zp.files) == {"images", "expert", "sums", "cond"}
    assert np.array_equal(zp["images"], z["images"]) and np.array_equal(zp["sums"], z["sums"])
