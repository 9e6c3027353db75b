"""The routed fast-simulation path on the GPU: es_bn_fold, es_conv2d_fwd_affine, generator.infer,
MoEWrapper.simulate, get_predictions_from_experts_results and ``cli.py --simulate``.

Tolerances: images <= 1e-4 of max|ref| in fp32 (the project's image bound, test_eval_gpu.py /
SURVEY.md §8(c)); bf16 convs <= 3e-2 of max|ref| (test_kernels_gpu.py, the same conv shapes in bf16);
the BatchNorm fold <= 1e-6 relative (a handful of fp32 roundings plus the device rsqrt); fp64 channel
sums of fp32 data <= 1e-6 relative.  The conv references at N = 192 are float64 CPU convolutions of
eight images spread over every 64-image group (a convolution is per image, so their reference is
exact for them), which keeps each case to seconds; every image is also compared with the affine of the
plain es_conv2d_fwd output."""
import copy
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO
from golden_utils import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLOPE = 0.1


def running_stats(n, expert):
    i = np.arange(n, dtype=np.float64)
    return ((0.1 * np.sin(0.37 * i + expert)).astype(np.float32),
            (0.75 + 0.25 * np.cos(0.11 * i + 2 * expert)).astype(np.float32))


@pytest.fixture
def split_fp32():
    """The fp32 arithmetic MoEWrapper sets by default (split-fp32, level 2); restored afterwards."""
    from expertsim import hip, layers
    prev = layers.f32_split_level()
    layers.set_f32_split(True)
    yield
    hip.lib().es_conv_set_f32_split(prev)
    layers._F32_SPLIT = None


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------ 1. es_bn_fold
def _fold_inputs(Cn, e):
    mean, var = running_stats(Cn, e)
    i = np.arange(Cn, dtype=np.float64)
    gamma = (1.0 + 0.3 * np.sin(0.05 * i + e)).astype(np.float32)
    beta = (0.2 * np.cos(0.07 * i - e)).astype(np.float32)
    return gamma, beta, mean, var


@pytest.mark.parametrize("Cn", [1, 64, 21632])
def test_bn_fold_matches_float64(Cn):
    from expertsim import hip
    eps = 1e-5
    host = _fold_inputs(Cn, 1)
    g, b, m, v = (torch.from_numpy(a).to(DEV) for a in host)
    scale, shift = torch.empty(Cn, device=DEV), torch.empty(Cn, device=DEV)
    hip.call("es_bn_fold", hip.ptr(g), hip.ptr(b), hip.ptr(m), hip.ptr(v), Cn, eps, hip.ptr(scale), hip.ptr(shift),
             hip.stream_ptr())
    g64, b64, m64, v64 = (a.astype(np.float64) for a in host)
    rs = g64 / np.sqrt(v64 + np.float64(np.float32(eps)))
    rh = b64 - m64 * rs
    es = np.abs(scale.cpu().numpy() - rs).max() / np.abs(rs).max()
    eh = np.abs(shift.cpu().numpy() - rh).max() / np.abs(rh).max()
    print(f"bn_fold C={Cn}: scale rel {es:.2e} shift rel {eh:.2e}")
    assert es <= 1e-6 and eh <= 1e-6


def test_bn_fold_batch_is_bitwise_the_single_form():
    from expertsim import hip
    sizes = [1, 64, 21632, 256, 100]
    ins = [[torch.from_numpy(a).to(DEV) for a in _fold_inputs(c, e)] for e, c in enumerate(sizes)]
    single = []
    for (g, b, m, v), c in zip(ins, sizes):
        s, h = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        hip.call("es_bn_fold", hip.ptr(g), hip.ptr(b), hip.ptr(m), hip.ptr(v), c, 1e-5, hip.ptr(s), hip.ptr(h),
                 hip.stream_ptr())
        single.append((s, h))
    n = len(sizes)
    outs = [(torch.full((c,), float("nan"), device=DEV), torch.full((c,), float("nan"), device=DEV)) for c in sizes]
    arr = lambda ts: (C.c_void_p * n)(*[t.data_ptr() for t in ts])
    hip.call("es_bn_fold_batch", n, arr([i[0] for i in ins]), arr([i[1] for i in ins]), arr([i[2] for i in ins]),
             arr([i[3] for i in ins]), (C.c_int * n)(*sizes), (C.c_float * n)(*([1e-5] * n)),
             arr([o[0] for o in outs]), arr([o[1] for o in outs]), hip.stream_ptr())
    for (s, h), (bs, bh) in zip(single, outs):
        assert torch.equal(_bits(s), _bits(bs)) and torch.equal(_bits(h), _bits(bh))


# --------------------------------------------------------------------------- 2. es_conv2d_fwd_affine
LAYERS = {
    # name: (Cin, H, W, Cout, k, upsample); fc2 is the pixel-block linear: 16 x 1 pixel images, 1x1 conv
    "fc2": (256, 16, 1, 21632, 1, None),
    "c0": (128, 13, 13, 256, 3, (2, 2)),
    "c5": (256, 24, 24, 128, 3, (2, 2)),
    "c9": (128, 46, 46, 64, 2, None),
}


def _conv_case(name, N, dtype, seed=0):
    from expertsim.layers import Act, ConvOp, Upsample
    Cin, H, W, Cout, k, up = LAYERS[name]
    g = torch.Generator().manual_seed(seed + Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / np.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    scale = 0.5 + torch.rand(Cout, generator=g)
    shift = 0.5 * torch.randn(Cout, generator=g)
    op = ConvOp(torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV)),
                upsample=Upsample((H, W), scale=up) if up else None)
    xa = Act.nhwc(N, Cin, H, W, dtype, DEV)
    xa.t.copy_(x.permute(0, 2, 3, 1).reshape(-1).to(dtype))
    if name == "fc2":
        xa.px = 16
    return op, xa, (x, w, b, scale, shift)


def _reference(name, host, images):
    x, w, b, scale, shift = (t.double() for t in host)
    up = LAYERS[name][5]
    xs = x[images]
    if up:
        xs = F.interpolate(xs, scale_factor=up, mode="nearest")
    y = F.conv2d(xs, w, b)
    return F.leaky_relu(y * scale[None, :, None, None] + shift[None, :, None, None], SLOPE)


def _epi(scale, shift, act=2):
    from expertsim import hip
    s, h = scale.to(DEV).contiguous(), shift.to(DEV).contiguous()
    e = hip.Affine()
    e.scale, e.shift, e.act, e.slope = s.data_ptr(), h.data_ptr(), act, SLOPE
    return e, (s, h)


def _run_affine(op, xa, epi, out_dtype, out=None, plain=False):
    from expertsim import hip
    from expertsim.layers import Act
    d = op.desc(xa)
    cdt = xa.t.dtype
    if op.subpixel(d, cdt):
        d.subpixel = 1
        wk = op.packed(cdt, 2)
    else:
        wk = op.packed(cdt, 0)
    if out is None:
        out = Act.nhwc(d.N, d.K, d.P, d.Q, out_dtype, DEV)
    flag = C.c_int(-1)
    if plain:
        hip.call("es_conv2d_fwd", C.byref(d), xa.dt, xa.ptr, hip.strides4(xa.strides), hip.ptr(wk), hip.ptr(op.bias),
                 out.ptr, out.dt, hip.strides4(out.strides), hip.stream_ptr())
    else:
        hip.call("es_conv2d_fwd_affine", C.byref(d), xa.dt, xa.ptr, hip.strides4(xa.strides), hip.ptr(wk),
                 hip.ptr(op.bias), C.byref(epi), out.ptr, out.dt, hip.strides4(out.strides), C.byref(flag),
                 hip.stream_ptr())
    return out, flag.value


@pytest.mark.parametrize("N", [5, 192])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(LAYERS))
def test_conv_fwd_affine_layer_shapes(name, dtype, N, split_fp32):
    op, xa, host = _conv_case(name, N, dtype)
    epi, keep = _epi(host[3], host[4])
    ya, fused = _run_affine(op, xa, epi, dtype)
    assert fused == 1
    got = ya.torch_nchw().float()
    images = list(range(N)) if N <= 8 else [0, 1, 63, 64, 127, 128, N - 2, N - 1]
    ref = _reference(name, host, images)
    tol = 1e-4 if dtype == torch.float32 else 3e-2
    err = float((got[images].cpu().double() - ref).abs().max() / ref.abs().max())
    print(f"{name} N={N} {dtype}: rel err {err:.3e} (bound {tol})")
    assert err <= tol
    # every image: the same affine applied to the plain conv output (fp32 store)
    yp, _ = _run_affine(op, xa, None, torch.float32, plain=True)
    s, h = keep
    allref = F.leaky_relu(yp.torch_nchw() * s[None, :, None, None] + h[None, :, None, None], SLOPE)
    err_all = float((got - allref).abs().max() / allref.abs().max())
    print(f"{name} N={N} {dtype}: vs affine of the plain conv, all images: {err_all:.3e}")
    assert err_all <= (1e-4 if dtype == torch.float32 else 3e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(LAYERS))
def test_conv_fwd_affine_dynamic_rows(name, dtype, split_fp32):
    from expertsim import hip
    from expertsim.layers import Act
    N = 5
    op, xa, host = _conv_case(name, N, dtype)
    epi, keep = _epi(host[3], host[4])
    full, fused = _run_affine(op, xa, epi, dtype)
    assert fused == 1
    px = 16 if name == "fc2" else 1          # the pixel-block linear counts samples (= pixels)
    for rows in (3, 0):
        live = torch.tensor([rows * px], dtype=torch.int32, device=DEV)
        with hip.live_rows(N * px, live, live):
            d = op.desc(xa)
            assert d.rows is not None
            out = Act.nhwc(N, d.K, d.P, d.Q, dtype, DEV)
            out.t.fill_(-777.0)
            sentinel = out.t.clone()
            _, fused = _run_affine(op, xa, epi, dtype, out=out)
        assert fused == 1
        per = out.t.numel() // N
        assert torch.equal(_bits(out.t[:rows * per]), _bits(full.t[:rows * per]))
        assert torch.equal(_bits(out.t[rows * per:]), _bits(sentinel[rows * per:]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_fwd_affine_fallback_is_plain_fwd(dtype, split_fp32):
    """fc1 (C = 19, K = 256): no kernel with the epilogue -> fused = 0 and y is es_conv2d_fwd's, bit for bit."""
    from expertsim.layers import Act, ConvOp
    g = torch.Generator().manual_seed(4)
    op = ConvOp(torch.nn.Parameter((torch.randn(256, 19, generator=g) / 4).to(DEV)),
                torch.nn.Parameter(torch.randn(256, generator=g).to(DEV)))
    xa = Act.rows(5, 19, dtype, DEV)
    xa.t.copy_(torch.randn(5 * 19, generator=g).to(dtype))
    epi, keep = _epi(torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g))
    ya, fused = _run_affine(op, xa, epi, dtype)
    yp, _ = _run_affine(op, xa, None, dtype, plain=True)
    assert fused == 0
    assert torch.equal(_bits(ya.t), _bits(yp.t))


# ----------------------------------------------------------------------------------------- 3. infer
def _golden(arch):
    z = np.load(os.path.join(GOLDEN_DIR, f"eval_{arch}.npz"), allow_pickle=False)
    return z, json.loads(str(z["meta"]))


def _generators(arch, seed, n=2):
    from expertsim.config import inject_shared, load_config
    from expertsim.models import build_model
    cfg = inject_shared(load_config(overrides=[f"model.architecture={arch}", "train.precision=fp32"]))
    torch.manual_seed(seed)
    g0 = build_model(f"{arch}.generator", cfg.model.generator, DEV)
    gens = [g0] + [copy.deepcopy(g0) for _ in range(n - 1)]
    with torch.no_grad():
        for e, g in enumerate(gens):
            for m in g.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    mean, var = running_stats(m.num_features, e)
                    m.running_mean.copy_(torch.from_numpy(mean))
                    m.running_var.copy_(torch.from_numpy(var))
    return gens


def _infer_images(g, noise, cond, fused=True):
    x0 = torch.cat([noise, cond], dim=1).to(DEV).float().contiguous()
    with torch.no_grad():
        h6 = g.infer(x0, fused=fused)
        return torch.relu(h6.torch_nchw()[:, 0]).float().cpu().numpy()


@pytest.mark.parametrize("arch,fused", [("neutron", True), ("neutron", False), ("proton", False)])
def test_infer_matches_reference_golden(arch, fused, split_fp32):
    z, meta = _golden(arch)
    g = _generators(arch, meta["seed"])[1]
    n = meta["n_pred"]
    got = _infer_images(g, torch.from_numpy(z["pred/noise"]), torch.from_numpy(z["cond"][:n]), fused)
    ref = z["pred/raw"]
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)
    print(f"infer {arch} fused={fused}: rel err {err:.3e}")
    assert err <= 1e-4


@pytest.fixture(scope="module")
def b192():
    g = torch.Generator().manual_seed(21)
    return torch.randn(192, 10, generator=g), torch.randn(192, 9, generator=g)


@pytest.mark.parametrize("arch", ["neutron", "neutron56"])
def test_infer_matches_eval_fwd_b192(arch, b192, split_fp32):
    noise, cond = b192
    g = _generators(arch, 5)[1]
    with torch.no_grad():
        img, _ = g.fwd(noise.to(DEV), cond.to(DEV), train=False)
        ref = img.torch_nchw()[:, 0].float().cpu().numpy()
    for fused in (True, False):
        got = _infer_images(g, noise, cond, fused)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print(f"infer {arch} B=192 fused={fused} vs fwd(train=False): {err:.3e}")
        assert err <= 1e-4


def test_infer_bf16(b192, split_fp32):
    """bf16: infer(fused=False) against fwd(train=False) under the bf16 conv bound (3e-2 of max|ref|,
    test_kernels_gpu.py); the fused path skips one bf16 rounding of every conv output, so its rms
    distance to the fp32 result is no larger than the unfused path's."""
    noise, cond = b192
    g = _generators("neutron", 5)[1]
    ref32 = _infer_images(g, noise, cond, True)
    g.compute_dtype = torch.bfloat16
    with torch.no_grad():
        img, _ = g.fwd(noise.to(DEV), cond.to(DEV), train=False)
        fwd16 = img.torch_nchw()[:, 0].float().cpu().numpy()
    unf = _infer_images(g, noise, cond, False)
    fus = _infer_images(g, noise, cond, True)
    err = np.abs(unf - fwd16).max() / np.abs(fwd16).max()
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - ref32) ** 2)))
    print(f"bf16 infer(fused=False) vs fwd: {err:.3e}; rms to fp32: fused {rms(fus):.4e} unfused {rms(unf):.4e}")
    assert err <= 3e-2
    assert rms(fus) <= rms(unf)


# -------------------------------------------------------------------------------------- 4. simulate
def _moe(precision="fp32", E=3, seed=3):
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", f"train.precision={precision}",
                                 "model.router.diff_strength=1e-6"])
    torch.manual_seed(seed)
    moe = setup_moe_system(cfg, torch.device(DEV))
    with torch.no_grad():   # distinct, non-trivial running statistics per expert
        for e, g in enumerate(moe.generators):
            for m in g.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    mean, var = running_stats(m.num_features, e)
                    m.running_mean.copy_(torch.from_numpy(mean))
                    m.running_var.copy_(torch.from_numpy(var))
    return moe, cfg


def _cond(n, seed=11):
    from expertsim.utils.synthetic import make_batch
    return torch.from_numpy(make_batch(n, "neutron", seed=seed)["cond"]).to(DEV)


def _check_against_fwd(moe, cond, res, tol):
    """Each expert's eval-mode fwd on the rows it was given reproduces the log-domain images there."""
    expert = res["expert"].cpu().numpy()
    for e in range(moe.n_experts):
        ix = np.where(expert == e)[0]
        if len(ix) == 0:
            continue
        sel = torch.as_tensor(ix, device=DEV)
        img, _ = moe.generators[e].fwd(res["noise"][sel].contiguous(), cond[sel].contiguous(), train=False)
        ref = img.torch_nchw()[:, 0].float()
        got = res["images"][sel]
        err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-6))
        print(f"simulate expert {e} ({len(ix)} rows): rel err vs fwd(train=False) {err:.3e}")
        assert err <= tol
        if moe.generators[e].compute_dtype == torch.bfloat16:
            # bf16: fwd(train=False) is itself a bf16 approximation, so the two are compared through the
            # fp32 result of the same weights: the fused path skips one bf16 rounding per conv output and
            # must be no further (rms) from it than the existing bf16 eval forward is
            g = moe.generators[e]
            g.compute_dtype = torch.float32
            try:
                img32, _ = g.fwd(res["noise"][sel].contiguous(), cond[sel].contiguous(), train=False)
                ref32 = img32.torch_nchw()[:, 0].double()
            finally:
                g.compute_dtype = torch.bfloat16
            rms = lambda a: float(((a.double() - ref32) ** 2).mean().sqrt())
            print(f"  rms to the fp32 result: simulate {rms(got):.4e}, bf16 fwd(train=False) {rms(ref):.4e}")
            assert rms(got) <= rms(ref)
    return expert


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_simulate_three_experts(precision):
    from expertsim.train.utils import channel_sums
    moe, _ = _moe(precision)
    cond = _cond(96)
    log = moe.simulate(cond, seed=5, domain="log", sums=True)
    assert log["images"].shape == (96, 44, 44) and log["images"].dtype == torch.float32
    assert log["expert"].dtype == torch.int32 and log["sums"].dtype == torch.float64 and log["noise"].shape == (96, 10)
    assert bool(torch.isfinite(log["images"]).all())       # every position written (none left as allocated)
    # bf16: simulate and fwd(train=False) are two bf16 evaluations, each within the bf16 conv bound
    # (3e-2 of max|ref|, test_kernels_gpu.py) of the exact result, so within twice that of each other
    expert = _check_against_fwd(moe, cond, log, 1e-4 if precision == "fp32" else 6e-2)
    assert len(set(expert.tolist())) >= 1 and expert.min() >= 0 and expert.max() < 3
    ref_sums = channel_sums(log["images"], log_domain=True)
    assert torch.allclose(log["sums"], ref_sums, rtol=1e-6, atol=1e-9)
    pho = moe.simulate(cond, seed=5, domain="photons", sums=True)
    assert torch.equal(pho["expert"], log["expert"]) and torch.equal(pho["noise"], log["noise"])
    assert torch.allclose(pho["images"], torch.expm1(log["images"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(pho["sums"], ref_sums, rtol=1e-6, atol=1e-9)


def test_simulate_nan_prefill_every_position_written_once():
    """The chunk's static output buffer pre-filled with NaN: afterwards every value is finite."""
    moe, _ = _moe("fp32")
    cond = _cond(96)
    moe.simulate(cond, seed=1, domain="log", sums=True, graph=False)
    for st in moe._sim.values():
        st["images"].fill_(float("nan"))
        st["sums"].fill_(float("nan"))
    res = moe.simulate(cond, seed=1, domain="log", sums=True, graph=False)
    assert bool(torch.isfinite(res["images"]).all()) and bool(torch.isfinite(res["sums"]).all())


def test_simulate_argmax_and_empty_experts():
    moe, _ = _moe("fp32")
    cond = _cond(96)
    res = moe.simulate(cond, seed=2, domain="log", routing="argmax")
    _, logits = moe.router(cond)
    assert np.array_equal(res["expert"].cpu().numpy(), torch.argmax(logits, 1).cpu().numpy().astype(np.int32))
    _check_against_fwd(moe, cond, res, 1e-4)
    with torch.no_grad():
        moe.router._modules["fc_layers"]._modules["6"].bias[0] += 100.0
    moe.router.invalidate()
    res = moe.simulate(cond, seed=2, domain="log", routing="argmax", sums=True)
    assert int(res["expert"].abs().sum()) == 0
    counts = next(st["counts"] for k, st in moe._sim.items() if k[4] == "argmax" and k[2])
    assert counts.cpu().tolist() == [96, 0, 0]
    assert bool(torch.isfinite(res["images"]).all()) and bool(torch.isfinite(res["sums"]).all())
    _check_against_fwd(moe, cond, res, 1e-4)


# ----------------------------------------------------------------------- 5. determinism and chunking
def test_simulate_determinism_and_chunking():
    moe, _ = _moe("fp32")
    cond = _cond(200, seed=12)
    a = moe.simulate(cond, seed=9, batch_size=64, domain="log")
    b = moe.simulate(cond, seed=9, batch_size=200, domain="log")
    assert torch.equal(a["expert"], b["expert"]) and torch.equal(_bits(a["noise"]), _bits(b["noise"]))
    err = float((a["images"] - b["images"]).abs().max() / b["images"].abs().max())
    print(f"chunk 64 vs 200: rel {err:.3e}")
    assert err <= 1e-4
    a2 = moe.simulate(cond, seed=9, batch_size=64, domain="log")
    for k in ("images", "noise", "expert"):
        assert torch.equal(_bits(a[k]) if a[k].dtype != torch.int32 else a[k], _bits(a2[k]) if a2[k].dtype != torch.int32 else a2[k])
    c = moe.simulate(cond, seed=10, batch_size=64, domain="log")
    assert not torch.equal(c["noise"], a["noise"])
    d = moe.simulate(cond[64:128], seed=9, sample_offset=64, batch_size=64, domain="log")
    assert torch.equal(_bits(d["noise"]), _bits(a["noise"][64:128])) and torch.equal(d["expert"], a["expert"][64:128])
    assert torch.equal(_bits(d["images"]), _bits(a["images"][64:128]))


# ----------------------------------------------------------------------------------------- 6. graph
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_simulate_graph_capture_then_replay(precision):
    moe, _ = _moe(precision)
    c1, c2 = _cond(64, seed=13), _cond(64, seed=14)
    cap0, rep0 = moe.sim_captures, moe.sim_replays
    g1 = moe.simulate(c1, seed=3, sums=True, graph=True)
    g1 = {k: v.clone() for k, v in g1.items()}
    g2 = moe.simulate(c2, seed=4, sums=True, graph=True)
    assert (moe.sim_captures - cap0, moe.sim_replays - rep0) == (1, 1)
    for c, s, g in ((c1, 3, g1), (c2, 4, g2)):
        e = moe.simulate(c, seed=s, sums=True, graph=False)
        for k in ("images", "noise", "sums"):
            assert torch.equal(g[k].view(torch.uint8), e[k].view(torch.uint8)), k
        assert torch.equal(g["expert"], e["expert"])


# ------------------------------------------------------------------- 7. no side effects, freshness
def _step(moe, opts, b):
    og, od, oa, orr = opts
    t = lambda k: torch.from_numpy(b[k]).to(DEV)
    return moe.train_step(0, t("cond"), t("real_images").unsqueeze(1), t("true_positions"), t("std"),
                          t("intensity"), oa, og, od, orr, None, DEV)


def _state(moe, opts):
    out = {}
    mods = {"router": moe.router, **{f"G{i}": g for i, g in enumerate(moe.generators)},
            **{f"D{i}": g for i, g in enumerate(moe.discriminators)}, **{f"A{i}": g for i, g in enumerate(moe.aux_regs)}}
    for n, m in mods.items():
        for k, v in m.state_dict().items():
            out[f"{n}.{k}"] = v.detach().clone()
    flat = [o for grp in opts[:3] for o in grp] + [opts[3]]
    for i, o in enumerate(flat):
        def walk(prefix, x):
            if isinstance(x, torch.Tensor):
                out[prefix] = x.detach().clone()
            elif isinstance(x, dict):
                for k, v in x.items():
                    walk(f"{prefix}.{k}", v)
            elif isinstance(x, (list, tuple)):
                for k, v in enumerate(x):
                    walk(f"{prefix}.{k}", v)
            else:
                out[prefix] = x
        walk(f"opt{i}", o.state_dict())
    out["step_count"] = moe.step_count
    out["rng"] = moe.rng.counter
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].reshape(-1).contiguous().view(torch.uint8), b[k].reshape(-1).contiguous().view(torch.uint8)), k
        else:
            assert a[k] == b[k], k


def test_simulate_no_side_effects_and_fresh_weights():
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.utils.synthetic import make_batch
    batches = [make_batch(48, "neutron", seed=40 + i) for i in range(2)]
    cond = _cond(64, seed=15)
    runs = []
    for with_sim in (False, True):
        moe, cfg = _moe("fp32")
        opts = setup_optimizers(moe, cfg)
        _step(moe, opts, batches[0])
        flags = [m.training for m in moe.modules()]
        if with_sim:
            before = _state(moe, opts)
            first = moe.simulate(cond, seed=6, domain="log", graph=True)
            _same(before, _state(moe, opts))
            assert flags == [m.training for m in moe.modules()]
            first = {k: v.clone() for k, v in first.items()}
        met = _step(moe, opts, batches[1])
        torch.cuda.synchronize()
        runs.append(({k: float(v) for k, v in met.items()}, _state(moe, opts)))
    assert runs[0][0] == runs[1][0]
    _same(runs[0][1], runs[1][1])
    # the replayed graph reads the new weights and running statistics
    rep0 = moe.sim_replays
    again = moe.simulate(cond, seed=6, domain="log", graph=True)
    assert moe.sim_replays == rep0 + 1
    assert not torch.equal(again["images"], first["images"])
    _check_against_fwd(moe, cond, again, 1e-4)


# --------------------------------------------------------------------------- 8. reference API, CLI
def test_get_predictions_from_experts_results(split_fp32):
    from expertsim.train.utils import get_predictions_from_experts_results
    moe, _ = _moe("fp32")
    cond = _cond(96)
    g = torch.Generator().manual_seed(8)
    noise = torch.randn(96, 10, generator=g)
    sim = moe.simulate(cond, noise=noise, routing="argmax", domain="photons")
    got = get_predictions_from_experts_results(96, 10, torch.device(DEV), cond, moe.router, list(moe.generators),
                                               shape_images=(44, 44), input_noise=noise,
                                               input_expo=torch.ones(96, 3))
    assert got.shape == (96, 44, 44) and got.dtype == np.float64
    ref = sim["images"].double().cpu().numpy()
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()


@pytest.mark.timeout(600)
def test_cli_simulate(tmp_path):
    common = ["model.architecture=neutron", "dataset.input_image_shape=[44,44]", "model.n_experts=3",
              "train.batch_size=32", "dataset.synthetic_samples=128", "train.save_experiment_data=true",
              "train.ws_threshold_model_save=1e9", f"train.dir_models={tmp_path}/models/", "train.epochs=1"]
    cli = os.path.join(REPO, "cli.py")
    r = subprocess.run([sys.executable, cli, "--max-steps-per-epoch", "1", "-o", *common], capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = tmp_path / "sim.npz"
    r = subprocess.run([sys.executable, cli, "-o", *common, "--simulate", "--checkpoint", f"{tmp_path}/models/",
                        "--num-samples", "40", "--sim-batch-size", "16", "--out", str(out)], capture_output=True,
                       text=True, timeout=500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert z["images"].shape == (40, 44, 44) and z["expert"].shape == (40,) and z["sums"].shape == (40, 5)
    assert z["cond"].shape == (40, 9)
    for k in ("images", "expert", "sums", "cond"):
        assert np.isfinite(z[k]).all(), k
