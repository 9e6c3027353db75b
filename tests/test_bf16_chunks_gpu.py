"""bf16 ring convolutions over image chunks.

The ring kernels address their gathered operand with 32-bit buffer offsets (out-of-range marker at
2^31), so operands of >= 1 GiB launch as image chunks (es_conv_ring_launch): a capacity-2048 expert's
conv_layers.5 output gradient is 1.1 GB in bf16 (BASELINE configs[3], E = 4, B = 2048 on one GPU),
which before the chunks fell back to the generic GEMM kernels (c5 WGRAD 5.3 ms instead of ~1.3).
Forced small chunks (es_conv_set_f32_chunk, the same knob as the fp32 ring) must give the FWD /
DGRAD of the whole-batch launch bit for bit (each output element's K order does not depend on the
row tiling) and its WGRAD up to the order of the float atomics; against torch fp64 within the bf16
tolerance of tests/test_kernels_gpu.py.

Reference: upsample + conv2d of neutron/generator.py:23-35 (torch CPU fp64).
"""
import pytest
import torch

from test_f32_ring_gpu import _ref
from test_kernels_gpu import DEV, _bnred_operands, _hip, from_act, rel, to_act

pytestmark = pytest.mark.gpu

CASES = [
    (130, 256, 24, 24, 128, 3, 1, 0, 2),   # neutron G conv_layers.5 (sub-pixel), ragged last chunk
    (70, 128, 46, 46, 64, 2, 1, 0, None),  # neutron G conv_layers.9
]


def _run(case, x, w, b, gy):
    from expertsim.layers import ConvOp, Upsample
    N, Cin, H, W, Cout, k, st, pad, up = case
    upsample = Upsample((H, W), scale=(up, up)) if up else None
    op = ConvOp(torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV)), stride=st, pad=pad, upsample=upsample)
    xa = to_act(x, torch.bfloat16)
    ya = op.fwd(xa, out_dtype=torch.bfloat16)
    gya = to_act(gy, torch.bfloat16)
    dxa = op.dgrad(gya, xa, dx_dtype=torch.bfloat16)
    dw = torch.zeros_like(op.weight)
    op.wgrad(gya, xa, dw, None, beta=1.0)
    torch.cuda.synchronize()
    return from_act(ya).float(), from_act(dxa).float(), dw.cpu()


@pytest.fixture
def perf_mode():
    from expertsim import layers
    old = layers.deterministic()
    layers.set_deterministic(False)
    yield
    layers.set_deterministic(old)


@pytest.mark.parametrize("case", CASES)
def test_bf16_ring_image_chunks(case, perf_mode):
    hip = _hip()
    x, w, b, gy, y, gx, gw, gb = _ref(case, seed=7)
    full = _run(case, x, w, b, gy)
    launches = hip.lib().es_conv_launch_count()
    old = hip.lib().es_conv_set_f32_chunk(64)
    try:
        part = _run(case, x, w, b, gy)
    finally:
        hip.lib().es_conv_set_f32_chunk(old)
    # the chunked pass launched ring kernels per chunk (not the generic fallback)
    assert hip.lib().es_conv_launch_count() - launches >= 3 * ((case[0] + 63) // 64) - 1
    assert torch.equal(full[0], part[0])
    assert torch.equal(full[1], part[1])
    assert rel(part[2].double(), gw) < 2e-2
    assert rel(part[2], full[2]) < 1e-3
    assert rel(part[0].double(), y) < 2e-2
    assert rel(part[1].double(), gx) < 2e-2


# sub-pixel FWD over chunks of 64 + 64 + 2 images: 128 x 128 tiles of 2 pixels x 64 images, 72 per
# parity class (12 x 12 class pixels), 4 classes -> 288 partials per full chunk; the ragged chunk runs
# 8-image groups, 16 pixels per tile, 9 tiles per class -> 36
STATS_CASE = (130, 128, 13, 13, 256, 3, 1, 0, 2)
STATS_CHUNKS = 288 + 288 + 36


@pytest.mark.parametrize("variant", ["bf16", "fp32", "fp32_split"])
def test_fused_bn_stats_over_image_chunks(variant):
    """ConvOp.fwd(bn_stats=True) over forced image chunks: every chunk appends its row tiles'
    BatchNorm partials behind those of the chunks before it, the reported count is their sum, the
    merged statistics are those of the stored output (expressions and tolerances of
    test_conv_fused_bn_stats / test_f32_ring_fused_bn_stats) and the output is bitwise the
    un-chunked one."""
    hip = _hip()
    from expertsim import layers
    from expertsim.layers import ConvOp, NormOp, Upsample
    N, Cin, H, W, Cout, k, st, pad, up = STATS_CASE
    dtype = torch.bfloat16 if variant == "bf16" else torch.float32
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g) + 2.0
    old_det, old_split = layers.deterministic(), layers.f32_split()
    layers.set_deterministic(variant != "bf16")
    layers.set_f32_split(variant == "fp32_split")
    try:
        op = ConvOp(torch.nn.Parameter(w.to(DEV)), torch.nn.Parameter(b.to(DEV)), stride=st, pad=pad,
                    upsample=Upsample((H, W), scale=(up, up)))
        xa = to_act(x, dtype)
        full = op.fwd(xa, out_dtype=dtype, bn_stats=True)
        old = hip.lib().es_conv_set_f32_chunk(64)
        try:
            ya = op.fwd(xa, out_dtype=dtype, bn_stats=True)
        finally:
            hip.lib().es_conv_set_f32_chunk(old)
        assert ya.bn_part is not None
        print("chunks", variant, ya.bn_part[1])
        assert ya.bn_part[1] == STATS_CHUNKS
        mk = lambda: NormOp(hip.NORM_BN, torch.ones(Cout, device=DEV), torch.zeros(Cout, device=DEV),
                            running_mean=torch.zeros(Cout, device=DEV), running_var=torch.ones(Cout, device=DEV))
        mean, invstd = mk().stats(ya)
        yt = from_act(ya).double()
        m_ref = yt.mean(dim=(0, 2, 3))
        i_ref = 1.0 / torch.sqrt(yt.var(dim=(0, 2, 3), unbiased=False) + 1e-5)
        print("stats vs fp64", variant, rel(mean.cpu().double(), m_ref), rel(invstd.cpu().double(), i_ref))
        # (the partials are fp32 arithmetic over the stored values in either precision)
        assert rel(mean.cpu().double(), m_ref) < 1e-5
        assert rel(invstd.cpu().double(), i_ref) < 1e-5
        if variant == "bf16":   # = es_norm_stats over the output of a plain fwd
            y0 = op.fwd(xa, out_dtype=dtype)
            assert torch.equal(y0.t, ya.t)
            n1, n0 = mk(), mk()
            m1, i1 = n1.stats(ya)
            m0, i0 = n0.stats(y0)
            assert rel(m1.cpu(), m0.cpu()) < 1e-5
            assert rel(i1.cpu(), i0.cpu()) < 1e-5
            assert rel(n1.rv.cpu(), n0.rv.cpu()) < 1e-5 and rel(n1.rm.cpu(), n0.rm.cpu()) < 1e-5
        assert torch.equal(ya.t, full.t)
    finally:
        layers.set_f32_split(old_split)
        layers.set_deterministic(old_det)


def test_bn_reduce_declined_over_image_chunks(perf_mode):
    """A chunked DGRAD does not take the fused BatchNorm-backward reduction (its chunks would each
    write the workgroup slots): dx.bn_sums stays None, the caller runs the reduction pass, and dx is
    bitwise the plain un-chunked dgrad.  The next, un-chunked call fuses again: a call leaves nothing
    behind for the one after it."""
    hip = _hip()
    op, bn, h, y, stats, ch, gy, kb = _bnred_operands((70, 128, 23, 21, 64, 2), True)   # noqa: F841
    plain = op.dgrad(gy, y, dx_dtype=torch.bfloat16)
    old = hip.lib().es_conv_set_f32_chunk(64)
    try:
        dx = op.dgrad(gy, y, dx_dtype=torch.bfloat16, bn_reduce=(bn, h, stats, ch))
    finally:
        hip.lib().es_conv_set_f32_chunk(old)
    assert dx.bn_sums is None
    assert torch.equal(dx.t, plain.t)
    again = op.dgrad(gy, y, dx_dtype=torch.bfloat16, bn_reduce=(bn, h, stats, ch))
    assert again.bn_sums is not None
    assert torch.equal(again.t, plain.t)
