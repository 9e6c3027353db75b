"""The fp64 references of tests/loss_refs.py against the oracle functions they wrap, and the input
preconditions of every parametrised case of tests/test_loss_kernels_gpu.py (assertions on the
references and generators alone: no kernel runs here, no case is skipped or filtered)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_refs as R
from oracle import expertsim_oracle as O

F64 = torch.float64


def _close(a, b, tol=1e-12):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert torch.all((a - b).abs() <= tol * b.abs().clamp(min=1.0)), (a, b)


# ------------------------------------------------------------------ agreement of the references
@pytest.mark.parametrize("case", [(2, 1, 10), (5, 64, 10), (7, 128, 70)])
def test_gen_losses_ref_equals_oracle_composition(case):
    """The generator loss of OracleMoE.train_step composed from the oracle's functions, with the
    photon sums taken from an image (4 pixels of log1p(s / 4) each)."""
    inp = R.gen_inputs(*case)
    ref = R.gen_ref_of(inp)
    n, st = case[0], R.GEN_STRENGTHS
    img = torch.log1p(inp["s"] / 4.0).view(n, 1, 1, 1).expand(n, 1, 2, 2)
    div = O.sdi_gan_regularization(inp["l1"], inp["l2"], inp["n1"], inp["n2"], inp["std"].view(n, 1), st["di"])
    il, sums, s_std, s_mean = O.intensity_regularization(img, inp["intensity"], st["ins"])
    aux = O.regressor_loss(inp["pos"], inp["coord"]) * st["aux"]
    g = -inp["fo"].mean()
    _close(sums.view(-1), inp["s"])
    _close(ref["out"], torch.stack([(g + div + il + aux) * inp["w"], g, div, il, aux, s_std, s_mean,
                                    torch.tensor(inp["w"], dtype=F64)]))


@pytest.mark.parametrize("case", [(2, 1, 10), (5, 64, 10), (257, 64, 10)])
def test_sdi_broadcast_closed_form(case):
    """The [n,1] / [n] broadcast of moe.py:573-588 equals mean(std)^2 * mean(1 / (div + 1e-5))."""
    inp = R.gen_inputs(*case)
    n = case[0]
    a = (inp["l1"], inp["l2"], inp["n1"], inp["n2"])
    inv = torch.mean(1.0 / (R.sdi_div(*a) + 1e-5))
    _close(O.sdi_gan_regularization(*a, inp["std"].view(n, 1), 0.1), inp["std"].mean() ** 2 * inv * 0.1)
    # data parallel: the global mean replaces both factors mean(std)
    _close(R.gen_ref_of(inp, std_mean=1.25)["out"][2], 1.25 ** 2 * inv * R.GEN_STRENGTHS["di"])


@pytest.mark.parametrize("B,E", [(12, 3), (300, 64)])
def test_router_ref_equals_oracle(B, E):
    """router_ref on the logits of the oracle's router_forward: same gates, same terms."""
    torch.manual_seed(5)
    P = {k: v.double() for k, v in O.build_router(9, E).items()}
    inp = R.router_inputs(B, E, R.RLOSS_TAU)
    cond = torch.randn(B, 9, dtype=F64)
    soft, logits = O.router_forward(P, cond, R.RLOSS_TAU, inp["expo"])
    ref = R.router_ref(logits, inp["expo"], inp["feat"], R.RLOSS_TAU, 3e-2, 0.1, 0.01)
    _close(ref["soft"], soft)
    idx = soft.argmax(1)
    gates = F.one_hot(idx, num_classes=E).double()
    ent, ed, alb = O.router_loss_terms(soft, gates, inp["feat"].view(B, 1),
                                       dict(util_strength=0.1, ed_strength=0.01, alb_strength=3e-2))
    _close(torch.stack([ref["alb"], ref["ent"], ref["ed"]]), torch.stack([alb, ent, ed]))
    # a term whose strength is 0 is 0 and carries no gradient
    off = R.router_ref(logits, inp["expo"], None, R.RLOSS_TAU, 0.0, 0.0, 0.0)
    assert float(off["alb"]) == float(off["ent"]) == float(off["ed"]) == 0.0 and not off["dlogits"].any()


def test_step_metrics_ref_router_loss_is_finite_at_dec_w_zero():
    """min_weight 0 at epoch 0: dec_w = 0; the reported ALB stays the unweighted value (the oracle's
    metric dict) and router_loss the sum without it."""
    m = np.arange(27, dtype=np.float64).reshape(3, 9) / 7.0
    out, _ = R.step_metrics_ref(m, [0.5, -0.25, 0.125], [3, 4, 5], 0.1, 1e-6, 0.0, 1 | 2 | 4 | 8 | 16)
    assert out[9] == 0.5 and np.isfinite(out).all()
    assert out[5] == pytest.approx(0.125 + out[10] + out[7] - 0.25, rel=1e-14)


# ------------------------------------------------------------------ input preconditions
def _margin_ok(d, exact_zeros=0):
    """Every element is an exact planted tie or at least MARGIN from the kink."""
    z = d == 0
    assert int(z.sum()) == exact_zeros, (int(z.sum()), exact_zeros)
    assert torch.all(d[~z].abs() >= R.MARGIN)


def _is_f32(*ts):
    for t in ts:
        assert t.dtype == F64 and torch.equal(t, R.f32(t))


@pytest.mark.parametrize("n", R.HINGE_N)
def test_hinge_inputs(n):
    inp = R.hinge_inputs(n)
    _is_f32(inp["ro"], inp["fo"])
    _margin_ok(1.0 - inp["ro"], 1 if n >= 5 else 0)
    _margin_ok(1.0 + inp["fo"], 1 if n >= 5 else 0)
    # the kernel's own fp32 subtraction lands on the same side
    assert torch.equal((1.0 - inp["ro"]) > 0, (1.0 - inp["ro"].float()) > 0)


@pytest.mark.parametrize("case", R.GEN_CASES + sorted({c for c, _ in R.GEN_ROWS_CASES}))
def test_gen_inputs(case):
    n, latent, noise = case
    inp = R.gen_inputs(*case)
    _is_f32(*(inp[k] for k in ("fo", "l1", "l2", "n1", "n2", "std", "s", "intensity", "coord", "pos")))
    assert 1 <= n <= 4096 and (len(inp["ties"]) > 0) == (latent >= 8)
    _margin_ok(inp["l1"] - inp["l2"], len(inp["ties"]))
    _margin_ok(inp["s"] - inp["intensity"], 0 if inp["s_tie"] is None else 1)
    for live in [n] + [lv for c, lv in R.GEN_ROWS_CASES if c == case and lv > 0]:
        div = R.sdi_div(inp["l1"][:live], inp["l2"][:live], inp["n1"][:live], inp["n2"][:live])
        assert float(div.min()) >= 1e-2
    z = -2.0 * (inp["coord"] - inp["pos"])
    assert float(z.max()) > 29.0 and float(z.min()) < -29.0       # both softplus branches


@pytest.mark.parametrize("shape", R.EXPSUM_SHAPES)
@pytest.mark.parametrize("bf16", [False, True])
def test_expsum_inputs(shape, bf16):
    x = R.expsum_inputs(shape, bf16)["x"]
    assert torch.equal(x, x.to(torch.bfloat16 if bf16 else torch.float32).to(F64))
    assert float(x.abs().max()) < 5.0


def _router_cases():
    cases = {(B, E, tau) for B, E in R.GUMBEL_CASES for tau in R.GUMBEL_TAUS}
    cases |= {(B, E, R.RLOSS_TAU) for B, E in R.COLSUM_CASES + R.ALB_CASES + R.RLOSS_CASES}
    cases |= {(2 * B, E, R.RLOSS_TAU) for B, E in R.DP_CASES}
    return sorted(cases)


@pytest.mark.parametrize("B,E,tau", _router_cases())
def test_router_inputs(B, E, tau):
    inp = R.router_inputs(B, E, tau)
    _is_f32(inp["logits"], inp["expo"], inp["feat"])
    assert E <= 64 and float(inp["expo"].min()) > 0
    soft = O.gumbel_gates(inp["logits"], inp["expo"], tau)
    assert float(soft.sum(0).min()) >= 0.5                          # every S_e
    if E > 1:
        top = soft.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= R.MARGIN     # no near-tie of the argmax
    if B > 1024:
        assert set(inp["feat"].abs().topk(2).indices.tolist()) == {1023, 1024}
    if (B // 2, E) in R.DP_CASES:                                   # both halves hold every S_e share
        assert soft.shape[0] == B and B % 2 == 0
