"""Loss, router and step-plan kernels (csrc/loss.hip, step plumbing of csrc/misc.hip), each C entry
point called through hip.call on device tensors and compared with the fp64 references of
tests/loss_refs.py (autograd of the reference's expressions; inputs and their preconditions are
checked in tests/test_loss_refs_cpu.py).

Bounds (derived, not tuned): the kernels are fp32 with block reductions of at most 16 serial adds
per thread, 6 shuffle levels and at most 16 wave partials: <= 38 roundings, 38 * 2^-24 ~ 2.3e-6 of
sum|terms|, plus a few ulp per expf / logf / log1pf.  Every scalar is held to 1e-5 * sum|terms|,
every gradient array to 1e-5 * max|ref|.  The ED pair sums are one serial chain of B_all
non-negative terms per thread: out[2] and ED-bearing dlogits are held to max(1e-5, B_all * 2^-24)
relative.  Integer and index results, copies and planted ties (gradient exactly 0) are exact.

Largest error measured on an MI355X over all cases, absolute and as a fraction of its bound (every
check prints its figure as `[maxerr] name err=... ratio=...` before it asserts):
  kernel / quantity                bound                         max err    err / bound
  es_hinge_d out, dro, dfo         1e-5 sum|terms|, max|ref|     7.2e-08    0.008
  es_image_expsum s                1e-5 sum|exp(x)-1|            4.2e-05    0.005
  es_image_expsum_bwd dx           1e-5 max|ref|                 1.1e-06    0.009
  es_gen_losses out[0..6]          1e-5 sum|terms|               1.9e-06    0.016 (div)
  es_gen_losses dfo, coef          1e-5 max|ref|                 1.6e-09    0.004
  es_gen_losses dl1, dl2           1e-5 max|ref|                 3.0e-08    0.027
  es_gen_losses dcoord             1e-5 max|ref|                 1.4e-09    0.020
  es_router_gumbel gates           1e-5 max|ref|                 7.7e-07    0.077
  es_router_gumbel row sums        1e-5                          8.0e-07    0.080
  es_router_colsum                 1e-5 S_e                      4.9e-06    0.010
  es_router_alb out / dlogits      1e-5 |ref| / max|ref|         1.9e-10    0.015 / 0.171
  es_router_loss out[0], out[1]    1e-5 |ref|                    2.6e-08    0.015
  es_router_loss out[2] (ED)       max(1e-5, B_all 2^-24) |ref|  4.0e-07    0.003
  es_router_loss dlogits, no ED    1e-5 max|ref|                 4.1e-10    0.982 (entropy alone)
  es_router_loss dlogits, ED       max(1e-5, B_all 2^-24) max|ref|  1.9e-08  0.101
  es_step_metrics out[0..10]       1e-5 sum|terms|               6.0e-08    0.007
  es_dp_metrics_merge              1e-5 max(|ref|, max|rows|)    7.0e-07    0.004
  es_div_by                        3 * 2^-24 |ref|               1.3e-08    0.281
The one figure near its bound: with the entropy (or ALB) term alone, d loss / d gates is nearly the
same for every expert, and dlogits = gates * (dG - <gates, dG>) / tau cancels that common part, so
the fp32 rounding of dG (6e-8 relative) shows at ~1e-2 of dG.  One shape gives 0.98, the others
0.2 - 0.75; the kernel is deterministic, so each figure is one fixed number.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import loss_refs as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SENT = 777.25            # finite sentinel: what a kernel must not write keeps it
NAN = float("nan")


def _hip():
    from expertsim import hip
    hip.lib()
    return hip


def dev(t, dtype=torch.float32):
    return t.detach().to(dtype).contiguous().to(DEV)


def i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).to(DEV)


def full(shape, value=SENT, dtype=torch.float32):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=DEV)


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().to(F64) if t.is_floating_point() else t.detach().cpu()


def check(name, got, ref, bound):
    """max|got - ref| <= bound (bound a scalar or elementwise); prints the figure before asserting."""
    got, ref = torch.as_tensor(got, dtype=F64), torch.as_tensor(ref, dtype=F64)
    bound = torch.as_tensor(bound, dtype=F64).expand_as(ref)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert not torch.isnan(got).any(), f"{name}: NaN in the result"
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), (err > 0).to(F64) * 1e30)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"[maxerr] {name} err={float(err.max()) if err.numel() else 0.0:.3e} ratio={worst:.3f}")
    assert worst <= 1.0, f"{name}: error {float(err.max()):.3e} is {worst:.2f} x its bound"


def with_nan_past(t, live):
    """Device fp32 copy of t whose rows past `live` are NaN (they must not be read)."""
    d = dev(t)
    d[live:] = NAN
    return d


def eff_live(live, n):
    return n if live is None else max(0, min(int(live), n))


# ------------------------------------------------------------------------------------ es_hinge_d
@pytest.mark.parametrize("n", R.HINGE_N)
@pytest.mark.parametrize("live", [None, 0, "partial", "over", -2])
def test_hinge_d(n, live):
    hip = _hip()
    live = {"partial": max(1, n - 3), "over": n + 5}.get(live, live)
    k = eff_live(live, n)
    inp = R.hinge_inputs(n)
    ro, fo = with_nan_past(inp["ro"], k), with_nan_past(inp["fo"], k)
    rows = None if live is None else i32([live])
    w, out, dro, dfo = dev(torch.tensor([inp["w"]])), full(1), full(n), full(n)
    hip.call("es_hinge_d", hip.ptr(ro), hip.ptr(fo), n, hip.ptr(rows), hip.ptr(w), hip.ptr(out), hip.ptr(dro),
             hip.ptr(dfo), hip.stream_ptr())
    out, dro, dfo = host(out), host(dro), host(dfo)
    assert torch.all(dro[k:] == SENT) and torch.all(dfo[k:] == SENT)
    if k == 0:
        assert float(out) == 0.0
        return
    loss, rdro, rdfo, scale = R.hinge_d_ref(inp["ro"][:k], inp["fo"][:k], inp["w"])
    check("hinge_d out", out[0], loss, R.TOL * scale)
    check("hinge_d dro", dro[:k], rdro, R.TOL * rdro.abs().max())
    check("hinge_d dfo", dfo[:k], rdfo, R.TOL * rdfo.abs().max())
    if n >= 5 and k > 2:        # exactly at the kinks
        assert float(dro[1]) == 0.0 and float(dfo[2]) == 0.0


def test_hinge_d_without_gradients():
    hip = _hip()
    n = 257
    inp = R.hinge_inputs(n)
    w, out, ro, fo = dev(torch.tensor([inp["w"]])), full(1), dev(inp["ro"]), dev(inp["fo"])
    hip.call("es_hinge_d", hip.ptr(ro), hip.ptr(fo), n, None, hip.ptr(w), hip.ptr(out),
             None, None, hip.stream_ptr())
    loss, _, _, scale = R.hinge_d_ref(inp["ro"], inp["fo"], inp["w"])
    check("hinge_d out", host(out)[0], loss, R.TOL * scale)


# ------------------------------------------------------------------------ es_image_expsum (_bwd)
def _image(t, layout, dtype=torch.float32, fill=None):
    """Device storage of the logical NCHW tensor t in `layout` -> (storage, hip.View without rows)."""
    hip = _hip()
    n, c, h, w = t.shape
    if layout == "nhwc":
        st = dev(t.permute(0, 2, 3, 1), dtype)
        strides = (h * w * c, 1, w * c, c)
    else:
        st = dev(t, dtype)
        strides = (c * h * w, h * w, w, 1)
    if fill is not None:
        st[fill:] = NAN
    return st, hip.make_view((n, c, h, w), strides, sample=False)


def _logical(st, layout):
    return host(st).permute(0, 3, 1, 2) if layout == "nhwc" else host(st)


@pytest.mark.parametrize("shape", R.EXPSUM_SHAPES)
@pytest.mark.parametrize("layout", ["nchw", "nhwc", "bf16"])
@pytest.mark.parametrize("live", [None, "partial"])
def test_image_expsum(shape, layout, live):
    hip = _hip()
    n = shape[0]
    bf = layout == "bf16"
    x = R.expsum_inputs(shape, bf)["x"]
    k = n if live is None else n - 1
    st, view = _image(x, "nchw" if bf else layout, torch.bfloat16 if bf else torch.float32, fill=k)
    rows = None if live is None else i32([k])
    view.rows = None if rows is None else rows.data_ptr()
    s = full(n)
    hip.call("es_image_expsum", C.byref(view), hip.dt_of(st), hip.ptr(st), hip.ptr(s), hip.stream_ptr())
    s = host(s)
    ref, scale = R.expsum_ref(x[:k])
    assert torch.all(s[k:] == SENT)
    check(f"image_expsum {layout}", s[:k], ref, R.TOL * scale)


@pytest.mark.parametrize("shape", R.EXPSUM_SHAPES)
@pytest.mark.parametrize("layouts", [("nchw", "nhwc"), ("nhwc", "nchw"), ("bf16", "nhwc")])
@pytest.mark.parametrize("rows_on", [None, "x", "dx"])
def test_image_expsum_bwd(shape, layouts, rows_on):
    hip = _hip()
    n = shape[0]
    bf = layouts[0] == "bf16"
    inp = R.expsum_inputs(shape, bf)
    k = n if rows_on is None else n - 1
    rows = None if rows_on is None else i32([k])
    for beta in (0.0, 1.0):
        xs, xv = _image(inp["x"], "nchw" if bf else layouts[0], torch.bfloat16 if bf else torch.float32, fill=k)
        ds, dv = _image(inp["dx0"], layouts[1])
        if rows_on == "x":
            xv.rows = rows.data_ptr()
        if rows_on == "dx":
            dv.rows = rows.data_ptr()
        coef = with_nan_past(inp["coef"], k)
        hip.call("es_image_expsum_bwd", C.byref(xv), hip.dt_of(xs), hip.ptr(xs), hip.ptr(coef), C.byref(dv),
                 hip.ptr(ds), beta, hip.stream_ptr())
        got = _logical(ds, layouts[1])
        ref = R.expsum_bwd_ref(inp["x"][:k], inp["coef"][:k], inp["dx0"][:k], beta)
        assert torch.equal(got[k:], inp["dx0"][k:])                  # past the live count: untouched
        check(f"image_expsum_bwd beta={beta:g}", got[:k], ref, R.TOL * ref.abs().max())


# ------------------------------------------------------------------------------------ es_gen_losses
@functools.lru_cache(maxsize=None)
def _gen_ref(case, live, std_mean):
    return R.gen_ref_of(R.gen_inputs(*case), live, std_mean)


def _run_gen_losses(case, live=None, std_mean=None, n_arg=None):
    """-> dict of host results.  Every output has its full documented size and a sentinel fill."""
    hip = _hip()
    n, latent, noise = case
    inp = R.gen_inputs(*case)
    k = eff_live(live, n)
    names = ("fo", "l1", "l2", "n1", "n2", "std", "s", "intensity", "coord", "pos")
    a = {name: with_nan_past(inp[name], k) for name in names}
    rows = None if live is None else i32([live])
    smean = None if std_mean is None else dev(torch.tensor([std_mean]))
    p = hip.GenLoss()
    p.n, p.latent, p.noise = n if n_arg is None else n_arg, latent, noise
    p.di_strength, p.in_strength, p.aux_strength = (R.GEN_STRENGTHS[x] for x in ("di", "ins", "aux"))
    p.std_mean = None if smean is None else smean.data_ptr()
    p.rows = None if rows is None else rows.data_ptr()
    w = dev(torch.tensor([inp["w"]]))
    o = dict(out=full(8), dfo=full(n), dl1=full((n, latent)), dl2=full((n, latent)), dcoord=full((n, 2)),
             coef=full(n))
    hip.call("es_gen_losses", C.byref(p), *(hip.ptr(a[x]) for x in ("fo", "l1", "l2", "n1", "n2", "std", "s",
                                                                    "intensity", "coord", "pos")),
             hip.ptr(w), *(hip.ptr(o[x]) for x in ("out", "dfo", "dl1", "dl2", "dcoord", "coef")), hip.stream_ptr())
    return {x: host(t) for x, t in o.items()}


def _check_gen(case, live, std_mean, tag):
    n = case[0]
    inp = R.gen_inputs(*case)
    k = eff_live(live, n)
    got = _run_gen_losses(case, live, std_mean)
    for x in ("dfo", "dl1", "dl2", "dcoord", "coef"):
        assert torch.all(got[x][k:] == SENT), f"{x}: rows past the live count were written"
    if k == 0:
        assert torch.all(got["out"] == 0.0)
        return
    ref = _gen_ref(case, None if live is None else k, std_mean)
    out, rout = got["out"], ref["out"]
    if k == 1:                  # like torch.std of one sample
        assert torch.isnan(out[5]) and torch.isnan(rout[5])
        out, rout = out.clone(), rout.clone()
        out[5] = rout[5] = 0.0
    names = ("total", "gen", "div", "int", "aux", "std_int", "mean_int", "w")
    for j, nm in enumerate(names[:7]):
        check(f"gen_losses out[{j}] {nm}{tag}", out[j], rout[j], R.TOL * torch.nan_to_num(ref["scale"][j]))
    assert float(out[7]) == float(np.float32(inp["w"]))
    for x in ("dfo", "dl1", "dl2", "dcoord", "coef"):
        check(f"gen_losses {x}{tag}", got[x][:k], ref[x], R.TOL * ref[x].abs().max())
    for b, c in inp["ties"]:    # l1 == l2: gradient exactly 0
        if b < k:
            assert float(got["dl1"][b, c]) == 0.0 and float(got["dl2"][b, c]) == 0.0
    if inp["s_tie"] is not None and inp["s_tie"] < k:
        assert float(got["coef"][inp["s_tie"]]) == 0.0


@pytest.mark.parametrize("case", R.GEN_CASES)
@pytest.mark.parametrize("std_mean", [None, 1.25])
def test_gen_losses(case, std_mean):
    _check_gen(case, None, std_mean, "" if std_mean is None else " std_mean")


@pytest.mark.parametrize("case,live", R.GEN_ROWS_CASES)
def test_gen_losses_rows(case, live):
    _check_gen(case, live, None, " rows")


@pytest.mark.parametrize("n_arg", [0, 4097])
def test_gen_losses_rejects_n(n_arg):
    """ES_CHECK_ARG returns before any launch: HipError, outputs untouched."""
    hip = _hip()
    case = (1, 1, 1)
    n = max(n_arg, 1)
    a = full((n, 2), 0.5)
    o = dict(out=full(8), dfo=full(n), dl1=full(n), dl2=full(n), dcoord=full((n, 2)), coef=full(n))
    p = hip.GenLoss()
    p.n, p.latent, p.noise = n_arg, case[1], case[2]
    with pytest.raises(hip.HipError):
        hip.call("es_gen_losses", C.byref(p), *[hip.ptr(a)] * 10, hip.ptr(a),
                 *(hip.ptr(o[x]) for x in ("out", "dfo", "dl1", "dl2", "dcoord", "coef")), hip.stream_ptr())
    for x, t in o.items():
        assert torch.all(host(t) == SENT), x


# ------------------------------------------------------------------------------------ router
@functools.lru_cache(maxsize=None)
def _router_ref(B, E, tau, alb, util, ed, dec_w=1.0, with_feat=True):
    inp = R.router_inputs(B, E, tau)
    return R.router_ref(inp["logits"], inp["expo"], inp["feat"] if with_feat else None, tau, alb, util, ed, dec_w)


@pytest.mark.parametrize("B,E", R.GUMBEL_CASES)
@pytest.mark.parametrize("tau", R.GUMBEL_TAUS)
def test_router_gumbel(B, E, tau):
    hip = _hip()
    inp = R.router_inputs(B, E, tau)
    ref = _router_ref(B, E, tau, 0.0, 0.0, 0.0, 1.0, False)
    logits, expo = dev(inp["logits"]), dev(inp["expo"])
    for with_counts in (True, False):
        gates, idx = full((B, E)), torch.full((B,), -7, dtype=torch.int32, device=DEV)
        counts = torch.zeros(E, dtype=torch.int32, device=DEV) if with_counts else None   # atomics: zeroed
        hip.call("es_router_gumbel", hip.ptr(logits), hip.ptr(expo), B, E, tau, hip.ptr(gates), hip.ptr(idx),
                 hip.ptr(counts), hip.stream_ptr())
        g = host(gates)
        assert torch.equal(host(idx).long(), ref["idx"])
        if with_counts:
            assert torch.equal(host(counts).long(), ref["counts"])
        check("router_gumbel gates", g, ref["soft"], R.TOL * ref["soft"].abs().max())
        check("router_gumbel row sums", g.sum(1), torch.ones(B, dtype=F64), R.TOL)


@pytest.mark.parametrize("B,E", R.COLSUM_CASES)
def test_router_colsum(B, E):
    hip = _hip()
    gates32 = _router_ref(B, E, R.RLOSS_TAU, 0.0, 0.0, 0.0, 1.0, False)["soft"].float()
    out, gates = full(E), gates32.to(DEV)
    hip.call("es_router_colsum", hip.ptr(gates), B, E, hip.ptr(out), hip.stream_ptr())
    ref = gates32.double().sum(0)
    check("router_colsum", host(out), ref, R.TOL * ref)


@pytest.mark.parametrize("B,E", R.ALB_CASES)
def test_router_alb(B, E):
    hip = _hip()
    coef, tau = 3e-2, R.RLOSS_TAU
    ref = _router_ref(B, E, tau, coef, 0.0, 0.0, 1.0, False)
    out, dlogits, gates = full(1), full((B, E)), dev(ref["soft"])
    hip.call("es_router_alb", hip.ptr(gates), B, E, tau, coef, hip.ptr(out), hip.ptr(dlogits),
             hip.stream_ptr())
    check("router_alb out", host(out)[0], ref["alb"], R.TOL * ref["alb"].abs())
    check("router_alb dlogits", host(dlogits), ref["dlogits"], R.TOL * ref["dlogits"].abs().max())


def _router_loss(gates, idx, feat, B, E, tau, alb, dec_w, util, ed, colsum=None, B_total=0, feat_all=None,
                 idx_all=None, B_all=0):
    """es_router_loss with dlogits at its full [B, E] size (it is also the ED scratch)."""
    hip = _hip()
    out, dlogits = full(3), full((B, E))
    hip.call("es_router_loss", hip.ptr(gates), hip.ptr(idx), hip.ptr(feat), B, E, tau, alb, dec_w, util, ed,
             hip.ptr(colsum), B_total, hip.ptr(feat_all), hip.ptr(idx_all), B_all, hip.ptr(out), hip.ptr(dlogits),
             hip.stream_ptr())
    return host(out), host(dlogits)


def _check_router_loss(tag, out, dlogits, ref, ref_dlogits, ed_on, b_all, ed_ref=None):
    rel = R.ed_tol(b_all) if ed_on else R.TOL
    check(f"router_loss out[0] ALB{tag}", out[0], ref["alb"], R.TOL * ref["alb"].abs())
    check(f"router_loss out[1] ENT{tag}", out[1], ref["ent"], R.TOL * ref["ent"].abs())
    if ed_ref is not None:
        check(f"router_loss out[2] ED{tag}", out[2], ed_ref, R.ed_tol(b_all) * ed_ref.abs())
    check(f"router_loss dlogits{tag}" + (" (ED)" if ed_on else ""), dlogits, ref_dlogits,
          rel * ref_dlogits.abs().max())


@pytest.mark.parametrize("B,E", R.RLOSS_CASES)
@pytest.mark.parametrize("term", list(R.RLOSS_TERMS))
def test_router_loss(B, E, term):
    alb, util, ed = R.RLOSS_TERMS[term]
    tau, dec_w = R.RLOSS_TAU, R.RLOSS_DEC_W
    inp = R.router_inputs(B, E, tau)
    ref = _router_ref(B, E, tau, alb, util, ed, dec_w)
    ed_on = ed != 0.0
    gates = dev(ref["soft"])
    idx = i32(ref["idx"].numpy()) if ed_on else None          # feat / idx may be NULL without ED
    feat = dev(inp["feat"]) if ed_on else None
    out, dlogits = _router_loss(gates, idx, feat, B, E, tau, alb, dec_w, util, ed)
    _check_router_loss(f" {term}", out, dlogits, ref, ref["dlogits"], ed_on, B, ref["ed"])


def test_router_loss_dec_w_zero():
    """router.min_weight 0 at epoch 0: out[0] is the unweighted ALB (finite), no ALB gradient."""
    B, E, tau = 12, 3, R.RLOSS_TAU
    alb, util, ed = R.RLOSS_TERMS["all"]
    inp = R.router_inputs(B, E, tau)
    ref = _router_ref(B, E, tau, alb, util, ed, 0.0)
    assert float(ref["alb"]) > 0
    out, dlogits = _router_loss(dev(ref["soft"]), i32(ref["idx"].numpy()), dev(inp["feat"]), B, E, tau, alb, 0.0,
                                util, ed)
    _check_router_loss(" dec_w=0", out, dlogits, ref, ref["dlogits"], True, B, ref["ed"])
    # ALB alone at dec_w = 0: the gradient is exactly 0
    out, dlogits = _router_loss(dev(ref["soft"]), None, None, B, E, tau, alb, 0.0, 0.0, 0.0)
    check("router_loss out[0] ALB dec_w=0", out[0], ref["alb"], R.TOL * ref["alb"].abs())
    assert not dlogits.any()


@pytest.mark.parametrize("B,E", R.DP_CASES)
def test_router_loss_data_parallel_form(B, E):
    """Two halves of a global batch of 2B rows, each with the summed colsum, B_total = B_all = 2B and
    the concatenated ED features: every half's dlogits are its rows of the global autograd."""
    hip = _hip()
    alb, util, ed = R.RLOSS_TERMS["all"]
    tau, dec_w, G = R.RLOSS_TAU, R.RLOSS_DEC_W, 2 * B
    inp = R.router_inputs(G, E, tau)
    ref = _router_ref(G, E, tau, alb, util, ed, dec_w)
    gates_all, idx_all, feat_all = dev(ref["soft"]), i32(ref["idx"].numpy()), dev(inp["feat"])
    halves = [slice(0, B), slice(B, G)]
    shares = []
    for h in halves:
        cs = full(E)
        hip.call("es_router_colsum", hip.ptr(gates_all[h].contiguous()), B, E, hip.ptr(cs), hip.stream_ptr())
        shares.append(cs)
    colsum = shares[0] + shares[1]
    ed_sum = 0.0
    for r, h in enumerate(halves):
        out, dlogits = _router_loss(gates_all[h].contiguous(), idx_all[h].contiguous(), feat_all[h].contiguous(), B,
                                    E, tau, alb, dec_w, util, ed, colsum, G, feat_all, idx_all, G)
        _check_router_loss(f" dp half {r}", out, dlogits, ref, ref["dlogits"][h], True, G)
        ed_sum = ed_sum + out[2]
    check("router_loss out[2] ED dp sum", ed_sum, ref["ed"], R.ed_tol(G) * ref["ed"].abs())


@pytest.mark.parametrize("what", ["E=65", "ED without feat"])
def test_router_loss_rejects(what):
    """ES_CHECK_ARG returns before any launch: HipError, outputs untouched."""
    hip = _hip()
    B, E = (4, 65) if what == "E=65" else (4, 3)
    gates, out, dlogits = full((B, E), 1.0 / E), full(3), full((B, E))
    idx = i32(np.zeros(B))
    with pytest.raises(hip.HipError):
        hip.call("es_router_loss", hip.ptr(gates), hip.ptr(idx), None, B, E, 1.0, 1e-2, 1.0, 0.0,
                 0.0 if what == "E=65" else 0.01, None, 0, None, None, 0, hip.ptr(out), hip.ptr(dlogits),
                 hip.stream_ptr())
    assert torch.all(host(out) == SENT) and torch.all(host(dlogits) == SENT)


# ------------------------------------------------------------------------------------ step metrics
@pytest.mark.parametrize("E", [1, 3, 8])
@pytest.mark.parametrize("flags", [0, 1 | 2 | 4, 1 | 2 | 4 | 8 | 16, 1 | 4])
def test_step_metrics(E, flags):
    hip = _hip()
    rng = np.random.default_rng(100 + E)
    mbuf = rng.normal(size=(E, 9)).astype(np.float32)
    mbuf[:, 6] = rng.uniform(5.0, 50.0, size=E)
    rl = np.array([0.31, -0.12, 0.07], dtype=np.float32)
    counts = rng.integers(0, 40, size=E)
    gan_strength = 0.1
    md, rld = torch.from_numpy(mbuf).to(DEV), torch.from_numpy(rl).to(DEV)
    for as_float in (False, True):
        cnt = torch.from_numpy(counts.astype(np.float32 if as_float else np.int32)).to(DEV)
        for diff_strength in (0.0, 1e-6):
            for dec_w in (1.0, 0.2, 0.0):
                out = full(11 + 8 * E)
                hip.call("es_step_metrics", hip.ptr(md), E, hip.ptr(rld) if flags & 1 else None,
                         None if as_float else hip.ptr(cnt), hip.ptr(cnt) if as_float else None, gan_strength,
                         diff_strength, dec_w, flags, hip.ptr(out), hip.stream_ptr())
                ref, scale = R.step_metrics_ref(mbuf, rl, counts, np.float32(gan_strength),
                                                np.float32(diff_strength), np.float32(dec_w), flags)
                got = host(out)
                check(f"step_metrics dec_w={dec_w:g}", got[:11], ref[:11], R.TOL * scale[:11])
                assert np.array_equal(got[11:].numpy(), ref[11:])          # per-expert copies: exact


def test_dp_metrics_merge():
    """A rank that did not run the expert (count 0), an expert nobody ran, a total count of 1, and a
    rank with one sample (its std_int row is NaN, as es_gen_losses writes it) beside larger ranks."""
    hip = _hip()
    counts = [[3, 0, 1, 1], [0, 0, 0, 5], [4, 0, 0, 2]]
    rows, ref = R.dp_merge_case(counts)
    world, E = len(counts), len(counts[0])
    out, rd = full((E, 9)), torch.from_numpy(rows).to(DEV)
    hip.call("es_dp_metrics_merge", hip.ptr(rd), world, E, hip.ptr(out),
             hip.stream_ptr())
    scale = np.maximum(np.abs(ref), np.nanmax(np.abs(rows[:, :, :9]), axis=0))
    check("dp_metrics_merge", host(out), ref, R.TOL * torch.from_numpy(scale))
    assert ref[2, 5] == 0.0 and ref[1].tolist() == [0.0] * 9 and ref[3, 5] > 0


# ------------------------------------------------------------------------------------ expert plan
def _plan_counts(E, world):
    """Count tables [world][E]: a 0, a global count of exactly 1 (inactive) and a local count of 1
    beside an active global count (below min_local = 2)."""
    rng = np.random.default_rng(7 * E + world)
    base = rng.integers(0, 5, size=(world, E))
    tables = []
    for kind in range(3):
        c = base.copy()
        e = kind % E
        c[:, e] = 0
        if kind == 1:
            c[0, e] = 1                           # global count 1: inactive
        if kind == 2:
            c[0, e], c[world - 1, e] = 1, (3 if world > 1 else 1)
        tables.append(c)
    return tables


@pytest.mark.parametrize("E", [1, 3, 64])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_expert_plan(E, world):
    hip = _hip()
    B = 64
    for table in _plan_counts(E, world):
        call = None if world == 1 else i32(table)
        for rank in range(world):
            for min_local in (1, 2):
                ints = [torch.full((E,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
                flts = [full(E) for _ in range(3)]
                loc = i32(table[rank])
                hip.call("es_expert_plan", hip.ptr(loc), hip.ptr(call), world, rank, E, B, min_local,
                         *(hip.ptr(t) for t in ints + flts), hip.stream_ptr())
                ref = R.expert_plan_ref(table, rank, B, min_local)
                for name, got, want in zip(("rows", "active", "n0", "w", "gcnt", "lcnt"), ints + flts, ref):
                    assert np.array_equal(host(got).numpy().astype(want.dtype), want), (name, rank, min_local)


# ------------------------------------------------------------------------------------ gather / scatter
@pytest.mark.parametrize("rows", [1, 5, 300])
@pytest.mark.parametrize("cols", [1, 9, 74])
def test_gather_rows(rows, cols):
    hip = _hip()
    rng = np.random.default_rng(rows * 100 + cols)
    nsrc, sld, dld, start0 = rows + 7, cols + 3, cols + 2, 3
    src = rng.normal(size=(nsrc, sld)).astype(np.float32)
    idx = rng.integers(0, nsrc, size=rows)
    perm = np.concatenate([rng.integers(0, nsrc, size=start0), idx])
    sd, permd, startd = torch.from_numpy(src).to(DEV), i32(perm), i32([start0])
    stream = hip.stream_ptr()
    for ix in (idx, None):
        dst, ixd = full((rows, dld)), None if ix is None else i32(ix)
        hip.call("es_gather_rows", hip.ptr(sd), sld, hip.ptr(ixd), rows, cols,
                 hip.ptr(dst), dld, stream)
        got = host(dst).numpy()
        assert np.array_equal(got[:, :cols], R.gather_rows_ref(src, ix, rows, cols))
        assert np.all(got[:, cols:] == SENT)                             # padding columns
    for live in (None, rows // 2, 0, rows + 9):
        dst = full((rows, dld))
        lv = None if live is None else i32([live])
        hip.call("es_gather_rows_at", hip.ptr(sd), sld, hip.ptr(permd), hip.ptr(startd), rows, cols,
                 hip.ptr(dst), dld, hip.ptr(lv), stream)
        got = host(dst).numpy()
        assert np.array_equal(got[:, :cols], R.gather_rows_ref(src, idx, rows, cols, eff_live(live, rows)))
        assert np.all(got[:, cols:] == SENT)


@pytest.mark.parametrize("n", [1, 5, 300])
def test_scatter_rows(n):
    hip = _hip()
    rng = np.random.default_rng(n)
    ndst, start0 = n + 5, 2
    src = rng.normal(size=n).astype(np.float32)
    idx = rng.permutation(ndst)[:n]
    perm = np.concatenate([rng.integers(0, ndst, size=start0), idx])
    base = np.full(ndst, SENT, dtype=np.float32)
    sd, stream, permd, startd = torch.from_numpy(src).to(DEV), hip.stream_ptr(), i32(perm), i32([start0])
    for ix in (idx, None):
        dst, ixd = full(ndst), None if ix is None else i32(ix)
        hip.call("es_scatter_rows", hip.ptr(sd), hip.ptr(ixd), n, hip.ptr(dst), stream)
        assert np.array_equal(host(dst).numpy(), R.scatter_rows_ref(base, src, ix, n))
    for live in (None, n // 2, 0, n + 9):
        dst = full(ndst)
        lv = None if live is None else i32([live])
        hip.call("es_scatter_rows_at", hip.ptr(sd), hip.ptr(permd), hip.ptr(startd), n, hip.ptr(lv),
                 hip.ptr(dst), stream)
        assert np.array_equal(host(dst).numpy(), R.scatter_rows_ref(base, src, idx, n, eff_live(live, n)))


# ------------------------------------------------------------------------------------ small plumbing
@pytest.mark.parametrize("d", [0.0, 0.5, 1.0, 7.0])
def test_div_by(d):
    hip = _hip()
    x = R.f32(torch.randn(300, generator=torch.Generator().manual_seed(3), dtype=F64))
    xd, dd = dev(x), dev(torch.tensor([d]))
    hip.call("es_div_by", hip.ptr(xd), 300, hip.ptr(dd), hip.stream_ptr())
    ref = x / max(d, 1.0)
    check("div_by", host(xd), ref, 3.0 * 2.0 ** -24 * ref.abs())          # one fp32 division


def test_counter_add():
    hip = _hip()
    flags = {"null": None, "0": i32([0]), "1": i32([1])}
    c = i32([5])
    hip.call("es_counter_add", hip.ptr(c), 3, hip.stream_ptr())
    assert int(host(c)) == 8
    for name, f in flags.items():
        c = i32([5])
        hip.call("es_counter_add_if", hip.ptr(c), -2, hip.ptr(f), hip.stream_ptr())
        assert int(host(c)) == (5 if name == "0" else 3), name
        big = 2 ** 31 + 5
        c64 = torch.tensor([big], dtype=torch.int64, device=DEV)
        hip.call("es_counter_add_i64_if", hip.ptr(c64), 2 ** 31, hip.ptr(f), hip.stream_ptr())
        assert int(host(c64)) == (big if name == "0" else big + 2 ** 31), name
