"""fp64 CPU references of the loss, router and step-plan kernels (csrc/loss.hip, the step plumbing of
csrc/misc.hip) and the seeded inputs of their tests.

References are the reference project's own expressions on float64 tensors with gradients from
autograd -- never the kernels' closed forms.  Where oracle/expertsim_oracle.py states an expression
it is called here, so the tree holds one statement of it.  The step plumbing (metric dict, expert
plan, gathers, metric merge) is restated in numpy float64.

Inputs are drawn in fp64 from a seeded generator and rounded to fp32 before either side sees them.
Kinks and ties are constructed, not filtered: an element closer than MARGIN to a kink is moved to
PUSH past it on its own side, planted exact ties stay exact (tests/test_loss_refs_cpu.py asserts
all of it for every parametrised case of tests/test_loss_kernels_gpu.py).
"""
from __future__ import annotations

import functools
import math
import warnings

import numpy as np
import torch
import torch.nn.functional as F

from oracle import expertsim_oracle as O

F64 = torch.float64
MARGIN, PUSH = 1e-3, 2e-3
TOL = 1e-5                      # x sum|terms| for scalars, x max|ref| for gradient arrays


def ed_tol(b_all):
    """Relative bound of the ED pair sums: one serial fp32 chain of b_all non-negative terms."""
    return max(TOL, b_all * 2.0 ** -24)


# ---------------------------------------------------------------------------------- the cases
HINGE_N = [1, 5, 256, 257, 1000]
EXPSUM_SHAPES = [(3, 1, 5, 7), (2, 1, 56, 30), (2, 1, 44, 44), (3, 2, 6, 5)]
GEN_CASES = [(1, 64, 10), (2, 1, 10), (3, 65, 10), (5, 64, 10), (7, 128, 70), (257, 64, 10), (4096, 64, 10)]
GEN_ROWS_CASES = [((7, 128, 70), 0), ((7, 128, 70), 6), ((8, 64, 10), 5)]     # (capacity case, live)
GUMBEL_CASES = [(1, 1), (255, 2), (256, 5), (257, 5), (1000, 64)]
GUMBEL_TAUS = [0.5, 1.0, 2.3]
COLSUM_CASES = [(1, 1), (257, 5), (3000, 64)]
ALB_CASES = [(7, 2), (257, 5), (1000, 64)]
RLOSS_CASES = [(7, 2), (12, 3), (1023, 5), (1025, 5), (2100, 8), (300, 64)]
RLOSS_TERMS = {"alb": (3e-2, 0.0, 0.0), "ent": (0.0, 0.1, 0.0), "ed": (0.0, 0.0, 0.01),
               "all": (3e-2, 0.1, 0.01)}                                       # (alb_coef, util, ed)
RLOSS_TAU, RLOSS_DEC_W = 0.9, 0.2
DP_CASES = [(6, 3), (600, 5)]                                                  # (B per half, E)
GEN_STRENGTHS = dict(di=0.1, ins=0.05, aux=0.5)
GEN_W = float(np.float32(0.37))


def f32(x):
    """Round to fp32, keep as fp64: what both the kernel and the reference see."""
    return x.to(torch.float32).to(F64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def push_off(d):
    """Elements of d closer than MARGIN to the kink at 0 move to +-PUSH on their own side."""
    side = torch.where(d >= 0, torch.full_like(d, PUSH), torch.full_like(d, -PUSH))
    return torch.where(d.abs() < MARGIN, side, d)


# ---------------------------------------------------------------------------------- hinge D
@functools.lru_cache(maxsize=None)
def hinge_inputs(n, seed=11):
    g = _gen(seed)
    ro, fo = f32(_randn(g, n) * 1.5), f32(_randn(g, n) * 1.5)
    ro = f32(1.0 - push_off(1.0 - ro))
    fo = f32(push_off(1.0 + fo) - 1.0)
    if n >= 5:                       # exactly at the kinks: gradient 0 on both sides
        ro[1], fo[2] = 1.0, -1.0
    return dict(ro=ro, fo=fo, w=GEN_W)


def hinge_d_ref(ro, fo, w):
    """moe.py:518-523.  -> (loss, dro, dfo, sum|terms|)."""
    ro, fo = ro.detach().clone().requires_grad_(True), fo.detach().clone().requires_grad_(True)
    loss = (F.relu(1.0 - ro).mean() + F.relu(1.0 + fo).mean()) * w
    dro, dfo = torch.autograd.grad(loss, [ro, fo])
    return loss.detach(), dro, dfo, loss.detach().abs()


# ---------------------------------------------------------------------------------- photon sums
@functools.lru_cache(maxsize=None)
def expsum_inputs(shape, bf16=False, seed=23):
    g = _gen(seed)
    n = shape[0]
    x = _randn(g, *shape) * 0.7
    x = x.to(torch.bfloat16).to(F64) if bf16 else f32(x)
    return dict(x=x, coef=f32(_randn(g, n)), dx0=f32(_randn(g, *shape)))


def expsum_ref(x):
    """-> (s [n], sum|terms| [n])."""
    return O.photon_sums(x).sum(1), (torch.exp(x) - 1).abs().sum(dim=[1, 2, 3])


def expsum_bwd_ref(x, coef, dx0, beta):
    x = x.detach().clone().requires_grad_(True)
    (dx,) = torch.autograd.grad((O.photon_sums(x).sum(1) * coef).sum(), [x])
    return beta * dx0 + dx


# ---------------------------------------------------------------------------------- generator losses
@functools.lru_cache(maxsize=None)
def gen_inputs(n, latent, noise, seed=37):
    g = _gen(seed + n + 7 * latent)
    l2 = f32(_randn(g, n, latent))
    d = _randn(g, n, latent)
    if latent < 8:                   # a short latent: keep mean|l1 - l2| (and so div_b) away from 0
        d = torch.where(d >= 0, d.clamp(min=0.25), d.clamp(max=-0.25))
    l1 = f32(l2 + push_off(d))
    l1 = f32(l2 + push_off(l1 - l2))            # the margin holds after rounding too
    ties = []
    if latent >= 8:                  # l1 == l2: sign 0, gradient exactly 0
        ties = sorted({(0, 0), (n // 2, 3), (n - 1, latent - 1)})
        for b, k in ties:
            l1[b, k] = l2[b, k]
    n1, n2 = f32(_randn(g, n, noise)), f32(_randn(g, n, noise))
    std = f32(0.5 + 1.5 * _rand(g, n))
    intensity = f32(5.0 + 45.0 * _rand(g, n))
    s = f32(intensity + push_off(_randn(g, n) * 5.0))
    s = f32(intensity + push_off(s - intensity))
    s_tie = n // 2 if n >= 3 else None
    if s_tie is not None:            # s == intensity: coef exactly 0
        s[s_tie] = intensity[s_tie]
    pos = f32(_randn(g, n, 2))
    coord = f32(pos + _randn(g, n, 2))
    if n >= 2:                       # both softplus branches: z = -2 d = -+30
        coord[0] = f32(pos[0] + 15.0)
        coord[n - 1] = f32(pos[n - 1] - 15.0)
    else:
        coord[0, 0], coord[0, 1] = f32(pos[0, 0] + 15.0), f32(pos[0, 1] - 15.0)
    fo = f32(0.5 + _randn(g, n))
    return dict(fo=fo, l1=l1, l2=l2, n1=n1, n2=n2, std=std, s=s, intensity=intensity, coord=coord, pos=pos,
                w=GEN_W, ties=ties, s_tie=s_tie)


def sdi_div(l1, l2, n1, n2):
    """div_b of moe.py:573-580 (the precondition div_b >= 1e-2 is on this)."""
    return torch.mean(torch.abs(l1 - l2), dim=1) / (torch.mean(torch.abs(n1 - n2), dim=1) + 1e-5)


def gen_losses_ref(fo, l1, l2, n1, n2, std, s, intensity, coord, pos, w, di, ins, aux, std_mean=None):
    """moe.py:544-563: total = (-fo.mean() + SDI + intensity L1 + aux * regressor_loss) * w.  std is
    shaped [n, 1] so that the reference's [n,1] / [n] broadcast is kept; std_mean (data parallel)
    replaces both factors mean(std).  -> dict: out [8], scale [8] (sum|terms| of each scalar), and
    d total / d (fo, l1, l2, coord, s); the kernel's coef is d total / d s."""
    n = fo.shape[0]
    fo, l1, l2, coord, s = (t.detach().clone().requires_grad_(True) for t in (fo, l1, l2, coord, s))
    std_col = std.view(n, 1) if std_mean is None else torch.full((n, 1), float(std_mean), dtype=F64)
    gen = -fo.mean()
    div = O.sdi_gan_regularization(l1, l2, n1, n2, std_col, di)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # n = 1: std() is NaN, like torch.std
        inl, _, s_std, s_mean = O.intensity_terms(s.view(n, 1), intensity, ins)
    auxl = O.regressor_loss(pos, coord) * aux
    total = (gen + div + inl + auxl) * w
    dfo, dl1, dl2, dcoord, ds = torch.autograd.grad(total, [fo, l1, l2, coord, s])
    dd = (coord - pos).detach()
    aux_scale = aux * torch.mean(dd.abs() + F.softplus(-2.0 * dd) + math.log(2.0))
    out = torch.stack([total, gen, div, inl, auxl, s_std, s_mean, torch.tensor(w, dtype=F64)]).detach()
    scale = torch.stack([(gen.abs() + div.abs() + inl.abs() + auxl.abs()) * w, fo.detach().abs().mean(),
                         div.abs(), inl.abs(), aux_scale, s_std.abs(), s.detach().abs().mean(),
                         torch.tensor(0.0, dtype=F64)]).detach()
    return dict(out=out, scale=scale, dfo=dfo, dl1=dl1, dl2=dl2, dcoord=dcoord, coef=ds)


def gen_ref_of(inp, live=None, std_mean=None):
    """gen_losses_ref on the first `live` rows of gen_inputs' dict."""
    k = inp["fo"].shape[0] if live is None else live
    a = {name: inp[name][:k] for name in ("fo", "l1", "l2", "n1", "n2", "std", "s", "intensity", "coord", "pos")}
    return gen_losses_ref(w=inp["w"], std_mean=std_mean, **a, **GEN_STRENGTHS)


# ---------------------------------------------------------------------------------- router
@functools.lru_cache(maxsize=None)
def router_inputs(B, E, tau, seed=53):
    """logits, Exp(1) draws and ED features.  Constructed: row e (e < E) gives expert e a soft gate of
    0.6, so every S_e >= 0.5 (the condition number 1/S_e of exp(1/S_e) does not set the error); a
    top-2 gate gap below MARGIN is widened to PUSH by raising the winner's logit; with more than
    1024 rows the two largest |feat| sit at rows 1023 and 1024 (the ED kernel's tile boundary)."""
    g = _gen(seed + B + 131 * E)
    logits = f32(_randn(g, B, E))
    expo = f32(torch.empty(B, E, dtype=F64).exponential_(generator=g).clamp(min=1e-6))
    if E > 1:
        z = (logits - expo.log()) / tau
        for e in range(min(E, B)):
            others = torch.cat([z[e, :e], z[e, e + 1:]])
            logits[e, e] += tau * (torch.logsumexp(others, 0) + math.log(1.5) - z[e, e])
        logits = f32(logits)
        for _ in range(2):           # the second pass sees the first one's fp32 rounding
            soft = O.gumbel_gates(logits, expo, tau)
            top = soft.topk(2, dim=1)
            p1, p2 = top.values[:, 0], top.values[:, 1]
            a = (PUSH * (1.0 - p1) + p2) / (p1 * (1.0 - PUSH))        # gap(a) = PUSH, a = exp(dlogit / tau)
            bump = torch.where(p1 - p2 < MARGIN, tau * a.log(), torch.zeros_like(a))
            logits = f32(logits.scatter_add(1, top.indices[:, :1], bump.view(-1, 1)))
    feat = f32(30.0 * _rand(g, B))
    if B > 1024:
        feat[1023], feat[1024] = 500.0, 400.0
    return dict(logits=logits, expo=expo, feat=feat)


def router_ref(logits, expo, feat, tau, alb_coef, util, ed, dec_w=1.0):
    """Router forward tail (routers/router.py:23, moe.py:97-103) and the router-loss terms with
    gradient (the oracle's router_loss_terms; ALB weighted by dec_w in the loss, moe.py:424-434).
    -> dict: soft, idx, counts, alb (unweighted), ent, ed, dlogits = d(dec_w*alb + ent + ed)/d logits."""
    B, E = logits.shape
    logits = logits.detach().clone().requires_grad_(True)
    soft = O.gumbel_gates(logits, expo, tau)
    idx = soft.argmax(dim=1)
    gates = F.one_hot(idx, num_classes=E).to(F64) + (soft - soft.detach())
    rc = dict(util_strength=util, ed_strength=ed, alb_strength=alb_coef)
    ent, edv, alb = O.router_loss_terms(soft, gates, None if feat is None else feat.view(B, 1), rc)
    total = dec_w * alb + ent + edv
    dlogits = (torch.autograd.grad(total, [logits])[0] if total.requires_grad
               else torch.zeros(B, E, dtype=F64))
    return dict(soft=soft.detach(), idx=idx, counts=torch.bincount(idx, minlength=E),
                alb=alb.detach().to(F64), ent=ent.detach().to(F64), ed=edv.detach().to(F64), dlogits=dlogits)


# ---------------------------------------------------------------------------------- step plumbing
def step_metrics_ref(mbuf, rl, counts, gan_strength, diff_strength, dec_w, flags):
    """The metric dict of moe.py:480-502 (the oracle's `metrics`) from the per-expert rows mbuf [E][9]
    = total, gen, div, int, aux, std_int, mean_int, w, disc and the router terms rl = [ALB, entropy,
    ED] (moe.py:255-442).  flags: 1 router, 2 trained, 4 ALB, 8 entropy, 16 ED.  -> (out, sum|terms|)."""
    m = np.asarray(mbuf, dtype=np.float64)
    E = m.shape[0]
    out, scale = np.zeros(11 + 8 * E), np.zeros(11 + 8 * E)
    for k, col in enumerate((0, 8, 2, 3, 4)):
        out[k], scale[k] = m[:, col].mean(), np.abs(m[:, col]).mean()
    if flags & 1:
        gan = out[0] * gan_strength
        dli = sum(abs(m[a, 6] - m[b, 6]) for a in range(E) for b in range(a + 1, E)) * diff_strength
        diff = -dli * diff_strength if diff_strength != 0 else 0.0
        alb = float(rl[0]) if flags & 4 else 0.0
        ent = float(rl[1]) if flags & 8 else 0.0
        ed = float(rl[2]) if flags & 16 else 0.0
        terms = (ed, gan, diff, ent, dec_w * alb)
        out[5] = sum(terms) if flags & 2 else 0.0
        scale[5] = abs(ed) + scale[0] * abs(gan_strength) + abs(diff) + abs(ent) + abs(dec_w * alb)
        out[6:11] = ed, diff, ent, alb, gan
        scale[6:11] = abs(ed), abs(diff), abs(ent), abs(alb), scale[0] * abs(gan_strength)
    for e in range(E):
        out[11 + 8 * e:19 + 8 * e] = (m[e, 0], m[e, 8], m[e, 2], m[e, 3], m[e, 4], m[e, 5], m[e, 6], counts[e])
    return out, scale


def expert_plan_ref(counts_all, rank, B, min_local):
    """moe.py:97-135 as a plan: counts_all [world][E] int.  -> rows, active, n0 (int32), w, gcnt, lcnt
    (fp32).  An expert trains when its global count > 1; this rank runs it with >= min_local rows."""
    c = np.asarray(counts_all, dtype=np.int64)
    g, loc = c.sum(0), c[rank]
    active = (g > 1).astype(np.int32)
    rows = np.where((active == 1) & (loc >= min_local), loc, 0).astype(np.int32)
    n0 = c[:rank].sum(0).astype(np.int32)
    w = loc.astype(np.float32) / np.float32(B)
    return rows, active, n0, w, g.astype(np.float32), rows.astype(np.float32)


def gather_rows_ref(src, idx, rows, cols, live=None):
    """dst[r, :cols] = src[idx[r], :cols] for r < live, zeros past it (idx None: identity)."""
    dst = np.zeros((rows, cols), dtype=src.dtype)
    k = rows if live is None else live
    ix = np.arange(k) if idx is None else np.asarray(idx[:k])
    dst[:k] = src[ix, :cols]
    return dst


def scatter_rows_ref(dst, src, idx, n, live=None):
    """dst[idx[i]] = src[i] for i < live (idx None: identity); nothing past it."""
    dst = dst.copy()
    k = n if live is None else live
    ix = np.arange(k) if idx is None else np.asarray(idx[:k])
    dst[ix] = src[:k]
    return dst


def dp_merge_case(counts, seed=71):
    """Metric rows of `world` ranks for one expert each column of counts ([world][E] samples), built
    from per-sample draws, and the global-batch row they merge to: totals / w / disc average over
    the ranks, per-sample means are the mean over all samples, std_int / mean_int are those of the
    concatenated photon sums (0 with fewer than 2 / 1 samples).  A rank with one sample carries
    std_int = NaN, as es_gen_losses writes it.  -> rows fp32 [world][E][10], out fp64 [E][9]."""
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    world, E = counts.shape
    rows = np.zeros((world, E, 10), dtype=np.float32)
    out = np.zeros((E, 9))
    for e in range(E):
        per, ssum = [], []
        for r in range(world):
            n = int(counts[r, e])
            rows[r, e, [0, 7, 8]] = rng.normal(size=3) if n else 0.0
            rows[r, e, 9] = n
            if n == 0:
                continue
            per.append(rng.normal(size=(n, 4)))
            ssum.append(rng.uniform(5.0, 50.0, size=n).astype(np.float32).astype(np.float64))
            rows[r, e, 1:5] = per[-1].mean(0)
            rows[r, e, 5] = ssum[-1].std(ddof=1) if n > 1 else np.nan
            rows[r, e, 6] = ssum[-1].mean()
        out[e, [0, 7, 8]] = rows[:, e, [0, 7, 8]].astype(np.float64).mean(0)
        N = int(counts[:, e].sum())
        if N:
            # from the fp32 rank means the kernel is given (they are its inputs)
            out[e, 1:5] = sum(rows[r, e, 1:5].astype(np.float64) * counts[r, e] for r in range(world)) / N
            alls = np.concatenate(ssum)
            out[e, 6] = alls.mean()
            out[e, 5] = alls.std(ddof=1) if N > 1 else 0.0
    return rows, out
