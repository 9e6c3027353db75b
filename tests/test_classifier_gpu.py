"""es_rank_stats, es_logit_fit, es_logit_scores and expertsim.train.classifier.c2st on the device against the numpy
restatement and the scikit-learn / scipy record (tests/classifier_refs.py, whose docstring derives every bound;
tests/golden/classifier_sklearn.npz).  Every test prints its worst error-to-bound ratio before asserting.

A fit is judged without trusting the device: (a) its gradient is recomputed in numpy at the theta it returned and
must be at most gtol plus the rounding bound of two gradient evaluations; (b) its distance to the record's theta must
satisfy the convexity inequality of the docstring.  The rank statistics are integers and must be equal.
A problem is degenerate (status -1, theta NaN) when a side is EMPTY; a side of one row is an ordinary ridge problem
and is fitted."""
import numpy as np
import pytest
import torch

import classifier_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
UNITS = 4 * 2.0 ** -53
GTOL = R.GTOL


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if dtype is None else torch.tensor(x, dtype=dtype, device=DEV)


def _seg(pairs):
    return torch.tensor(pairs, dtype=torch.int32, device=DEV).reshape(-1, 2)


# ------------------------------------------------------------------------------------------ es_rank_stats
@pytest.mark.parametrize("kind", R.RANK_KINDS)
def test_rank_stats_record_cases(kind, golden):
    from expertsim import hip
    from expertsim.train.classifier import rank_stats
    assert hip.WS_LDS_MAX == 8192
    worst = 0.0
    for nu, nv in R.RANK_SIZES:
        u, v = R.rank_case(kind, nu, nv)
        out = rank_stats(_dev(u[:, None]), _dev(v[:, None]))
        again = rank_stats(_dev(u[:, None]), _dev(v[:, None]))
        got = tuple(int(x) for x in out.cpu().reshape(4))
        assert out.dtype == torch.int64 and tuple(out.shape) == (1, 1, 4) and torch.equal(out, again)
        assert got == R.rank_stats(u, v), (kind, nu, nv, got, R.rank_stats(u, v))
        ks_rec, u_rec, auc_rec = golden[f"rank_{kind}_{nu}_{nv}"]
        errs = (abs(got[3] / (nu * nv) - ks_rec), abs(got[2] / 2 - u_rec) / max(u_rec, 1.0),
                abs(got[2] / (2 * nu * nv) - auc_rec) / max(auc_rec, 1e-300))
        worst = max(worst, max(errs) / UNITS)
    print(f"rank {kind}: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_rank_stats_segments_index_stride_and_canaries():
    from expertsim.train.classifier import rank_stats
    rs = np.random.RandomState(5)
    rows_u, rows_v, ch, ld = 1500, 1400, 3, 5
    u, v = rs.randn(rows_u, ld), rs.randn(rows_v, ld) + 0.2
    u[:, 1], v[:, 1] = np.round(u[:, 1]), np.round(v[:, 1])                  # ties; some of them -0.0 against 0.0
    iu, iv = rs.permutation(rows_u).astype(np.int32), rs.permutation(rows_v).astype(np.int32)
    lens = (0, 1, 2, 63, 64, 65, 257, 1000)
    useg = [[10, 10 + L] for L in lens] + [[-5, 40], [1400, 9999], [700, 600]]          # clamped, clamped, inverted
    vseg = [[3, 3 + L] for L in reversed(lens)] + [[0, 17], [1390, 1500], [0, 50]]
    n_seg = len(useg)
    out = torch.full((n_seg + 2, ch, 4), -7, dtype=torch.int64, device=DEV)
    ut, vt = _dev(u)[:, :ch], _dev(v)[:, :ch]                               # a row stride above `channels`
    assert ut.stride(0) == ld
    got = rank_stats(ut, vt, u_idx=_dev(iu), u_seg=_seg(useg), u_cap=1000, v_idx=_dev(iv), v_seg=_seg(vseg),
                     v_cap=1000, out=out)
    host = got.cpu().numpy()
    assert (host[n_seg:] == -7).all()                                        # canary rows beyond n_seg
    for s in range(n_seg):
        (ub, ue), (vb, ve) = useg[s], vseg[s]
        ub, vb = min(max(ub, 0), rows_u), min(max(vb, 0), rows_v)
        ue, ve = min(max(ue, ub), rows_u), min(max(ve, vb), rows_v)
        for c in range(ch):
            ref = R.rank_stats(u[iu[ub:ue], c], v[iv[vb:ve], c])
            assert tuple(host[s, c]) == ref, (s, c, tuple(host[s, c]), ref)
    # a cap below a segment's length cuts it
    cut = rank_stats(ut, vt, u_seg=_seg([[0, 500]]), u_cap=100, v_seg=_seg([[0, 500]]), v_cap=64).cpu().numpy()
    assert tuple(cut[0, 0]) == R.rank_stats(u[:100, 0], v[:64, 0])
    print("rank segments: integers equal")


@pytest.mark.parametrize("nu,nv", [(700, 900), (4097, 4096), (10000, 10001)])
def test_rank_stats_leaves_wasserstein_alone(nu, nv):
    from expertsim.train.classifier import rank_stats
    from expertsim.train.utils import wasserstein_1d_device
    u, v = R.rank_case("three" if nu == 4097 else "cont", nu, nv) if (nu, nv) in R.RANK_SIZES else \
        (np.random.RandomState(1).randn(nu), np.round(np.random.RandomState(2).randn(nv), 1))
    ut, vt = _dev(u[:, None]), _dev(v[:, None])
    before = wasserstein_1d_device(ut, vt).clone()
    rk = rank_stats(ut, vt)
    after = wasserstein_1d_device(ut, vt)
    assert torch.equal(before, after) and tuple(int(x) for x in rk.cpu().reshape(4)) == R.rank_stats(u, v)
    from scipy.stats import wasserstein_distance
    ref = wasserstein_distance(u, v)
    err, bound = abs(float(after[0, 0]) - ref), 2 * (nu + nv) * 2.0 ** -52 * ref
    print(f"wasserstein around rank_stats: bit-equal, error / bound {err / bound:.3f}")
    assert err <= bound


# ------------------------------------------------------------------------------------------ es_logit_fit
def _embed(real, fake, seed):
    """The rows scattered into wider, longer tables: (real table, real idx, fake table, fake idx) on the device with a
    row stride above cols and a permuted index whose first m / k entries name the rows."""
    rs = np.random.RandomState(seed)
    out = []
    for x in (real, fake):
        n, cols = x.shape
        big = rs.randn(n + 9, cols + 3).astype(x.dtype) * 50.0
        idx = rs.permutation(n + 9).astype(np.int32)
        big[idx[:n], :cols] = x
        out += [_dev(big)[:, :cols], _dev(idx)]
    return out


def _judge(name, theta, stat, Z, y, theta_rec=None, l2=R.L2, gtol=GTOL):
    """Checks (a) and (b) of the module docstring; returns the worst error / bound ratio."""
    F, g, _ = R.objective(theta, Z, y, l2)
    gb, fb = R.grad_bound(theta, Z, l2), R.objective_bound(theta, Z, y, l2)
    ratios = {"certificate": np.abs(g).max() / (gtol + 2 * gb), "reported g": abs(stat[1] - np.abs(g).max()) / (2 * gb),
              "reported F": abs(stat[0] - F) / (2 * fb)}
    assert stat[3] == 1.0 and 1 <= stat[2] <= 30, (name, stat)
    if theta_rec is not None:
        D, bound, r = R.distance_bound(theta, theta_rec, Z, y, l2)
        ratios["distance"] = D / bound
        assert r < 1e-5, (name, r)
    worst = max(ratios.values())
    print(f"fit {name}: moves {int(stat[2])} |g| {stat[1]:.2e} " + " ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert worst <= 1.0, (name, ratios)
    return worst


@pytest.mark.parametrize("name", sorted(R.FIT_CASES))
def test_logit_fit_record_cases(name, golden):
    from expertsim import hip
    from expertsim.train.classifier import logit_fit
    assert hip.logit_block_rows() == R.block_rows()
    real, fake = R.fit_case(name)
    m, k = len(real), len(fake)
    rt, ri, ft, fi = _embed(real, fake, 7)
    args = dict(r_idx=ri, r_seg=_seg([[0, m]]), r_cap=m, f_idx=fi, f_seg=_seg([[0, k]]), f_cap=k, gtol=GTOL)
    theta, stat = logit_fit(rt, ft, **args)
    theta2, stat2 = logit_fit(rt, ft, **args)
    assert torch.equal(theta, theta2) and torch.equal(stat, stat2)           # a rerun is bit-equal
    assert rt.dtype == (torch.float32 if real.dtype == np.float32 else torch.float64)
    Z, y = R.design(real, fake)
    _judge(name, theta.cpu().numpy()[0], stat.cpu().numpy()[0], Z, y, golden[f"fit_{name}_theta"])


def test_logit_fit_segments_degenerate_and_canaries():
    from expertsim.train.classifier import logit_fit
    rs = np.random.RandomState(11)
    cols = 3
    real, fake = rs.randn(900, cols) + 0.5, rs.randn(800, cols)
    # (real bounds, generated bounds): lengths 0, 1, 2, 63, 64, 65, 257 on either side, unequal sides, clamped and
    # inverted bounds
    segs = [((0, 0), (0, 50)), ((0, 40), (5, 5)), ((7, 8), (0, 64)), ((0, 2), (2, 4)), ((10, 73), (0, 65)),
            ((100, 164), (100, 163)), ((200, 265), (300, 557)), ((300, 557), (0, 1)), ((-9, 30), (790, 5000)),
            ((50, 20), (0, 30)), ((0, 900), (0, 800))]
    n_seg = len(segs)
    theta = torch.full((n_seg + 2, cols + 1), -7.0, dtype=torch.float64, device=DEV)
    stat = torch.full((n_seg + 2, 4), -7.0, dtype=torch.float64, device=DEV)
    logit_fit(_dev(real), _dev(fake), r_seg=_seg([s[0] for s in segs]), f_seg=_seg([s[1] for s in segs]), r_cap=900,
              f_cap=800, gtol=GTOL, out=(theta, stat))
    th, st = theta.cpu().numpy(), stat.cpu().numpy()
    assert (th[n_seg:] == -7.0).all() and (st[n_seg:] == -7.0).all()        # canaries
    worst = 0.0
    for s, ((rb, re), (fb, fe)) in enumerate(segs):
        rb, fb = min(max(rb, 0), 900), min(max(fb, 0), 800)
        re, fe = min(max(re, rb), 900), min(max(fe, fb), 800)
        if re == rb or fe == fb:
            assert st[s, 3] == -1.0 and st[s, 2] == 0.0 and np.isnan(th[s]).all() and np.isnan(st[s, :2]).all(), s
            continue
        Z, y = R.design(real[rb:re], fake[fb:fe])
        worst = max(worst, _judge(f"segment {s}", th[s], st[s], Z, y))
    print(f"fit segments: worst error / bound {worst:.3g}")


def test_logit_fit_max_iter_and_l2():
    from expertsim.train.classifier import logit_fit
    real, fake = R.fit_case("c10")
    theta, stat = logit_fit(_dev(real), _dev(fake), max_iter=1, gtol=GTOL)
    st = stat.cpu().numpy()[0]
    assert st[3] == 0.0 and st[2] == 1.0 and np.isfinite(theta.cpu().numpy()).all(), st
    Z, y = R.design(real, fake)
    F, g, _ = R.objective(theta.cpu().numpy()[0], Z, y)
    assert abs(st[0] - F) <= 2 * R.objective_bound(theta.cpu().numpy()[0], Z, y) and st[0] < np.log(2.0)
    # another penalty: still the optimum of ITS objective
    theta, stat = logit_fit(_dev(real), _dev(fake), l2=25.0, gtol=GTOL)
    _judge("l2 = 25", theta.cpu().numpy()[0], stat.cpu().numpy()[0], Z, y, l2=25.0)


# ------------------------------------------------------------------------------------------ es_logit_scores
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_logit_scores(dtype):
    from expertsim.train.classifier import logit_fit, logit_scores, rank_stats
    rs = np.random.RandomState(21)
    cols = 10
    real, fake = (rs.randn(700, cols) + 0.4).astype(dtype), rs.randn(650, cols).astype(dtype)
    rseg, fseg = [(0, 300), (300, 700), (5, 5), (690, 700)], [(0, 257), (100, 650), (0, 9), (0, 3)]
    n_seg, r_cap, f_cap = len(rseg), 400, 550
    kw = dict(r_seg=_seg(rseg), f_seg=_seg(fseg), r_cap=r_cap, f_cap=f_cap)
    theta, _ = logit_fit(_dev(real), _dev(fake), gtol=GTOL, **kw)
    outs = (torch.full((n_seg + 1, r_cap), -7.0, dtype=torch.float64, device=DEV),
            torch.full((n_seg + 1, f_cap), -7.0, dtype=torch.float64, device=DEV),
            torch.full((n_seg + 1, 2), -7, dtype=torch.int32, device=DEV),
            torch.full((n_seg + 1, 2), -7, dtype=torch.int32, device=DEV),
            torch.full((n_seg + 1, 4), -7.0, dtype=torch.float64, device=DEV))
    sc = logit_scores(_dev(real), _dev(fake), theta, out=outs, **kw)
    again = logit_scores(_dev(real), _dev(fake), theta, **kw)
    th = theta.cpu().numpy()
    r_sc, f_sc, sums = sc["r_scores"].cpu().numpy(), sc["f_scores"].cpu().numpy(), sc["sums"].cpu().numpy()
    assert sc["r_seg"].cpu().tolist() == [[s * r_cap, s * r_cap + (e - b)] for s, (b, e) in enumerate(rseg)] + [[-7, -7]]
    assert sc["f_seg"].cpu().tolist() == [[s * f_cap, s * f_cap + (e - b)] for s, (b, e) in enumerate(fseg)] + [[-7, -7]]
    assert (r_sc[n_seg] == -7).all() and (f_sc[n_seg] == -7).all() and (sums[n_seg] == -7).all()
    worst = 0.0
    for s in range(n_seg):
        (rb, re), (fb, fe) = rseg[s], fseg[s]
        m, k = re - rb, fe - fb
        assert (r_sc[s, m:] == -7).all() and (f_sc[s, k:] == -7).all()      # nothing past a segment's length
        assert np.array_equal(again["r_scores"].cpu().numpy()[s, :m], r_sc[s, :m])
        assert np.array_equal(again["sums"].cpu().numpy()[s], sums[s], equal_nan=True)
        if m == 0 or k == 0:
            assert np.isnan(th[s]).all() and np.isnan(r_sc[s, :m]).all() and np.isnan(f_sc[s, :k]).all()
            continue
        Zr, Zf = R.design(real[rb:re], fake[:0])[0], R.design(fake[fb:fe], real[:0])[0]
        for Zs, got, hit, loss_fn, col in ((Zr, r_sc[s, :m], lambda t: t > 0, lambda t: R.softplus(-t), 0),
                                           (Zf, f_sc[s, :k], lambda t: t <= 0, R.softplus, 1)):
            ref, bound = Zs @ th[s], 2 * R.score_bound(th[s], Zs)
            worst = max(worst, (np.abs(got - ref) / bound).max())
            sure = np.abs(ref) > bound                                        # no reference score within the bound of 0
            if sure.all():
                assert sums[s, col] == hit(ref).sum(), (s, col)
            assert hit(ref[sure]).sum() <= sums[s, col] <= hit(ref[sure]).sum() + (~sure).sum()
            loss = loss_fn(ref)
            worst = max(worst, abs(sums[s, 2 + col] - loss.sum()) / (2 * R.logloss_bound(th[s], Zs, loss)))
    print(f"scores {np.dtype(dtype).name}: worst error / bound {worst:.3g}")
    assert worst <= 1.0
    # the layout reads back as segments: the ranks of the scores, no length on the host
    rk = rank_stats(sc["r_scores"][:n_seg].reshape(-1, 1), sc["f_scores"][:n_seg].reshape(-1, 1),
                    u_seg=sc["r_seg"][:n_seg], v_seg=sc["f_seg"][:n_seg], u_cap=r_cap, v_cap=f_cap).cpu().numpy()
    for s in range(n_seg):
        m, k = rseg[s][1] - rseg[s][0], fseg[s][1] - fseg[s][0]
        ref = R.rank_stats(r_sc[s, :m], f_sc[s, :k]) if m and k else (m, k, 0, 0)
        assert tuple(rk[s, 0]) == ref


# ------------------------------------------------------------------------------------------ c2st
@pytest.mark.parametrize("name", sorted(R.C2ST_CASES))
def test_c2st_against_the_record(name, golden):
    from expertsim.train.classifier import KEYS, c2st
    real, fake, expert, E, degree = R.c2st_case(name)
    N = len(real)
    ex = None if expert is None else _dev(expert)
    out = c2st(_dev(real), _dev(fake), ex, E, degree=degree, gtol=GTOL, details=True)
    xr_ref, xf_ref, _, _ = R.c2st_features(name)
    xr, xf = out["real"].cpu().numpy(), out["fake"].cpu().numpy()
    # the device's features against numpy's: one rounded shift and scale each (pooled moments of 2 N rows), then one
    # product; the tables are the joint rows followed by the experts' gathered rows
    tol = 64 * (2 * N) * R.U * (1.0 + np.abs(xr_ref).max()) ** 2
    assert xr.shape[0] == (2 * N if E > 1 else N) and np.abs(xr[:N] - xr_ref).max() <= tol
    assert np.abs(xf[:N] - xf_ref).max() <= tol
    segs = R.segments(expert, E, N)
    seg_dev = out["seg"].cpu().numpy()
    worst = 0.0
    for s, rows in enumerate(segs):
        b, e = seg_dev[s]
        assert e - b == len(rows) and (s == 0 or np.array_equal(xr[b:e], xr[rows]))
        # the reference: the restatement on the DEVICE's feature rows with the record's theta
        theta_rec = golden[f"c2st_{name}_s{s}_theta"]
        h = R.held_out(xr, xf, np.arange(b, e), theta_rec)
        Z, y = R.train_design(xr, xf, np.arange(b, e))
        theta = out["theta"].cpu().numpy()[s]
        D, bound, r = R.distance_bound(theta, theta_rec, Z, y)
        assert D <= bound and r < 1e-5, (name, s, D, bound)
        Zall = np.concatenate([h["Zr"], h["Zf"]])
        sb = (bound * np.linalg.norm(Zall, axis=1) + R.score_bound(theta, Zall) + R.score_bound(theta_rec, Zall)).max()
        prior = R.prior_score_slack(theta_rec, Z, y, Zall, GTOL)          # what the CPU test allowed for
        worst = max(worst, 2 * sb / h["gap"], sb / prior)
        assert h["gap"] > 2 * sb and sb <= prior, (name, s, h["gap"], sb, prior)   # no pair the slack could swap
        key = (lambda k: k) if s == 0 else (lambda k: f"{k}_{s - 1}")
        nu, nv, u2, ks = h["rank"]
        assert tuple(out["rank"].cpu().numpy()[s, 0]) == h["rank"], (name, s)          # integers: EQUAL
        assert out[key("c2st_auc")] == u2 / (2.0 * nu * nv) and out[key("c2st_ks")] == ks / (nu * nv)
        assert out[key("c2st_acc")] == 0.5 * (h["hits"][0] / nu + h["hits"][1] / nv)   # |t| > the slack everywhere?
        lb = (R.logloss_bound(theta_rec, h["Zr"], R.softplus(-h["r_scores"]))
              + R.logloss_bound(theta_rec, h["Zf"], R.softplus(h["f_scores"])) + 2 * (nu + nv) * sb) / (nu + nv)
        worst = max(worst, abs(out[key("c2st_logloss")] - sum(h["loss"]) / (nu + nv)) / lb)
        assert out[key("c2st_converged")] == 1.0 and 1 <= out[key("c2st_iter")] <= 30
        assert min(np.abs(h["r_scores"]).min(), np.abs(h["f_scores"]).min()) > sb      # ... yes
    print(f"c2st {name}: worst error / bound {worst:.3g}")
    assert worst <= 1.0
    plain = c2st(_dev(real), _dev(fake), ex, E, degree=degree, gtol=GTOL)
    assert set(plain) == ({*KEYS, *[f"{k}_{e}" for k in KEYS for e in range(E)]} if E > 1 else set(KEYS))
    assert all(plain[k] == out[k] for k in plain)                                      # a rerun is bit-equal


def test_c2st_edges():
    from expertsim.train.classifier import KEYS, c2st, standardise
    rs = np.random.RandomState(4)
    real, fake = rs.randn(40, 3), rs.randn(40, 3) + 1.0
    real[:, 1] = fake[:, 1] = 2.5                                            # a constant column drops out
    zr, zf, shift, scale = standardise(_dev(real), _dev(fake))
    assert scale.cpu().tolist()[1] == 0.0 and (zr[:, 1] == 0).all() and (zf[:, 1] == 0).all()
    expert = np.zeros(40, dtype=np.int32)
    expert[0] = 2                                                            # expert 1 empty, expert 2 one row
    out = c2st(_dev(real), _dev(fake), _dev(expert), 3, degree=1, gtol=GTOL)
    assert 0.5 < out["c2st_auc"] <= 1.0 and out["c2st_converged"] == 1.0 and not np.isnan(out["c2st_auc_0"])
    assert all(np.isnan(out[f"{k}_{e}"]) for k in KEYS for e in (1, 2))
    with pytest.raises(ValueError):
        c2st(_dev(rs.randn(20, 12)), _dev(rs.randn(20, 12)))
    identical = c2st(_dev(real), _dev(real), degree=2, gtol=GTOL)            # nothing to tell apart
    assert identical["c2st_auc"] == 0.5 and identical["c2st_ks"] == 0.0
    assert abs(identical["c2st_logloss"] - np.log(2.0)) < 1e-12


# ------------------------------------------------------------------------------------------ wiring
def _bytes(t):
    return t.contiguous().view(torch.uint8)


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


def _c2st_keys(E):
    from expertsim.train.classifier import KEYS
    return set(KEYS) | {f"{n}_{e}" for n in KEYS for e in range(E)}


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


def test_evaluate_device_classifier():
    from expertsim.train import classifier as K
    E, N, seed = 3, 96, 17
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, classifier=True)
    extra = {"c2st_obs_real", "c2st_obs_gen", "c2st_theta", "c2st_table"}
    assert set(det) == set(plain) | _c2st_keys(E) | extra
    for key, v in plain.items():                                                   # bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(_bytes(det[key]), _bytes(v)), key
        else:
            assert det[key] == v, key
    assert tuple(det["c2st_obs_real"].shape) == (N, 10) and det["c2st_obs_real"].dtype == torch.float64
    assert torch.equal(det["c2st_obs_real"][:, :5], det["sums_real"]) and torch.equal(det["c2st_obs_gen"][:, :5],
                                                                                      det["sums_gen"][0])
    assert tuple(det["c2st_theta"].shape) == (E + 1, 66) and np.isfinite(det["c2st_auc"]) and 0 <= det["c2st_ks"] <= 1
    want = K.c2st(det["c2st_obs_real"], det["c2st_obs_gen"], det["expert"], E)
    assert set(want) == _c2st_keys(E) and all(_same_float(det[k], v) for k, v in want.items())
    lin = moe.evaluate_device(5, cond, x, cfg, seed=seed, classifier=True, classifier_degree=1)
    want1 = K.c2st(det["c2st_obs_real"], det["c2st_obs_gen"], det["expert"], E, degree=1)
    assert all(_same_float(lin[k], v) for k, v in want1.items()) and lin["ws_mean"] == det["ws_mean"]
    both = moe.evaluate_device(5, cond, x, cfg, seed=seed, classifier=True, distances=True, features=True)
    alone = moe.evaluate_device(5, cond, x, cfg, seed=seed, distances=True, features=True)
    assert set(both) == set(alone) | _c2st_keys(E)
    assert all(_same_float(both[k], alone[k]) for k in alone) and all(_same_float(both[k], det[k]) for k in _c2st_keys(E))


def test_evaluate_epoch_averages_classifier():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    E, N, bs = 3, 106, 48
    on = ("train.eval_on_device=true", "train.eval_classifier=true", "train.eval_classifier_degree=1")
    moe, cfg = _moe(E, extra=on)
    b, x, cond = _batch(N)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg, device=torch.device(DEV))
    cfg_off = _cfg(E, extra=("train.eval_on_device=true",))
    off = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_off, device=torch.device(DEV))
    assert set(out) == set(off) | _c2st_keys(E) and all(out[key] == off[key] for key in off)
    per = [moe.evaluate_device(0, cond[i:i + bs], x[i:i + bs], cfg, seed=int(cfg.train.rng_seed), sample_offset=i,
                               classifier=True, classifier_degree=1) for i in range(0, N, bs)]
    assert all(np.isfinite(m["c2st_auc"]) for m in per) and np.isfinite(out["c2st_auc"])
    for key in _c2st_keys(E):
        finite = [m[key] for m in per if np.isfinite(m[key])]
        if finite:
            assert out[key] == sum(finite) / len(finite), key
        else:
            assert np.isnan(out[key]), key
    cfg_bad = _cfg(E, extra=("train.eval_classifier=true",))
    with pytest.raises(ValueError, match="train.eval_classifier needs train.eval_on_device"):
        evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_bad, device=torch.device(DEV))


def test_cli_simulate_real_classifier(tmp_path):
    import os
    import subprocess
    import sys

    from conftest import REPO
    from expertsim.train import distances as dist
    from expertsim.train.classifier import c2st
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    E, N = 3, 64
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
                        "--sim-batch-size", "16", "--real", str(tmp_path / "real.npy"), "--classifier",
                        "--classifier-degree", "1", "--seed", "5", "--out", str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert _c2st_keys(E) <= set(z.files) and int(z["c2st_degree"]) == 1
    images, expert = torch.from_numpy(z["images"]).to(DEV), torch.from_numpy(z["expert"]).to(DEV)
    obs_real = dist.observables(x.to(DEV), log_domain=True)
    obs_gen = dist.observables(images, log_domain=False, sums=torch.from_numpy(z["sums"]).to(DEV))
    want = c2st(obs_real, obs_gen, expert, E, degree=1)
    for key in _c2st_keys(E):
        assert z[key].dtype == np.float64 and _same_float(float(z[key]), want[key]), key
        assert f"{key} = " in r.stdout
    assert np.isfinite(float(z["c2st_auc"]))
