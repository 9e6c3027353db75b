"""es_segment_histogram / es_segment_kde on the device against tests/diag_refs.py and tests/golden/diag_kde.npz,
and MoEWrapper.diagnose / loop.evaluate_epoch(train.eval_diagnostics) / cli --diagnose end to end.

Bounds (tests/diag_refs.py has the derivations): counts, outside, edges, grids, valid and sd exactly; bw within
17 * 2^-53 relative of the golden's h; the density per grid point within (n + 40 A_j + 9) 2^-53 relative of the
golden (np.longdouble), below 2^-999 where the golden is below 2^-1000, NaN where invalid.

Worst density error / bound seen on an MI355X (one run): 0.098 (n5 0.089, n64 0.057, n65 0.098, n1000_clusters
0.037, n4097 0.002); bw equal to the golden's h bit for bit in all five."""
import numpy as np
import pytest
import torch

import diag_refs as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = ("const", "three", "edges", "normal", "gamma", "ints", "tiny", "neg", "wide")


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)


def _column(kind, rows, bins, rng):
    if kind == "const":
        return np.full(rows, 0.37)
    if kind == "three":                                   # mass / charge: whole waves on one bin
        return rng.choice([-1.0, 0.0, 1.0], rows)
    if kind == "edges":                                   # values exactly on the computed edges, lo and hi included
        e = DR.linspace_ref(-2.0, 5.5, bins + 1)
        v = e[rng.integers(0, bins + 1, rows)]
        v[0] = e[0]
        v[-1] = e[-1]
        return v
    if kind == "normal":
        return rng.normal(0.0, 3.0, rows)
    if kind == "gamma":
        return rng.gamma(2.0, 1.5, rows)
    if kind == "ints":
        return rng.integers(-5, 6, rows).astype(np.float64)
    if kind == "tiny":
        return rng.normal(0.0, 1e-12, rows)
    if kind == "neg":
        return -rng.gamma(1.0, 100.0, rows)
    return rng.normal(0.0, 1.0, rows) * 10.0 ** rng.integers(-3, 4, rows)


def _layout(rows, E, rng):
    """(expert [rows], perm, segments [S, 2] over perm, members per segment): E = 4 keeps expert 2 empty and adds
    the overlapping "all rows" segment."""
    if E == 1:
        return np.zeros(rows, dtype=np.int64), np.arange(rows), np.array([[0, rows]]), [np.arange(rows)]
    expert = rng.choice([0, 1, 3], rows)
    perm = np.argsort(expert, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(expert, minlength=E))])
    seg = np.concatenate([np.stack([offs[:-1], offs[1:]], axis=1), [[0, rows]]])
    return expert, perm, seg, [perm[a:b] for a, b in seg]


def _device_matrix(x, pad):
    """x [rows, cols] on the device with a row stride of cols + pad (the pad columns hold NaN)."""
    rows, cols = x.shape
    full = torch.full((rows, cols + pad), float("nan"), device=DEV,
                      dtype=torch.float64 if x.dtype == np.float64 else torch.float32)
    full[:, :cols] = torch.from_numpy(np.array(x)).to(DEV)      # np.array: a writable copy (goldens are read-only)
    return full[:, :cols]


def _run_hist(x, perm, seg, bins, right, use_idx, pad, edges=None):
    from expertsim.train.diagnostics import segment_histogram_raw
    if use_idx:
        xd, idx = _device_matrix(x, pad), _i32(perm)
    else:                                                 # the same members, contiguous: the rows in perm order
        xd, idx = _device_matrix(np.ascontiguousarray(x[perm]), pad), None
    e = None if edges is None else torch.from_numpy(edges).to(DEV)
    c, eo, o = segment_histogram_raw(xd, _i32(seg), idx, None, bins, right, e)
    return c.cpu().numpy(), eo.cpu().numpy(), o.cpu().numpy()


# ------------------------------------------------------------------------------------ 1. histogram
@pytest.mark.parametrize("cols", [1, 9])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000, 4097])
def test_histogram_equals_the_restatement(rows, cols):
    rng = np.random.default_rng(1000 * rows + cols)
    runs = 0
    for bins in (1, 50, 257):
        full = np.stack([_column(k, rows, bins, rng) for k in KINDS], axis=1)
        for E in (1, 4):
            _, perm, seg, members = _layout(rows, E, rng)
            lengths = np.array([len(m) for m in members])
            for dtype in (np.float64, np.float32):
                # one column: each content in turn; nine: all of them side by side
                for x in ([full[:, k:k + 1] for k in range(4)] if cols == 1 else [full]):
                    x = np.ascontiguousarray(x.astype(dtype))
                    for right in (False, True):
                        want_c, want_e, want_o = DR.segment_histogram_ref(x, members, bins, right)
                        lin = np.stack([np.linspace(np.float64(col.min()), np.float64(col.max()), bins + 1)
                                        for col in x.T])
                        for use_idx, pad in ((True, 0), (False, 0), (True, 3), (False, 1)):
                            got_c, got_e, got_o = _run_hist(x, perm, seg, bins, right, use_idx, pad)
                            assert (got_e == lin).all() and (got_e == want_e).all()        # np.linspace, bit for bit
                            assert np.array_equal(got_c, want_c), (bins, E, dtype, right, use_idx, pad)
                            assert not got_o.any() and np.array_equal(got_o, want_o)
                            assert np.array_equal(got_c.sum(axis=2), lengths[:, None] - got_o)
                            runs += 1
    assert runs == (3 * 2 * 2 * 2 * 4) * (4 if cols == 1 else 1)


def test_histogram_content_columns_do_what_they_are_for():
    rng = np.random.default_rng(8)
    rows, bins = 1000, 50
    x = np.stack([_column(k, rows, bins, rng) for k in KINDS], axis=1)
    seg, perm = np.array([[0, rows]]), np.arange(rows)
    c0, e0, _ = _run_hist(x, perm, seg, bins, False, False, 0)
    c1, _, _ = _run_hist(x, perm, seg, bins, True, False, 0)
    assert (e0[0] == 0.37).all() and c0[0, 0, -1] == rows and c1[0, 0, 0] == rows            # the constant column
    assert sorted(c0[0, 1][c0[0, 1] > 0].tolist()) == sorted(np.bincount((x[:, 1] + 1).astype(int)).tolist())
    assert np.array_equal(e0[2], DR.linspace_ref(-2.0, 5.5, bins + 1)) and np.isin(x[:, 2], e0[2]).all()
    assert not np.array_equal(c0[0, 2], c1[0, 2])                       # ties on the edges tell the modes apart
    assert c0[0, 2, 0] >= 1 and c0[0, 2, -1] >= 2 and c1[0, 2, 0] >= 2 and c1[0, 2, -1] >= 1


@pytest.mark.parametrize("rows", [65, 4097])
def test_histogram_with_given_edges_counts_the_outside(rows):
    rng = np.random.default_rng(rows)
    for cols, bins in ((1, 1), (9, 50), (9, 257)):
        x = np.stack([_column(k, rows, bins, rng) for k in KINDS[:cols]], axis=1) if cols > 1 else \
            _column("normal", rows, bins, rng)[:, None]
        edges = np.empty((cols, bins + 1))
        for c in range(cols):
            lo, hi = x[:, c].min(), x[:, c].max()
            span = hi - lo if hi > lo else 1.0
            e = rng.uniform(lo + 0.2 * span, lo + 0.8 * span, bins + 1)
            take = min(bins + 1, 5)
            e[:take] = rng.choice(x[:, c], take)          # edges that are data values: ties
            if bins >= 8:
                e[5:8] = e[4]                             # repeated edges: empty bins
            edges[c] = np.sort(e)
        _, perm, seg, members = _layout(rows, 4, rng)
        lengths = np.array([len(m) for m in members])
        for dtype in (np.float64, np.float32):
            xt = np.ascontiguousarray(x.astype(dtype))
            for right in (False, True):
                want_c, _, want_o = DR.segment_histogram_ref(xt, members, bins, right, edges)
                for use_idx, pad in ((True, 0), (False, 2)):
                    got_c, got_e, got_o = _run_hist(xt, perm, seg, bins, right, use_idx, pad, edges)
                    assert np.array_equal(got_e.view(np.int64), edges.view(np.int64))
                    assert np.array_equal(got_c, want_c) and np.array_equal(got_o, want_o)
                    assert np.array_equal(got_c.sum(axis=2), lengths[:, None] - got_o)
                if cols > 1 and rows > 100:
                    assert (want_o[-1] > 0).sum() >= 5 and want_c.sum() > 0


def test_histogram_rerun_is_bitwise_equal_and_public_wrapper():
    from expertsim.train.diagnostics import segment_histogram
    rng = np.random.default_rng(4)
    rows = 4097
    x = torch.from_numpy(np.stack([_column(k, rows, 50, rng) for k in KINDS], axis=1)).to(DEV)
    expert = torch.from_numpy(rng.choice([0, 1, 3], rows).astype(np.int32)).to(DEV)
    a = segment_histogram(x, expert, 4, bins=50, right=True)
    b = segment_histogram(x, expert, 4, bins=50, right=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    counts, edges, outside = a
    assert counts.shape == (4, 9, 50) and edges.shape == (9, 51) and outside.shape == (4, 9)
    assert torch.equal(counts.sum(dim=2), torch.bincount(expert.long(), minlength=4).int()[:, None].expand(4, 9))
    members = [np.flatnonzero(expert.cpu().numpy() == e) for e in range(4)]
    want, _, _ = DR.segment_histogram_ref(x.cpu().numpy(), members, 50, True)
    assert np.array_equal(counts.cpu().numpy(), want)
    one, _, _ = segment_histogram(x[:, 3])                               # a 1-D input, one segment over all rows
    assert one.shape == (1, 1, 50) and int(one.sum()) == rows


# --------------------------------------------------------------------------------------- 2. KDE
def _run_kde(x, seg, idx=None, points=100, grid=None, pad=0, **kw):
    from expertsim.train.diagnostics import segment_kde_raw
    xd = _device_matrix(np.ascontiguousarray(x), pad)
    g = None if grid is None else torch.from_numpy(np.array(grid)).to(DEV)      # a writable copy
    out = segment_kde_raw(xd, _i32(seg), None if idx is None else _i32(idx), None, points, g, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_kde_moments_and_validity():
    rng = np.random.default_rng(6)
    d = rng.gamma(2.0, 1.5, 9)
    x = np.stack([d, np.full(9, 0.3), d * 1e-13], axis=1)   # random, constant, below std_eps
    seg = np.array([[0, 4], [0, 5], [0, 9], [3, 3]])
    out = _run_kde(x, seg, points=11)
    assert out["valid"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]]
    for s, (a, b) in enumerate(seg):
        for c in range(3):
            ref = DR.kde_ref(x[a:b, c], out["grid"][c])
            assert out["valid"][s, c] == ref["valid"]
            assert out["sd"][s, c] == ref["sd"]                              # fp64 + - * / sqrt: bit-equal
            if ref["valid"]:
                assert abs(out["bw"][s, c] - ref["bw"]) <= DR.BW_BOUND * ref["bw"]
                assert np.isfinite(out["density"][s, c]).all()
            else:
                assert out["bw"][s, c] == 0.0 and np.isnan(out["density"][s, c]).all()
    # the grid: np.linspace of the column's range over all rows, a constant column widened by 1e-6 either side
    for c in range(3):
        assert np.array_equal(out["grid"][c], np.linspace(x[:, c].min(), x[:, c].max(), 11)) or c == 1
    assert np.array_equal(out["grid"][1], np.linspace(0.3 - 1e-6, 0.3 + 1e-6, 11))
    # min_samples / std_eps are the caller's
    loose = _run_kde(x, seg, points=11, min_samples=2, std_eps=0.0)
    assert loose["valid"][:, [0, 2]].tolist() == [[1, 1], [1, 1], [1, 1], [0, 0]]
    for s, (a, b) in enumerate(seg):
        assert loose["valid"][s, 1] == DR.kde_ref(x[a:b, 1], loose["grid"][1], 2, 0.0)["valid"]
    # Q = 0 exactly (0.5 sums without rounding) is never valid: there is no bandwidth
    flat = _run_kde(np.full((6, 1), 0.5), np.array([[0, 6]]), points=5, min_samples=2, std_eps=0.0)
    assert flat["valid"][0, 0] == 0 and flat["sd"][0, 0] == 0.0 and np.isnan(flat["density"]).all()


@pytest.mark.parametrize("name", DR.GOLDEN_CASES)
def test_kde_density_against_the_golden(name):
    case = DR.golden()[name]
    d, grid = case["d"], case["grid"]
    n, points = len(d), len(grid)
    assert (n, points) in ((5, 100), (64, 100), (65, 100), (1000, 37), (4097, 100))
    seg = np.array([[0, n], [0, 0]])                          # the members, and an empty segment
    out = _run_kde(d[:, None], seg, points=points, grid=grid[None])
    assert out["valid"][:, 0].tolist() == [1, 0] and np.isnan(out["density"][1, 0]).all() and out["bw"][1, 0] == 0.0
    assert np.array_equal(out["grid"][0].view(np.int64), grid.view(np.int64))
    assert out["sd"][0, 0] == case["sd"]
    assert abs(out["bw"][0, 0] - case["h"]) <= DR.BW_BOUND * case["h"]
    worst = DR.check_density(out["density"][0, 0], case)
    print(f"{name}: n={n} points={points} worst density error / bound {worst:.4f}; "
          f"bw error {abs(out['bw'][0, 0] - case['h']) / case['h'] / DR.U:.2f} ulp")
    if name != "n1000_clusters":                              # the grid the kernel computes is the golden's
        own = _run_kde(d[:, None], seg, points=points)
        assert np.array_equal(own["grid"][0].view(np.int64), grid.view(np.int64))
        assert np.array_equal(own["density"][0, 0].view(np.int64), out["density"][0, 0].view(np.int64))
    else:
        assert (case["density"] < 2.0 ** -1000).sum() >= 2
    # float32 members are widened exactly
    d32 = d.astype(np.float32)
    out32 = _run_kde(d32[:, None], seg, points=points, grid=grid[None])
    out64 = _run_kde(d32.astype(np.float64)[:, None], seg, points=points, grid=grid[None])
    for k in ("density", "bw", "sd", "valid"):
        assert np.array_equal(out32[k].view(np.uint8), out64[k].view(np.uint8)), k


def test_kde_segment_is_independent_of_its_surroundings():
    rng = np.random.default_rng(9)
    n, rows, points = 600, 1500, 33                          # 600: three member chunks, the split moments
    d = np.stack([rng.gamma(2.0, 1.5, n), rng.normal(1.0, 4.0, n)], axis=1)
    grid = np.stack([np.linspace(-1.0, 12.0, points), np.linspace(-12.0, 14.0, points)])
    alone = _run_kde(d, np.array([[0, n]]), points=points, grid=grid)
    assert alone["valid"].all()
    # embedded: the members at shuffled rows of a larger matrix, listed in the same member order, among others
    where = rng.permutation(rows)[:n]
    big = rng.normal(0.0, 50.0, (rows, 2))
    big[where] = d
    others = np.setdiff1d(np.arange(rows), where)
    idx = np.concatenate([others[:400], where, others[400:]])
    seg = np.array([[0, 400], [400, 400 + n], [0, rows], [400 + n, rows]])
    for pad in (0, 3):
        emb = _run_kde(big, seg, idx=idx, points=points, grid=grid, pad=pad)
        for k in ("density", "bw", "sd", "valid"):
            assert np.array_equal(emb[k][1].view(np.uint8), alone[k][0].view(np.uint8)), (k, pad)
        again = _run_kde(big, seg, idx=idx, points=points, grid=grid, pad=pad)
        for k in emb:
            assert np.array_equal(again[k].view(np.uint8), emb[k].view(np.uint8)), k
    # contiguous against through idx, and a wider ld, on the segment alone
    wide = _run_kde(d, np.array([[0, n]]), points=points, grid=grid, pad=5)
    via = _run_kde(big, np.array([[0, n]]), idx=np.concatenate([where, others]), points=points, grid=grid)
    for k in ("density", "bw", "sd", "valid"):
        assert np.array_equal(wide[k].view(np.uint8), alone[k].view(np.uint8)), k
        assert np.array_equal(via[k].view(np.uint8), alone[k].view(np.uint8)), k
    # and it is the restatement's order up to the exponential's last bits
    ref = DR.kde_ref(d[:, 0], grid[0])
    assert alone["sd"][0, 0] == ref["sd"]
    assert np.allclose(alone["density"][0, 0], ref["density"], rtol=1e-11, atol=0.0)


# --------------------------------------------------------------------------------- 3. integration
def _moe(E, extra=()):
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", "train.precision=fp32", "model.router.diff_strength=1e-6",
                                 *extra])
    torch.manual_seed(4)
    moe = setup_moe_system(cfg, torch.device(DEV))
    moe.eval()
    moe.eval_batch_size = 128                                # N = 257: chunks of 128, 128, 1
    return moe, cfg


def _batch(n):
    from expertsim.utils.synthetic import make_batch
    return make_batch(n, "neutron", seed=11)


def _state(moe):
    out = {k: v.detach().clone() for k, v in moe.state_dict().items()}
    out["step_count"] = moe.step_count
    out["rng"] = moe.rng.counter
    out["g_steps"], out["d_steps"] = list(moe.g_steps), list(moe.d_steps)
    return out


def _same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].reshape(-1).contiguous().view(torch.uint8),
                               b[k].reshape(-1).contiguous().view(torch.uint8)), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("E", [4, 1])
def test_diagnose(E):
    from expertsim.train.diagnostics import DIAGNOSTIC_KEYS
    from expertsim.utils.data_preparation import photon_sums_and_peaks
    N, seed, bins, points = 257, 13, 50, 100
    moe, _ = _moe(E)
    cond_host = _batch(N)["cond"].astype(np.float32)
    cond = torch.from_numpy(cond_host).to(DEV)
    C = cond_host.shape[1]
    before = _state(moe)
    flags = [m.training for m in moe.modules()]
    diag = moe.diagnose(cond, seed=seed)
    _same_state(before, _state(moe))
    assert flags == [m.training for m in moe.modules()]
    assert set(diag) == set(DIAGNOSTIC_KEYS)
    K = len(np.unique(cond_host[:, -1]))
    shapes = {"expert_count": (E,), "photon_sum_hist": (E, bins), "photon_sum_edges": (bins + 1,),
              "cond_hist": (E, C, bins), "cond_edges": (C, bins + 1), "cond_kde": (E, C - 1, points),
              "cond_kde_grid": (C - 1, points), "cond_kde_bw": (E, C - 1), "cond_kde_valid": (E, C - 1),
              "cat_values": (K,), "cat_count": (E, K)}
    assert {k: diag[k].shape for k in shapes} == shapes
    sim = moe.simulate(cond, seed=seed, domain="photons")
    expert = sim["expert"].cpu().numpy()
    count = np.bincount(expert, minlength=E)
    assert np.array_equal(diag["expert_count"], torch.bincount(sim["expert"].long(), minlength=E).cpu().numpy())
    if E > 1:
        assert (count > 0).sum() >= 2, "the tiny router sends everything to one expert: the test shows nothing"
    members = [np.flatnonzero(expert == e) for e in range(E)]
    ps = photon_sums_and_peaks(sim["images"], check=False)[0].cpu().numpy()
    want, edges, _ = DR.segment_histogram_ref(ps[:, None], members, bins, False)
    assert np.array_equal(diag["photon_sum_hist"], want[:, 0]) and np.array_equal(diag["photon_sum_edges"], edges[0])
    want, edges, _ = DR.segment_histogram_ref(cond_host, members, bins, True)
    assert np.array_equal(diag["cond_hist"], want) and np.array_equal(diag["cond_edges"], edges)
    assert np.array_equal(diag["photon_sum_hist"].sum(axis=1), count)
    assert np.array_equal(diag["cond_hist"].sum(axis=2), np.repeat(count[:, None], C, axis=1))
    values, codes = np.unique(cond_host[:, -1], return_inverse=True)
    assert np.array_equal(diag["cat_values"], values.astype(np.float64))
    assert np.array_equal(diag["cat_count"], np.stack([np.bincount(codes[m], minlength=K) for m in members]))
    wide = cond_host.astype(np.float64)
    for c in range(C - 1):
        grid = DR.kde_grid_ref(wide[:, c].min(), wide[:, c].max(), points)
        assert np.array_equal(diag["cond_kde_grid"][c], grid)
        for e in range(E):
            ref = DR.kde_ref(wide[members[e], c], grid)
            assert diag["cond_kde_valid"][e, c] == ref["valid"]
            if ref["valid"]:
                assert abs(diag["cond_kde_bw"][e, c] - ref["bw"]) <= (DR.BW_BOUND + DR.U) * ref["bw"]
                assert np.isfinite(diag["cond_kde"][e, c]).all() and diag["cond_kde"][e, c].max() > 0
            else:
                assert np.isnan(diag["cond_kde"][e, c]).all() and diag["cond_kde_bw"][e, c] == 0.0
    assert diag["cond_kde_valid"].any()
    again = moe.diagnose(cond, seed=seed, names=[f"v{i}" for i in range(C)])
    assert again.pop("cond_names").tolist() == [f"v{i}" for i in range(C)]
    assert all(np.array_equal(again[k], diag[k], equal_nan=True) for k in diag)


def test_evaluate_epoch_with_eval_diagnostics(tmp_path):
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    N = 257
    b = _batch(N)
    x = torch.from_numpy(b["real_images"])
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    outs = {}
    for flag in (False, True):
        moe, cfg = _moe(4, extra=("train.eval_on_device=true", f"train.eval_diagnostics={str(flag).lower()}",
                                  "train.save_experiment_data=true"))
        cfg.train.dir_info = str(tmp_path / "info")
        outs[flag] = evaluate_epoch(moe, DataLoader(ds, batch_size=200), epoch=5, cfg=cfg, device=torch.device(DEV))
    off, on = outs[False], outs[True]
    assert set(on) == set(off) | {"expert_diagnostics"}
    assert all(on[k] == off[k] for k in off)                  # bit for bit
    want = moe.diagnose(torch.from_numpy(b["cond"]).to(DEV), seed=int(cfg.train.rng_seed), sample_offset=0)
    diag = on["expert_diagnostics"]
    assert set(diag) == set(want) and all(np.array_equal(diag[k], want[k], equal_nan=True) for k in want)
    assert int(diag["expert_count"].sum()) == N
    z = np.load(tmp_path / "info" / "diagnostics_epoch_5.npz")
    assert set(z.files) == set(want) and all(np.array_equal(z[k], want[k], equal_nan=True) for k in want)


def test_cli_diagnose(tmp_path):
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    import cli
    moe, cfg = _moe(4)
    models = tmp_path / "models"
    models.mkdir()
    save_checkpoint(str(models), 0, moe, *setup_optimizers(moe, cfg))
    cond = _batch(64)["cond"]
    np.save(tmp_path / "cond.npy", cond)
    args = cli.parse_args(["-o", "model.architecture=neutron", "dataset.input_image_shape=[44,44]", "model.n_experts=4",
                           "model.router.diff_strength=1e-6", "train.precision=fp32", "--diagnose", "--checkpoint", str(models), "--conditions",
                           str(tmp_path / "cond.npy"), "--out", str(tmp_path / "diag.npz"), "--seed", "3"])
    path = cli.diagnose(args)
    z = np.load(path)
    want = moe.diagnose(torch.from_numpy(cond).to(DEV), seed=3)
    assert set(z.files) == set(want) and all(np.array_equal(z[k], want[k], equal_nan=True) for k in want)
