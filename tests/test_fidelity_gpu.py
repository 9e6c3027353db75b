"""es_knn_radius / es_prdc_count on the device against scikit-learn's record (tests/golden/prdc_sklearn.npz) and the
numpy restatement (tests/prdc_refs.py), and expertsim.train.fidelity / MoEWrapper.evaluate_device(prdc=True) /
loop.evaluate_epoch(train.eval_prdc) / ``cli.py --simulate --real`` end to end.

Bounds.  Against the restatement: the contract pins the order of every floating-point operation of a distance and
only values are selected or compared, so radius2 and r_min2 are compared bitwise and f_count, r_hit and totals
exactly.  Against the record: the totals exactly (tools/make_prdc_golden.py asserted a gap of at least 1000 B
around every strict comparison) and the squared radii within B = (cols + 3) 2^-52 4 max|x|^2, the rounding bound
of scikit-learn's expansion form (prdc_refs.bound).  Outputs are pre-filled (NaN / -1) and must keep the fill
past a segment's length."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prdc_refs as R
import segment_refs as S
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _check_against_restatement(real, fake, k, r_idx=None, r_seg=None, f_idx=None, f_seg=None, real_dev=None,
                               fake_dev=None):
    """Run prdc_raw (sentinel-filled outputs) and compare every output of every segment with the restatement."""
    from expertsim.train.fidelity import prdc_raw
    n_r, n_f = len(real), len(fake)
    r_seg = np.array([[0, n_r]]) if r_seg is None else np.asarray(r_seg)
    f_seg = np.array([[0, n_f]]) if f_seg is None else np.asarray(f_seg)
    rd = torch.from_numpy(real).to(DEV) if real_dev is None else real_dev
    fd = torch.from_numpy(fake).to(DEV) if fake_dev is None else fake_dev
    raw = prdc_raw(rd, fd, k, r_idx=None if r_idx is None else torch.from_numpy(r_idx).to(DEV),
                   r_seg=torch.from_numpy(r_seg.astype(np.int32)).to(DEV), r_cap=n_r,
                   f_idx=None if f_idx is None else torch.from_numpy(f_idx).to(DEV),
                   f_seg=torch.from_numpy(f_seg.astype(np.int32)).to(DEV), f_cap=n_f)
    got = {key: v.cpu().numpy() for key, v in raw.items()}
    m_r, m_f = S.members(n_r, r_idx, r_seg, n_r), S.members(n_f, f_idx, f_seg, n_f)
    for s, (ir, jf) in enumerate(zip(m_r, m_f)):
        ref = R.segment(real[ir], fake[jf], k)
        L_r, L_f = len(ir), len(jf)
        assert np.array_equal(got["totals"][s], ref["totals"]), (s, got["totals"][s], ref["totals"])
        assert np.array_equal(_bits(got["r_radius2"][s, :L_r]), _bits(ref["r_radius2"])), s
        assert np.array_equal(_bits(got["f_radius2"][s, :L_f]), _bits(ref["f_radius2"])), s
        assert np.array_equal(_bits(got["r_min2"][s, :L_r]), _bits(ref["r_min2"])), s
        assert np.array_equal(got["f_count"][s, :L_f], ref["f_count"]), s
        assert np.array_equal(got["r_hit"][s, :L_r], ref["r_hit"]), s
        # past the segment's length the fill is untouched
        assert np.isnan(got["r_radius2"][s, L_r:]).all() and np.isnan(got["f_radius2"][s, L_f:]).all()
        assert np.isnan(got["r_min2"][s, L_r:]).all()
        assert (got["f_count"][s, L_f:] == -1).all() and (got["r_hit"][s, L_r:] == -1).all()
    return got


def _images(rs, n, cols, density=0.2):
    return (rs.rand(n, cols) * 5.0 * (rs.rand(n, cols) < density)).astype(np.float32)


# ------------------------------------------------------------------------------------------ 1. the record
@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


@pytest.mark.parametrize("arch", list(R.ARCHS))
def test_record(golden, arch):
    from expertsim.segments import expert_segments
    from expertsim.train.fidelity import prdc, prdc_raw
    real, fake = golden[f"{arch}_real"], golden[f"{arch}_fake"]
    rd, fd = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    r_perm, r_seg, _ = expert_segments(torch.from_numpy(golden[f"{arch}_expert_r"]), R.N_EXPERTS, len(real), rd.device,
                                       joint=True)
    f_perm, f_seg, _ = expert_segments(torch.from_numpy(golden[f"{arch}_expert_f"]), R.N_EXPERTS, len(fake), fd.device,
                                       joint=True)
    m_r = R.members(golden[f"{arch}_expert_r"], R.N_EXPERTS)
    m_f = R.members(golden[f"{arch}_expert_f"], R.N_EXPERTS)
    rp, rs_, fp, fs_ = (t.cpu().numpy() for t in (r_perm, r_seg, f_perm, f_seg))
    for k in R.KS:
        want = golden[f"{arch}_k{k}_totals"]
        joint = prdc(rd, fd, k=k, details=True)
        assert np.array_equal(joint["totals"].cpu().numpy(), want[:1])
        assert tuple(joint[n] for n in ("precision", "recall", "density", "coverage")) == R.metrics(want[0], k)
        raw = prdc_raw(rd, fd, k, r_idx=r_perm, r_seg=r_seg, r_cap=len(real), f_idx=f_perm, f_seg=f_seg,
                       f_cap=len(fake))
        totals = raw["totals"].cpu().numpy()
        assert np.array_equal(totals, want), (k, totals, want)
        from expertsim.train.fidelity import metrics_from_totals
        m = metrics_from_totals(totals, k)
        assert np.array_equal(np.isnan(m).all(axis=1), want[:, 2] == 0)       # NaN exactly for the invalid segments
        assert np.array_equal(np.isnan(m).any(axis=1), want[:, 2] == 0)
        r2, f2 = raw["r_radius2"].cpu().numpy(), raw["f_radius2"].cpu().numpy()
        for s in range(R.N_EXPERTS + 1):
            L_r, L_f = len(m_r[s]), len(m_f[s])
            # entry p of the device's segment is row perm[b + p]; the record lists the members in ascending order
            at_r = np.searchsorted(m_r[s], rp[rs_[s, 0]:rs_[s, 1]])
            at_f = np.searchsorted(m_f[s], fp[fs_[s, 0]:fs_[s, 1]])
            assert len(at_r) == L_r and len(at_f) == L_f
            if want[s, 2]:
                B = R.bound(real[m_r[s]], fake[m_f[s]])
                err = max(np.abs(r2[s, :L_r] - golden[f"{arch}_k{k}_s{s}_r_radius2"][at_r]).max(),
                          np.abs(f2[s, :L_f] - golden[f"{arch}_k{k}_s{s}_f_radius2"][at_f]).max())
                print(f"{arch} k={k} segment {s}: radius2 error {err:.3g}, B {B:.3g}")
                assert err <= B
            else:
                assert (r2[s, :L_r] == np.inf).all() or L_r > k
                assert (f2[s, :L_f] == np.inf).all() or L_f > k


# ------------------------------------------------------------------------------------------ 2. the restatement
@pytest.mark.parametrize("n_r,n_f,cols,k", [(17, 130, 1, 1), (130, 17, 65, 16)])
def test_tile_edges(n_r, n_f, cols, k):
    rs = np.random.RandomState(n_r + cols)
    _check_against_restatement(_images(rs, n_r, cols, 0.7), _images(rs, n_f, cols, 0.7), k)


def test_column_limit_with_padded_rows():
    rs = np.random.RandomState(7)
    n_r, n_f, cols, k = 257, 255, 4096, 5
    real, fake = _images(rs, n_r, cols, 0.16), _images(rs, n_f, cols, 0.16)
    dark = np.ones(cols, dtype=bool)                 # 3 of 4 columns dark on both sides (the restatement skips them,
    dark[::4] = False                                # the kernel walks all 4096); the last chunk and the chunk edges lit
    dark[-17:] = False
    dark[15:18] = False
    real[:, dark] = 0
    fake[:, dark] = 0
    rbuf = torch.full((n_r, cols + 4), 1e30, dtype=torch.float32, device=DEV)     # the padding would dominate
    fbuf = torch.full((n_f, cols + 13), -1e30, dtype=torch.float32, device=DEV)
    rbuf[:, :cols] = torch.from_numpy(real).to(DEV)
    fbuf[:, :cols] = torch.from_numpy(fake).to(DEV)
    rd, fd = rbuf[:, :cols], fbuf[:, :cols]
    assert rd.stride(0) == cols + 4 and fd.stride(0) == cols + 13
    _check_against_restatement(real, fake, k, real_dev=rd, fake_dev=fd)


def test_index_with_repeated_rows():
    rs = np.random.RandomState(8)
    real, fake = _images(rs, 64, 1936, 0.04), _images(rs, 64, 1936, 0.04)
    r_idx = rs.permutation(64).astype(np.int32)
    r_idx[10:20] = r_idx[40:50]                                                    # ten rows twice
    f_idx = rs.permutation(64).astype(np.int32)
    f_idx[0:7] = f_idx[30]                                                         # one row eight times
    got = _check_against_restatement(real, fake, 5, r_idx=r_idx, f_idx=f_idx)
    assert (got["f_radius2"][0, :7] == 0).all()                                    # eight copies: more than k = 5


def test_collapsed_generator():
    rs = np.random.RandomState(9)
    real = _images(rs, 33, 7, 0.8)
    fake = np.repeat(_images(rs, 1, 7, 0.8), 33, axis=0)
    got = _check_against_restatement(real, fake, 16)
    assert (got["f_radius2"][0] == 0).all() and got["totals"][0, 4] == 0           # recall 0


def test_segment_lengths_around_k_and_empty_segments():
    rs = np.random.RandomState(10)
    real, fake = _images(rs, 40, 50), _images(rs, 37, 50)
    r_seg = [[0, 5], [0, 6], [3, 3], [0, 10], [0, 40], [30, 99], [-4, 7]]
    f_seg = [[0, 6], [0, 5], [0, 10], [7, 7], [0, 37], [20, 37], [5, 2]]
    got = _check_against_restatement(real, fake, 5, r_seg=r_seg, f_seg=f_seg)
    assert got["totals"][:, 2].tolist() == [0, 0, 0, 0, 1, 1, 0]
    assert (got["r_radius2"][0, :5] == np.inf).all() and np.isfinite(got["f_radius2"][0, :6]).all()
    assert (got["r_min2"][3, :10] == np.inf).all()                                 # nothing generated there


def test_segments_of_a_router_dispatch():
    from expertsim.train.fidelity import prdc_device
    rs = np.random.RandomState(11)
    N, k = 150, 3
    real, fake = _images(rs, N, 30), _images(rs, N, 30)
    expert = rs.randint(0, 3, N).astype(np.int32)
    raw = prdc_device(torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV), k,
                      torch.from_numpy(expert).to(DEV), 3, per_row=True)
    perm, seg = raw["perm"].cpu().numpy(), raw["seg"].cpu().numpy()
    assert seg[0].tolist() == [0, N] and sorted(perm.tolist()) == list(range(N))
    for e in range(3):
        assert sorted(perm[seg[1 + e, 0]:seg[1 + e, 1]].tolist()) == np.nonzero(expert == e)[0].tolist()
    _check_against_restatement(real, fake, k, r_idx=perm, r_seg=seg, f_idx=perm, f_seg=seg)
    want = np.stack([R.segment(real[m], fake[m], k)["totals"] for m in S.members(N, perm, seg, N)])
    assert np.array_equal(raw["totals"].cpu().numpy(), want)


def test_several_tiles_and_runs():
    """More than one 128-row tile on both sides: the partial lists of several runs are merged."""
    rs = np.random.RandomState(12)
    real, fake = _images(rs, 300, 20, 0.5), _images(rs, 421, 20, 0.5)
    fake[100:140] = fake[7]
    _check_against_restatement(real, fake, 16)


# ------------------------------------------------------------------------------------------ 3. arguments
def test_bad_arguments_write_nothing():
    from expertsim import hip
    rs = np.random.RandomState(13)
    n, cols, k = 20, 8, 3
    x = torch.from_numpy(_images(rs, n, cols)).to(DEV)
    seg = torch.tensor([[0, n]], dtype=torch.int32, device=DEV)
    rad = torch.full((1, n), -7.0, dtype=torch.float64, device=DEV)
    outs = {"f_count": torch.full((1, n), -7, dtype=torch.int32, device=DEV),
            "r_hit": torch.full((1, n), -7, dtype=torch.int32, device=DEV),
            "r_min2": torch.full((1, n), -7.0, dtype=torch.float64, device=DEV),
            "totals": torch.full((1, 8), -7, dtype=torch.int64, device=DEV)}
    work = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p, st = hip.ptr, hip.stream_ptr()

    def radius(x_=x, ld=cols, cols_=cols, seg_=seg, k_=k, out=rad, work_=work, wb=work.numel()):
        return hip.call("es_knn_radius", p(x_), ld, n, cols_, None, p(seg_), 1, n, k_, p(out), p(work_), wb, st)

    def count(k_=k, cols_=cols, ld=cols, totals=outs["totals"], rr=rad, wb=work.numel()):
        return hip.call("es_prdc_count", p(x), ld, n, None, p(seg), n, p(x), ld, n, None, p(seg), n, cols_, 1, k_,
                        p(rr), p(rad), p(outs["f_count"]), p(outs["r_hit"]), p(outs["r_min2"]), p(totals), p(work), wb,
                        st)

    bad = [lambda: radius(k_=0), lambda: radius(k_=17), lambda: radius(cols_=4097, ld=4097),
           lambda: radius(cols_=cols, ld=cols - 1), lambda: radius(x_=None), lambda: radius(seg_=None),
           lambda: radius(out=None), lambda: radius(wb=8), lambda: radius(work_=None),
           lambda: count(k_=0), lambda: count(k_=17), lambda: count(cols_=4097, ld=4097), lambda: count(ld=cols - 1),
           lambda: count(totals=None), lambda: count(rr=None), lambda: count(wb=8)]
    with torch.cuda.device(x.device):
        for i, fn in enumerate(bad):
            with pytest.raises(hip.HipError):
                fn()
        torch.cuda.synchronize()
        assert (rad == -7.0).all() and all((v == -7).all() for v in outs.values())
        radius()                                                                   # the same calls, good arguments
        count(rr=rad)
        torch.cuda.synchronize()
    ref = R.segment(x.cpu().numpy(), x.cpu().numpy(), k)
    assert np.array_equal(_bits(rad.cpu().numpy()[0]), _bits(ref["r_radius2"]))
    assert np.array_equal(outs["totals"].cpu().numpy()[0], ref["totals"])


# ------------------------------------------------------------------------------------------ 4. rerun
def test_rerun_is_bitwise_equal_on_a_side_stream_too():
    from expertsim.train.fidelity import prdc_device
    rs = np.random.RandomState(14)
    N = 333
    real = torch.from_numpy(_images(rs, N, 100)).to(DEV)
    fake = torch.from_numpy(_images(rs, N, 100)).to(DEV)
    expert = torch.from_numpy(rs.randint(0, 4, N).astype(np.int32)).to(DEV)
    first = prdc_device(real, fake, 5, expert, 4, per_row=True)
    again = prdc_device(real, fake, 5, expert, 4, per_row=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = prdc_device(real, fake, 5, expert, 4, per_row=True)
    side.synchronize()
    torch.cuda.synchronize()
    assert int(first["totals"][0, 2]) == 1 and int(first["totals"][:, 5].sum()) > 0
    for other in (again, third):
        for key, v in first.items():
            assert torch.equal(v.contiguous().view(torch.uint8), other[key].contiguous().view(torch.uint8)), key


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


def _prdc_keys(E):
    from expertsim.train.fidelity import METRICS
    return {f"prdc_{n}" for n in METRICS} | {f"prdc_{n}_{e}" for n in METRICS for e in range(E)}


def _same_float(a, b):
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("E", [1, 3])
def test_evaluate_device_prdc(E):
    from expertsim.train.fidelity import prdc
    N, seed, k = 96, 17, 5
    moe, cfg = _moe(E)
    _, x, cond = _batch(N)
    plain = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True)
    det = moe.evaluate_device(5, cond, x, cfg, seed=seed, details=True, prdc=True, prdc_k=k)
    extra = {"prdc_totals", "prdc_r_radius2", "prdc_f_radius2"}
    assert set(det) == set(plain) | _prdc_keys(E) | extra
    for key, v in plain.items():                                                   # bit for bit
        if isinstance(v, torch.Tensor):
            assert torch.equal(det[key].view(torch.uint8), v.view(torch.uint8)), key
        else:
            assert det[key] == v, key
    sim = moe.simulate(cond, seed=seed, sums=True)
    assert torch.equal(sim["expert"], det["expert"])
    want = prdc(x.to(DEV), torch.log1p(sim["images"]), k=k, expert=sim["expert"], n_experts=E, details=True)
    assert torch.equal(want["totals"], det["prdc_totals"]) and det["prdc_totals"].shape == (E + 1, 8)
    for name in ("precision", "recall", "density", "coverage"):
        assert _same_float(det[f"prdc_{name}"], want[name]) and np.isfinite(det[f"prdc_{name}"])
        for e in range(E):
            assert _same_float(det[f"prdc_{name}_{e}"], want[f"{name}_{e}"])
    totals = det["prdc_totals"].cpu().numpy()
    assert totals[0, :3].tolist() == [N, N, 1] and totals[1:, 0].sum() == N
    short = moe.evaluate_device(5, cond, x, cfg, seed=seed, prdc=True, prdc_k=k)
    assert set(short) == {k_ for k_, v in plain.items() if not isinstance(v, torch.Tensor)} | _prdc_keys(E)
    assert all(_same_float(short[k_], det[k_]) for k_ in short)


def test_evaluate_epoch_averages_over_the_finite_batches():
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    E, k, N, bs = 3, 16, 106, 48                     # batches of 48, 48 and 10 rows: the last has at most k
    moe, cfg = _moe(E, extra=("train.eval_on_device=true", "train.eval_prdc=true", f"train.eval_prdc_k={k}"))
    b, x, cond = _batch(N)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg, device=torch.device(DEV))
    cfg_off = _cfg(E, extra=("train.eval_on_device=true",))
    off = evaluate_epoch(moe, DataLoader(ds, batch_size=bs), epoch=0, cfg=cfg_off, device=torch.device(DEV))
    assert set(out) == set(off) | _prdc_keys(E) and all(out[key] == off[key] for key in off)
    per = [moe.evaluate_device(0, cond[i:i + bs], x[i:i + bs], cfg, seed=int(cfg.train.rng_seed), sample_offset=i,
                               prdc=True, prdc_k=k) for i in range(0, N, bs)]
    assert all(np.isnan(per[2][key]) for key in _prdc_keys(E))                      # 10 rows, k = 16
    assert all(np.isfinite(per[i]["prdc_precision"]) for i in (0, 1))
    for key in _prdc_keys(E):
        finite = [m[key] for m in per if np.isfinite(m[key])]
        if finite:
            assert out[key] == sum(finite) / len(finite), key
        else:
            assert np.isnan(out[key]), key
    assert len([m for m in per if np.isfinite(m["prdc_recall"])]) == 2


def test_cli_simulate_real(tmp_path):
    from expertsim.train.fidelity import prdc
    from expertsim.train.training_setup import setup_optimizers
    from expertsim.train.training_utils import save_checkpoint
    E, N, k = 3, 40, 3
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
                        "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert set(z.files) == {"images", "expert", "sums", "cond"} | _prdc_keys(E) | {"prdc_totals", "prdc_k"}
    want = prdc(x.to(DEV), torch.log1p(torch.from_numpy(z["images"]).to(DEV)), k=k,
                expert=torch.from_numpy(z["expert"]).to(DEV), n_experts=E, details=True)
    assert int(z["prdc_k"]) == k and np.array_equal(z["prdc_totals"], want["totals"].cpu().numpy())
    for key in _prdc_keys(E):
        assert z[key].dtype == np.float64 and _same_float(float(z[key]), want[key[5:]]), key
        assert f"{key} = " in r.stdout
    assert np.isfinite(float(z["prdc_precision"]))
