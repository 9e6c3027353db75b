"""Dataset preparation on the GPU: es_group_diversity and es_image_sum_peak against their numpy restatement
(tests/prepare_refs.py) and the pandas / numpy record (tests/golden/prepare_*.npz), then prepare_dataset,
write_dataset, the pickle data source and ``cli.py --prepare``.

Tolerances: the kernels' arithmetic order is fixed (include/expertsim_hip.h), so pix_var, group_sum and the
photon sums are compared with the restatement bit for bit (fp64 +, -, *, / and sqrt are correctly rounded on
the device as in numpy) and the peaks exactly; against the record group_sum holds
(2 n_g + h w + 16) 2^-53 relative and photon_sum h w 2^-53 relative (prepare_refs); std = group_sum / max is a
quotient of two such numbers: the sum of their bounds plus one rounding."""
import ctypes as C
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import prepare_refs as PR
from conftest import REPO

pytestmark = pytest.mark.gpu
DEV = "cuda"
# group sizes: empty, one member, the register path (<= 8) and the chain above it, around 16 and the wave width,
# and both sides of the split of a large group (256 | 257)
SIZES = (1, 0, 2, 3, 8, 9, 16, 17, 64, 65, 256, 257)
# 6x5: an odd width with an even pixel count (dense images are read in pairs across row ends); 1x1: a pixel
# without a neighbour; the "window" layout has odd strides and takes the scalar loads
SHAPES = [(1, 1), (6, 5), (44, 44), (56, 30), (64, 64)]
ZDCS = ("neutron", "proton")


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _raw(x, perm, offs, maps=True):
    from expertsim.utils.data_preparation import diversity_raw
    dev = lambda a: torch.from_numpy(np.array(a, dtype=np.int32)).to(DEV)
    gs, pv = diversity_raw(x, dev(perm), dev(offs), len(offs) - 1, maps)
    return gs.cpu().numpy(), (pv.cpu().numpy() if maps else None)


def _layouts(x_host, layout):
    t = torch.from_numpy(np.array(x_host))
    n, h, w = t.shape
    if layout == "dense":
        return t.to(DEV)
    if layout == "second":          # every second image of a larger buffer; the others would change every result
        buf = torch.full((2 * n, h, w), 1e30, dtype=t.dtype, device=DEV)
        xd = buf[::2]
        xd.copy_(t)
        assert xd.stride(0) == 2 * h * w
        return xd
    buf = torch.full((n, h + 3, w + 5), 1e30, dtype=t.dtype, device=DEV)   # a window of a wider buffer
    xd = buf[:, 1:1 + h, 2:2 + w]
    xd.copy_(t)
    return xd


# ------------------------------------------------------------------------ 1.-3. kernel = restatement
@pytest.mark.parametrize("layout", ["dense", "second", "window"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_diversity_equals_restatement(shape, dtype, layout):
    h, w = shape
    x, group, perm, offs, gs_ref, pv_ref = PR.case(h, w, SIZES, 0, dtype)
    assert not np.array_equal(perm, np.arange(len(perm)))
    gs, pv = _raw(_layouts(x, layout), perm, offs)
    assert np.array_equal(_bits(pv), _bits(pv_ref)), (shape, dtype, layout)
    same = np.array_equal(_bits(gs), _bits(gs_ref))
    err = np.abs(gs - gs_ref) / np.where(gs_ref > 0, gs_ref, 1.0)
    print(f"{shape} {dtype} {layout}: group_sum bitwise equal to the restatement: {same}; worst rel {err.max():.3e}")
    assert (err <= PR.group_sum_bound(np.diff(offs), h * w)).all()
    assert same
    for g in (0, 1):                                   # one member, no member: exactly +0.0
        assert gs[g] == 0.0 and not np.signbit(gs[g]) and not pv[g].any()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("zdc", ZDCS)
def test_diversity_matches_the_record(zdc, dtype):
    g, r = PR.golden(zdc), PR.golden_ref(zdc, dtype)
    h, w = g["images"].shape[1:]
    gs, pv = _raw(torch.from_numpy(np.array(g["images"], dtype=dtype)).to(DEV), r["perm"], r["offs"])
    assert np.array_equal(_bits(pv), _bits(r["pix_var"]))
    assert np.array_equal(_bits(gs), _bits(r["group_sum"]))
    zero = g["group_sum"] == 0.0                       # two one-member groups and the identical-images group
    assert zero.sum() == 3 and np.array_equal(gs == 0.0, zero) and not np.signbit(gs).any()
    if dtype == "float64":
        bound = PR.group_sum_bound(r["counts"], h * w)
        err = np.abs(gs - g["group_sum"]) / np.where(zero, 1.0, g["group_sum"])
        print(f"{zdc}: worst group_sum error / bound against the record {(err / bound).max():.4f}")
        assert (err <= bound).all()


def test_large_and_overlapping_groups():
    # 5000 members: chunks of 313; offs that run backwards give an empty group and two groups over the same
    # rows, more large groups than n / 257 (the large-group launch then sweeps its list twice)
    rng = np.random.default_rng(11)
    x = np.log1p(rng.poisson(2.0, size=(5000, 4, 5)) * rng.random((5000, 4, 5)))
    perm = rng.permutation(5000).astype(np.int32)
    gs_ref, pv_ref = PR.group_diversity_ref(x, perm, [0, 5000])
    gs, pv = _raw(torch.from_numpy(x).to(DEV), perm, np.array([0, 5000], dtype=np.int32))
    assert np.array_equal(_bits(pv), _bits(pv_ref)) and np.array_equal(_bits(gs), _bits(gs_ref))
    offs = np.array([0, 300, 0, 300, 7000, -5], dtype=np.int32)
    gs_ref, pv_ref = PR.group_diversity_ref(x[:300], perm[:300] % 300, offs)
    gs, pv = _raw(torch.from_numpy(x[:300]).to(DEV), perm[:300] % 300, offs)
    assert np.array_equal(_bits(pv), _bits(pv_ref)) and np.array_equal(_bits(gs), _bits(gs_ref))
    assert gs[0] == gs[2] > 0 and gs[1] == 0.0 and gs[3] == 0.0 and gs[4] == 0.0
    # row indices outside [0, n) are clamped
    wild = np.array([-4, 0, 1, 2, 99, 299, 300, 2 ** 30], dtype=np.int32)
    gs_ref, pv_ref = PR.group_diversity_ref(x[:300], wild, [0, 8])
    gs, pv = _raw(torch.from_numpy(x[:300]).to(DEV), np.concatenate([wild, np.zeros(292, dtype=np.int32)]),
                  np.array([0, 8], dtype=np.int32))
    assert np.array_equal(_bits(pv), _bits(pv_ref)) and np.array_equal(_bits(gs), _bits(gs_ref))


# ----------------------------------------------------------- 4.-5. independence and reproducibility
def test_group_result_does_not_depend_on_the_rest():
    x, group, perm, offs, gs_ref, pv_ref = PR.case(44, 44, SIZES, 0, "float64")
    xd = torch.from_numpy(np.array(x)).to(DEV)
    gs, pv = _raw(xd, perm, offs)
    again, pv2 = _raw(xd, perm, offs)
    assert np.array_equal(_bits(gs), _bits(again)) and np.array_equal(_bits(pv), _bits(pv2))      # a rerun
    for g in (3, 5, 7, 9, 11):                         # alone, among fewer images, in another position
        rows = np.flatnonzero(group == g)
        alone_gs, alone_pv = _raw(torch.from_numpy(x[rows]).to(DEV), np.arange(len(rows), dtype=np.int32),
                                  np.array([0, len(rows)], dtype=np.int32))
        assert np.array_equal(_bits(alone_gs), _bits(gs[g:g + 1])) and np.array_equal(_bits(alone_pv), _bits(pv[g:g + 1]))
    # more images and more groups around the same groups: n grows, the results stay
    more = torch.cat([torch.zeros(100, 44, 44, dtype=torch.float64, device=DEV), xd,
                      torch.rand(50, 44, 44, dtype=torch.float64, device=DEV)])
    perm2 = np.concatenate([np.arange(100), perm + 100, np.arange(50) + 100 + len(perm)]).astype(np.int32)
    offs2 = np.concatenate([[0, 40], offs + 100, [offs[-1] + 150]]).astype(np.int32)
    gs2, pv2 = _raw(more, perm2, offs2)
    assert np.array_equal(_bits(gs2[2:-1]), _bits(gs)) and np.array_equal(_bits(pv2[2:-1]), _bits(pv))
    assert gs2[0] == 0.0 and gs2[1] == 0.0 and gs2[-1] > 0.0


# ------------------------------------------------------------------------------ 6. sums and peaks
def _sum_peak_raw(x, s, p):
    from expertsim import hip
    n, h, w = x.shape
    v = hip.make_view((n, 1, h, w), (x.stride(0), h * w, x.stride(1), x.stride(2)), False)
    return hip.call("es_image_sum_peak", C.byref(v), 1 if x.dtype == torch.float64 else 0, hip.ptr(x), hip.ptr(s),
                    hip.ptr(p), hip.stream_ptr())


@pytest.mark.parametrize("layout", ["dense", "second", "window"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", SHAPES + [(7, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_sum_peak_equals_restatement(shape, dtype, layout):
    from expertsim.utils.data_preparation import photon_sums_and_peaks
    h, w = shape
    for n in (1, 9):                                   # 9: two full workgroups of four images and one with one
        rng = np.random.default_rng(100 * h + w + n)
        x = (np.log1p(rng.poisson(3.0, size=(n, h, w)) * rng.random((n, h, w))) - 0.25).astype(dtype)
        if n > 3 and h * w >= 2:                       # a doubled maximum: the first wins
            a, b = sorted(rng.choice(h * w, size=2, replace=False))
            x[3].reshape(-1)[[a, b]] = x[3].max() + 1.0
        s_ref, p_ref = PR.image_sum_peak_ref(x)
        am = x.reshape(n, -1).argmax(axis=1)
        assert np.array_equal(p_ref, np.stack(np.unravel_index(am, (h, w)), axis=1))
        s, p = photon_sums_and_peaks(_layouts(x, layout))
        assert s.dtype == torch.float64 and p.dtype == torch.int32 and s.is_cuda and p.shape == (n, 2)
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(s_ref)), (shape, dtype, layout, n)
        assert np.array_equal(p.cpu().numpy(), p_ref), (shape, dtype, layout, n)


@pytest.mark.parametrize("zdc", ZDCS)
def test_sum_peak_matches_the_record(zdc):
    from expertsim.utils.data_preparation import photon_sums_and_peaks
    g, r = PR.golden(zdc), PR.golden_ref(zdc)
    h, w = g["images"].shape[1:]
    s, p = photon_sums_and_peaks(g["images"])          # host input: copied to the device
    s, p = s.cpu().numpy(), p.cpu().numpy()
    assert np.array_equal(_bits(s), _bits(r["sum"]))
    assert np.array_equal(p[:, 0], g["max_x"]) and np.array_equal(p[:, 1], g["max_y"])
    assert (np.abs(s - g["photon_sum"]) <= h * w * PR.U * g["photon_sum"]).all()


def test_sum_peak_outputs_alone_and_errors():
    from expertsim import hip
    from expertsim.utils import data_preparation as DP
    x = torch.rand(5, 7, 5, dtype=torch.float64, device=DEV)
    s_ref, p_ref = PR.image_sum_peak_ref(x.cpu().numpy())
    s = torch.full((5,), -7.0, dtype=torch.float64, device=DEV)
    p = torch.full((5, 2), -7, dtype=torch.int32, device=DEV)
    _sum_peak_raw(x, s, None)
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(s_ref)) and bool((p == -7).all())
    s.fill_(-7.0)
    _sum_peak_raw(x, None, p)
    assert np.array_equal(p.cpu().numpy(), p_ref) and bool((s == -7.0).all())
    p.fill_(-7)
    with pytest.raises(hip.HipError, match="both outputs"):
        _sum_peak_raw(x, None, None)
    with pytest.raises(hip.HipError, match="es_image_sum_peak failed"):
        _sum_peak_raw(torch.zeros(2, 65, 64, device=DEV), s, p)
    torch.cuda.synchronize()
    assert bool((s == -7.0).all()) and bool((p == -7).all())
    s0, p0 = DP.photon_sums_and_peaks(torch.empty(0, 4, 4, device=DEV))
    assert s0.shape == (0,) and p0.shape == (0, 2)
    gs0, _ = DP.diversity_raw(torch.empty(0, 4, 4, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                              torch.zeros(3, dtype=torch.int32, device=DEV), 2)
    assert gs0.shape == (2,) and not gs0.any()


def test_non_finite_pixels_and_singleton_groups(caplog):
    from expertsim.utils import data_preparation as DP
    x = np.random.default_rng(2).random((12, 6, 5))
    group = np.arange(12) // 3
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 2, 3] = bad
        y[9, 0, 0] = bad
        with pytest.raises(ValueError, match="image 7"):
            DP.photon_sums_and_peaks(y)
        with pytest.raises(ValueError, match="image 7"):
            DP.diversity(y, group, 4)
    std, gs = DP.diversity(x.astype(np.float32), group, 4)
    assert std.shape == (12,) and float(std.max()) == 1.0 and float(std.min()) > 0.0
    with caplog.at_level(logging.WARNING):
        std, gs = DP.diversity(x, np.arange(12), 12)       # pandas: 0 / 0 = NaN
    assert not std.any() and not gs.any() and "NaN" in caplog.text
    std, gs, maps = DP.diversity(x, group, 4, return_maps=True)
    want = np.stack([x[group == g].reshape(3, -1).var(axis=0) for g in range(4)])
    assert maps.shape == (4, 30) and np.allclose(maps.cpu().numpy(), want, rtol=1e-13, atol=0.0)


# ------------------------------------------------------------------------------------ 7. end to end
def _cfg(zdc, paths, tmp, shape):
    from expertsim.config import AttrDict as A
    return A(limit_samples=None, config=A(run_name="t", experiment_dir=str(tmp / "exp")), model=A(architecture=zdc),
             dataset=A(zdc_type=zdc, source="pickle", MIN_INTENSITY_THRESHOLD=None, MAX_INTENSITY_THRESHOLD=None,
                       read_n_samples=None, shuffle_train_test_split=False, test_size=0.2, resident=True,
                       input_image_shape=list(shape), **paths),
             train=A(save_experiments_dir=str(tmp), checkpoint_experiment_dir=None, epoch_to_load=None,
                     save_experiment_data=False, batch_size=16))


@pytest.mark.parametrize("zdc", ZDCS)
def test_prepare_dataset_end_to_end(tmp_path, zdc):
    pd = pytest.importorskip("pandas")
    from expertsim.utils import data_preparation as DP
    from expertsim.utils import data_transformations as DT
    g, r = PR.golden(zdc), PR.golden_ref(zdc)
    h, w = g["images"].shape[1:]
    frame = pd.DataFrame(g["cond"], columns=DT.COND_COLUMNS)
    images, cond, pos = DP.prepare_dataset(g["images"], frame, zdc)
    sfx = "_proton" if zdc == "proton" else ""
    assert images.shape == g["images"].shape and list(cond.columns[:9]) == DT.COND_COLUMNS
    assert np.array_equal(cond["group_number" + sfx], g["group_number"])
    assert np.array_equal(pos["max_x"], g["max_x"]) and np.array_equal(pos["max_y"], g["max_y"])
    ps = cond[f"{zdc}_photon_sum"].to_numpy()
    assert (np.abs(ps - g["photon_sum"]) <= h * w * PR.U * g["photon_sum"]).all()
    bound = PR.group_sum_bound(r["counts"], h * w)
    std = cond["std" + sfx].to_numpy()
    tol = (bound[g["group_number"]] + bound[np.argmax(g["group_sum"])] + 2.0 * PR.U) * g["std"]
    assert (np.abs(std - g["std"]) <= tol).all() and np.array_equal(std == 0.0, g["std"] == 0.0) and std.max() == 1.0
    # the photon-sum filter comes first: the groups and the normalisation are those of the kept samples
    lo, hi = np.quantile(g["photon_sum"], [0.1, 0.9])
    keep = (ps >= lo) & (ps <= hi)
    im2, cond2, pos2 = DP.prepare_dataset(torch.from_numpy(np.array(g["images"])).to(DEV), frame, zdc, lo, hi)
    assert len(im2) == len(cond2) == len(pos2) == int(keep.sum()) < len(ps)
    assert np.array_equal(im2, g["images"][keep]) and np.array_equal(cond2[f"{zdc}_photon_sum"], ps[keep])
    grp2, n2 = DP.group_numbers(g["cond"][keep])
    assert np.array_equal(cond2["group_number" + sfx], grp2)
    ref2, _ = PR.group_diversity_ref(g["images"][keep], *PR.layout(grp2, n2))
    assert np.array_equal(cond2["std" + sfx], (ref2 / ref2.max())[grp2])
    # the files feed the pickle data source
    paths = DP.write_dataset(tmp_path / "data", zdc, images, cond, pos)
    cfg = _cfg(zdc, paths, tmp_path, (h, w))
    np.random.seed(0)
    tr, te = DT.get_train_test_data_loaders(cfg)
    batch = next(iter(tr))
    assert len(batch) == 6 and batch[0].shape == (16, h, w) and batch[0].is_cuda and batch[0].dtype == torch.float32
    assert batch[2].shape == (16, 9) and batch[3].shape == (16, 1) and batch[5].shape == (16, 2)
    assert float(batch[3].min()) >= 0.0 and float(batch[3].max()) <= 1.0
    assert len(tr.tensors[0]) + len(te.tensors[0]) == len(images)


# ------------------------------------------------------------------------------------------- 8. CLI
def test_cli_prepare(tmp_path):
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(8)
    counts = rng.poisson(4.0, size=(64, 44, 44)).astype(np.float32)        # raw photon counts
    cond = np.repeat(rng.integers(0, 3, size=(16, 9)).astype(np.float64), 4, axis=0)
    cond[:, 0] += np.repeat(np.arange(16), 4) * 10.0                       # 16 distinct rows of 4 samples
    np.save(tmp_path / "counts.npy", counts)
    np.save(tmp_path / "cond.npy", cond)
    out = tmp_path / "prepared"
    r = subprocess.run([sys.executable, os.path.join(REPO, "cli.py"), "-o", "dataset.zdc_type=neutron", "--prepare",
                        "--raw", "--images", str(tmp_path / "counts.npy"), "--conditions", str(tmp_path / "cond.npy"),
                        "--out-dir", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Prepared 64 neutron samples in " in r.stdout and "group-size quartiles" in r.stdout
    assert f"dataset.DATA_COND_PATH={out}" in r.stdout
    files = sorted(os.listdir(out))
    assert len(files) == 3
    from expertsim.utils import data_preparation as DP
    frames = {}
    for line in r.stdout.splitlines():
        if "Wrote " in line:
            for kv in line.split("Wrote ")[1].split():
                k, v = kv.split("=", 1)
                frames[k] = pd.read_pickle(v)
    images, cf, pf = (frames[f"dataset.DATA_{k}_PATH"] for k in ("IMAGES", "COND", "POSITIONS"))
    x = np.log1p(counts.astype(np.float64))
    assert np.array_equal(np.asarray(images), x)
    grp, n_groups = DP.group_numbers(cond)
    assert np.array_equal(cf["group_number"], grp) and f"in {n_groups} groups" in r.stdout
    gs, _ = PR.group_diversity_ref(x, *PR.layout(grp, n_groups))
    s, p = PR.image_sum_peak_ref(x)
    assert np.array_equal(cf["std"], (gs / gs.max())[grp]) and np.array_equal(cf["neutron_photon_sum"], s)
    assert np.array_equal(pf[["max_x", "max_y"]].to_numpy(), p)
