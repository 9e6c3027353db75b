"""Host-side checks of the dataset preparation (no GPU): the C ABI entries and their ctypes bindings, the
argument checks that return before any launch, the numpy restatement of the kernels (tests/prepare_refs.py)
against the pandas / numpy record (tests/golden/prepare_*.npz), group_numbers against pandas, the CLI flags
and the frames `prepare_dataset` assembles against the pickle data source.

Bounds (tests/prepare_refs.py): group_number, the peaks and the zeros exactly; group_sum within
(2 n_g + h w + 16) 2^-53 relative; photon_sum within h w 2^-53 relative."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prepare_refs as PR
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
ZDCS = ("neutron", "proton")
SHAPE = {"neutron": (44, 44), "proton": (56, 30)}


def _prototype(name, res="int"):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b%s\s+%s\s*\(([^;]*)\)\s*;" % (res, name), src)
    assert m, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------ 1. ABI
def test_header_declares_the_entries():
    assert _prototype("es_group_diversity") == [
        "const es_view_t* x", "int x_f64", "const void* xp", "const int32_t* perm", "const int32_t* offs",
        "int n_groups", "double* group_sum", "double* pix_var", "void* work", "size_t work_bytes",
        "es_stream_t stream"]
    assert _prototype("es_image_sum_peak") == ["const es_view_t* x", "int x_f64", "const void* xp", "double* sum",
                                               "int32_t* peak", "es_stream_t stream"]
    assert _prototype("es_group_diversity_workspace", "size_t") == ["int n_groups", "int h", "int w"]
    src = open(HEADER).read()
    doc = src[src.index("Dataset preparation"):src.index("int es_image_sum_peak")]
    for words in ("Values must be finite", "ddof = 0", "no float atomics", "ES_PREP_SPLIT_MIN", "ES_PREP_CHUNKS"):
        assert words in doc, words


def test_bindings_match_the_header():
    from expertsim import hip
    for name, res in (("es_group_diversity", "int"), ("es_image_sum_peak", "int"),
                      ("es_group_diversity_workspace", "size_t")):
        r, args = hip._SIGS[name]
        assert r is (C.c_int if res == "int" else C.c_size_t) and len(args) == len(_prototype(name, res)), name
        assert hasattr(hip.lib(), name)
    src = open(HEADER).read()
    assert int(re.search(r"#define ES_PREP_SPLIT_MIN (\d+)", src).group(1)) == hip.PREP_SPLIT_MIN == PR.SPLIT_MIN
    assert int(re.search(r"#define ES_PREP_CHUNKS (\d+)", src).group(1)) == hip.PREP_CHUNKS == PR.CHUNKS


def test_workspace_size():
    from expertsim import hip
    ws = hip.lib().es_group_diversity_workspace
    assert ws(0, 44, 44) == 0 and ws(5, 0, 44) == 0 and ws(5, 65, 64) == 0 and ws(-1, 4, 4) == 0
    # tile partials [G][ceil(hw / 128)] fp64 + the list of large groups [G] int32 + its length
    assert ws(5, 44, 44) == 5 * 16 * 8 + 5 * 4 + 8
    assert ws(3, 1, 1) == 3 * 8 + 3 * 4 + 8
    assert ws(1, 64, 64) == 32 * 8 + 4 + 8


# ------------------------------------------------------------------- 2. argument errors, no device
def _view(dims):
    from expertsim import hip
    return hip.make_view(dims, (dims[2] * dims[3], dims[2] * dims[3], dims[3], 1), False)


def test_group_diversity_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)
    big = 1 << 20

    def call(v, f64=0, xp=fake, perm=fake, offs=fake, G=2, gs=fake, pv=fake, work=fake, wb=big):
        return hip.call("es_group_diversity", None if v is None else C.byref(v), f64, xp, perm, offs, G, gs, pv,
                        work, wb, None)

    good = _view((4, 1, 4, 4))
    for bad in ((4, 1, 65, 64), (4, 1, 1, 4097), (4, 2, 4, 4), (4, 1, 0, 4), (4, 1, 4, 0), (-1, 1, 4, 4)):
        with pytest.raises(hip.HipError):
            call(_view(bad))
    for kw in (dict(xp=None), dict(perm=None), dict(offs=None), dict(gs=None), dict(f64=2), dict(f64=-1),
               dict(G=-1), dict(work=None), dict(wb=0), dict(wb=2 * 8 + 2 * 4 + 8 - 1)):
        with pytest.raises(hip.HipError):
            call(good, **kw)
    with pytest.raises(hip.HipError):
        call(None)
    with pytest.raises(hip.HipError, match="workspace"):
        call(good, wb=8)
    # nothing to do: ES_OK without a launch (and without a workspace)
    assert call(_view((0, 1, 4, 4)), work=None, wb=0) == 0
    assert call(good, G=0, work=None, wb=0) == 0


def test_image_sum_peak_rejects_bad_arguments_before_any_launch():
    from expertsim import hip
    fake = C.c_void_p(256)
    good = _view((2, 1, 4, 4))
    for bad in ((2, 1, 65, 64), (2, 1, 4097, 1), (2, 2, 4, 4), (2, 1, 0, 4), (-1, 1, 4, 4)):
        with pytest.raises(hip.HipError):
            hip.call("es_image_sum_peak", C.byref(_view(bad)), 0, fake, fake, fake, None)
    with pytest.raises(hip.HipError, match="both outputs"):
        hip.call("es_image_sum_peak", C.byref(good), 0, fake, None, None, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_sum_peak", C.byref(good), 0, None, fake, fake, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_sum_peak", None, 0, fake, fake, fake, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_sum_peak", C.byref(good), 2, fake, fake, fake, None)
    assert hip.call("es_image_sum_peak", C.byref(_view((0, 1, 4, 4))), 1, fake, fake, fake, None) == 0


def test_device_functions_raise_without_a_device(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from expertsim import hip
    from expertsim.utils import data_preparation as DP
    x = np.zeros((2, 4, 4))
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        DP.photon_sums_and_peaks(x)
    with pytest.raises(hip.HipError, match="no CPU fallback"):
        DP.diversity(x, np.zeros(2, dtype=np.int64), 1)


# --------------------------------------------------------------------- 3. restatement = the record
@pytest.mark.parametrize("zdc", ZDCS)
def test_golden_holds_the_required_cases(zdc):
    g = PR.golden(zdc)
    h, w = SHAPE[zdc]
    assert g["images"].shape == (456, h, w) and g["images"].dtype == np.float64 and g["cond"].shape == (456, 9)
    counts = np.bincount(g["group_number"])
    assert sorted(counts.tolist()) == [1, 1, 2, 3, 63, 64, 65, 257]
    assert not np.array_equal(np.sort(g["group_number"]), g["group_number"])           # perm is not the identity
    zero = g["group_sum"] == 0.0
    assert zero.sum() == 3 and sorted(counts[zero].tolist()) == [1, 1, 3]
    same = int(np.flatnonzero(zero & (counts == 3))[0])
    members = g["images"][g["group_number"] == same]
    assert (members == members[0]).all() and members[0].any()
    assert any((img == img.max()).sum() == 2 for img in g["images"])
    assert np.array_equal(g["std"], (g["group_sum"] / g["group_sum"].max())[g["group_number"]])


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("zdc", ZDCS)
def test_restatement_matches_the_record(zdc, dtype):
    g, r = PR.golden(zdc), PR.golden_ref(zdc, dtype)
    h, w = SHAPE[zdc]
    x = g["images"].astype(dtype).astype(np.float64)
    assert np.array_equal(r["counts"], np.bincount(g["group_number"]))
    # the peak is taken in the input's own precision (rounding to float32 may create a tie)
    assert np.array_equal(r["peak"][:, 0] * w + r["peak"][:, 1], g["images"].astype(dtype).reshape(456, -1).argmax(axis=1))
    if dtype == "float64":
        assert np.array_equal(r["peak"][:, 0], g["max_x"]) and np.array_equal(r["peak"][:, 1], g["max_y"])
    # float32 images: the record's definitions on the widened values (numpy, ddof = 0)
    if dtype == "float64":
        want_sum, want_gs = g["photon_sum"], g["group_sum"]
    else:
        want_sum = x.reshape(456, -1).sum(axis=1)
        want_gs = np.array([np.std(x[g["group_number"] == k], axis=0).sum() for k in range(len(r["counts"]))])
    zero = want_gs == 0.0
    assert zero.sum() == 3 and np.array_equal(r["group_sum"] == 0.0, zero)
    assert not np.signbit(r["group_sum"]).any()
    bound = PR.group_sum_bound(r["counts"], h * w)
    err = np.abs(r["group_sum"] - want_gs) / np.where(zero, 1.0, want_gs)
    print(f"{zdc} {dtype}: worst group_sum error / bound {(err / bound).max():.4f}")
    assert (err <= bound).all(), (err, bound)
    serr = np.abs(r["sum"] - want_sum) / want_sum
    print(f"{zdc} {dtype}: worst photon_sum error / bound {(serr / (h * w * PR.U)).max():.4f}")
    assert (serr <= h * w * PR.U).all()


def test_restatement_order():
    # sequential member sums: (1 + 2^-53) + 2^-53 = 1 in member order (each add ties to even), 1 + 2^-52 in
    # the reverse order
    x = np.array([1.0, 2.0 ** -53, 2.0 ** -53]).reshape(3, 1, 1)
    _, var_fwd = PR.group_diversity_ref(x, [0, 1, 2], [0, 3])
    _, var_rev = PR.group_diversity_ref(x, [2, 1, 0], [0, 3])

    def want(m, order):
        q = 0.0
        for v in order:
            d = v - m
            q += d * d
        return q / 3.0

    assert var_fwd[0, 0] == want(1.0 / 3.0, [1.0, 2.0 ** -53, 2.0 ** -53])
    assert var_rev[0, 0] == want((1.0 + 2.0 ** -52) / 3.0, [2.0 ** -53, 2.0 ** -53, 1.0])
    assert var_fwd[0, 0] != var_rev[0, 0]
    # a group above SPLIT_MIN is cut into CHUNKS chunks of ceil(n / CHUNKS): 257 members -> 15 x 17 + 2
    n = PR.SPLIT_MIN + 1
    rng = np.random.default_rng(5)
    col = rng.random(n)
    L = -(-n // PR.CHUNKS)
    S = 0.0
    for c in range(PR.CHUNKS):
        part = 0.0
        for v in col[c * L:(c + 1) * L]:
            part += v
        S += part
    m = S / n
    Q = 0.0
    for c in range(PR.CHUNKS):
        part = 0.0
        for v in col[c * L:(c + 1) * L]:
            d = v - m
            part += d * d
        Q += part
    gs, var = PR.group_diversity_ref(col.reshape(n, 1, 1), np.arange(n), [0, n])
    assert var[0, 0] == Q / n and gs[0] == np.sqrt(Q / n)
    # the butterfly: lane 0 ends with ((a0 + a32) + (a16 + a48)) + ..
    a = rng.random(64)
    t = a.copy()
    for o in (32, 16, 8, 4, 2, 1):
        t = np.array([t[i] + t[i ^ o] for i in range(64)])
    assert PR.butterfly(a) == t[0]
    pairs = np.concatenate([[a[0] + a[1], a[2] + a[3], a[4] + 0.0], np.zeros(61)])
    assert PR.tile_sum(a[:5]) == PR.butterfly(pairs)
    b = rng.random(300)                                # three tiles: 128 + 128 + 44
    tiles = [PR.tile_sum(b[:128]), PR.tile_sum(b[128:256]), PR.tile_sum(b[256:])]
    assert PR.tile_sum(b) == (0.0 + tiles[0] + tiles[1]) + tiles[2]
    # one member, no member, clamped bounds
    gs, var = PR.group_diversity_ref(rng.random((4, 3, 3)), [3, 1, 2, 0], [0, 1, 1, 9])
    assert gs[0] == 0.0 and gs[1] == 0.0 and not var[:2].any() and gs[2] > 0.0


# --------------------------------------------------------------------------------- 4. group_numbers
def test_group_numbers():
    from expertsim.utils import data_preparation as DP
    from expertsim.utils.data_transformations import COND_COLUMNS
    for zdc in ZDCS:
        g = PR.golden(zdc)
        group, n_groups = DP.group_numbers(g["cond"])
        assert group.dtype == np.int64 and n_groups == 8 and np.array_equal(group, g["group_number"])
    rng = np.random.default_rng(3)
    cond = rng.integers(-2, 3, size=(500, 9)).astype(np.float64) * 0.5
    group, n_groups = DP.group_numbers(cond)
    uniq, inv = np.unique(cond, axis=0, return_inverse=True)
    assert n_groups == len(uniq) and np.array_equal(group, inv.reshape(-1))
    try:
        import pandas as pd
    except ImportError:
        pd = None
    if pd is not None:
        want = pd.DataFrame(cond, columns=COND_COLUMNS).groupby(COND_COLUMNS).ngroup().to_numpy()
        assert np.array_equal(group, want)
    assert DP.group_numbers(np.zeros((0, 9)))[1] == 0
    for bad in (np.nan, np.inf, -np.inf):
        c = cond.copy()
        c[17, 4] = bad
        with pytest.raises(ValueError, match="row 17"):
            DP.group_numbers(c)


def test_photon_sum_mask():
    from expertsim.utils.data_preparation import photon_sum_mask
    s = np.array([0.5, 1.0, 2.0, 3.0, 3.5])
    assert photon_sum_mask(s).all()
    assert photon_sum_mask(s, 1.0).tolist() == [False, True, True, True, True]
    assert photon_sum_mask(s, None, 3.0).tolist() == [True, True, True, True, False]
    assert photon_sum_mask(s, 1.0, 3.0).tolist() == [False, True, True, True, False]


def test_cli_knows_prepare():
    import cli
    assert cli.parse_args([]).prepare is False and cli.parse_args(["--simulate"]).prepare is False
    a = cli.parse_args(["--prepare", "--images", "i.npy", "--conditions", "c.pkl", "--raw", "--min-photon-sum", "2",
                        "--max-photon-sum", "9.5", "--out-dir", "d"])
    assert a.prepare and a.raw and (a.images, a.conditions, a.out_dir) == ("i.npy", "c.pkl", "d")
    assert (a.min_photon_sum, a.max_photon_sum) == (2.0, 9.5) and a.cond_columns is None
    with pytest.raises(SystemExit):
        cli.prepare(cli.parse_args(["--prepare", "--images", "i.npy"]))


# ----------------------------------------------------------- 5. assembled frames -> the pickle source
@pytest.mark.parametrize("zdc", ZDCS)
def test_assembled_frames_pass_through_the_pickle_source(tmp_path, zdc):
    pd = pytest.importorskip("pandas")
    pytest.importorskip("sklearn")
    from expertsim.config import AttrDict as A
    from expertsim.utils import data_preparation as DP
    from expertsim.utils import data_transformations as DT
    g, r = PR.golden(zdc), PR.golden_ref(zdc)
    h, w = SHAPE[zdc]
    frame = pd.DataFrame(g["cond"], columns=DT.COND_COLUMNS)
    frame["neutron_photon_sum"] = g["photon_sum"] + 1.0          # the simulation's own sum: kept for neutrons
    # the device functions' results, injected: the restatement's
    std = (r["group_sum"] / r["group_sum"].max())[g["group_number"]]
    cond_out, pos = DP.assemble_frames(frame, zdc, std, g["group_number"], r["sum"], r["peak"])
    if zdc == "neutron":
        assert list(cond_out.columns) == DT.COND_COLUMNS + ["std", "neutron_photon_sum", "group_number"]
        assert np.array_equal(cond_out["neutron_photon_sum"], g["photon_sum"] + 1.0)
    else:
        assert list(cond_out.columns) == DT.COND_COLUMNS + ["std_proton", "proton_photon_sum", "group_number_proton",
                                                            "expert_number"]
        assert np.array_equal(cond_out["proton_photon_sum"], r["sum"]) and not cond_out["expert_number"].any()
    assert list(pos.columns) == ["max_x", "max_y"]
    assert np.array_equal(pos["max_x"], g["max_x"]) and np.array_equal(pos["max_y"], g["max_y"])
    paths = DP.write_dataset(tmp_path / "data", zdc, g["images"], cond_out, pos)
    assert sorted(paths) == ["DATA_COND_PATH", "DATA_IMAGES_PATH", "DATA_POSITIONS_PATH"]
    cfg = A(limit_samples=None, config=A(run_name="t", experiment_dir=str(tmp_path / "exp")),
            model=A(architecture=zdc),
            dataset=A(zdc_type=zdc, source="pickle", MIN_INTENSITY_THRESHOLD=1, MAX_INTENSITY_THRESHOLD=None,
                      read_n_samples=None, shuffle_train_test_split=False, test_size=0.2, resident=False,
                      input_image_shape=[h, w], **paths),
            train=A(save_experiments_dir=str(tmp_path), checkpoint_experiment_dir=None, epoch_to_load=None,
                    save_experiment_data=False, batch_size=16))
    np.random.seed(0)
    data, data_cond, data_posi = DT.get_dataset(cfg)
    keep = cond_out[DT._photon_sum_column(zdc)].to_numpy() >= 1
    assert len(data) == int(keep.sum()) > 400
    out = DT.transform_data_for_training(cfg, data, data_cond, data_posi)
    x_tr, x_te, cond_tr, std_tr, pos_tr = out[0], out[1], out[4], out[6], out[10]
    assert x_tr.shape[1:] == (h, w) and x_tr.dtype == np.float32 and len(x_tr) + len(x_te) == len(data)
    assert cond_tr.shape[1] == 9 and list(out[15]) == DT.COND_COLUMNS
    assert std_tr.min() >= 0.0 and std_tr.max() <= 1.0 and pos_tr.shape[1] == 2
    tr, te = DT.get_train_test_data_loaders(cfg)
    batch = next(iter(tr))
    assert len(batch) == 6 and batch[0].shape == (16, h, w) and batch[2].shape == (16, 9) and batch[5].shape == (16, 2)
