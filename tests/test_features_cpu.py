"""Host-side checks of the shower-shape observables (no GPU): the fp64 restatement of es_image_features
against the reference's record (tests/golden/image_features.npz), the C ABI entry and its ctypes binding,
the CLI flag, ws_feature_summary and the eval_features configuration.

Bounds: nonzero, center_x, center_y and peak equal the reference exactly (integers, and one fp64 division
of the same integers); max_x / max_y differ from the reference's float32 np.sum by at most the float32
summation bound (h-1) 2^-24 max_j sum_i |v| resp. (w-1) 2^-24 max_i sum_j |v| (feature_refs.max_sum_bounds)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_refs as FR
from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")


@pytest.mark.parametrize("shape", FR.GOLDEN_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_matches_the_reference(shape):
    images, gfeat, _ = FR.golden()[shape]
    assert images.shape == (6, *shape) and images.dtype == np.float32 and gfeat.shape == (5, 6)
    feat, peak = FR.image_features_ref(images)
    FR.assert_matches_golden(feat, peak, shape)


def test_golden_holds_the_edge_images():
    for (h, w), (images, gfeat, gpeak) in FR.golden().items():
        assert not images[0].any() and gfeat[4, 0] == 0 and gfeat[2, 0] == w / 2 and gfeat[3, 0] == h / 2
        assert (images[1] > 0).sum() == 1 and gpeak[1, 0] == h - 1 and gfeat[3, 1] == h - 1
        if h * w >= 2:
            assert (images[2] == images[2].max()).sum() == 2
            first = int(np.flatnonzero(images[2].reshape(-1) == images[2].max())[0])
            assert tuple(gpeak[2]) == (first // w, first % w)
        assert not (images[3] > 0).any() and images[3].sum() < 0 and gfeat[4, 3] == 0 and gfeat[0, 3] <= 0
        assert (images[4:] >= 0).all()
        if h * w >= 1000:
            assert gfeat[4, 4] > gfeat[4, 5] > 0


def test_restatement_sums_sequentially():
    # an image on which the order of an fp64 sum shows (float32 holds 1 and 2^-53 exactly): column 0 is
    # (1 + 2^-53) + 2^-53 = 1 top to bottom (each add ties to even) but 1 + 2^-52 bottom to top; row 1 is
    # (2^-53 + 2^-53) + 1 = 1 + 2^-52 left to right but 1 right to left
    img = np.zeros((1, 3, 3), dtype=np.float32)
    img[0, :, 0] = [1.0, 2.0 ** -53, 2.0 ** -53]
    img[0, 1, :] = [2.0 ** -53, 2.0 ** -53, 1.0]
    feat, peak = FR.image_features_ref(img)
    assert feat[0, 0] == 1.0
    assert feat[0, 1] == 1.0 + 2.0 ** -52
    assert tuple(peak[0]) == (0, 0)                # 1.0 at (0, 0) and at (1, 2): the first wins


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_es_image_features():
    args = _prototype("es_image_features")
    assert args == ["const es_view_t* x", "es_dtype_t dt", "const void* xp", "int log_domain", "double* feat",
                    "int32_t* peak", "es_stream_t stream"]
    src = open(HEADER).read()
    assert "train/utils.py:81-112" in src
    doc = src[src.index("Shower-shape observables"):src.index("int es_image_features")]
    assert "must not be NaN" in doc


def test_binding_matches_the_header_arity():
    from expertsim import hip
    res, args = hip._SIGS["es_image_features"]
    assert res is C.c_int and len(args) == len(_prototype("es_image_features"))
    assert hasattr(hip.lib(), "es_image_features")


def test_entry_rejects_bad_arguments_before_any_launch():
    # argument errors return before the first HIP call, so they can be checked without a device
    from expertsim import hip
    v = hip.make_view((2, 1, 4, 4), (16, 16, 4, 1), False)
    fake = C.c_void_p(256)
    for bad, kw in (((2, 1, 65, 4), {}), ((2, 1, 4, 65), {}), ((2, 2, 4, 4), {}), ((2, 1, 0, 4), {})):
        b = hip.make_view(bad, (bad[2] * bad[3], bad[2] * bad[3], bad[3], 1), False)
        with pytest.raises(hip.HipError):
            hip.call("es_image_features", C.byref(b), hip.ES_F32, fake, 0, fake, fake, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_features", C.byref(v), hip.ES_F32, fake, 0, None, None, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_features", C.byref(v), hip.ES_F32, None, 0, fake, fake, None)
    with pytest.raises(hip.HipError):
        hip.call("es_image_features", None, hip.ES_F32, fake, 0, fake, fake, None)
    empty = hip.make_view((0, 1, 4, 4), (16, 16, 4, 1), False)
    assert hip.call("es_image_features", C.byref(empty), hip.ES_F32, fake, 0, fake, fake, None) == 0


def test_cli_knows_features_default_off():
    import cli
    assert cli.parse_args([]).features is False
    assert cli.parse_args(["--simulate"]).features is False
    assert cli.parse_args(["--simulate", "--features"]).features is True


def test_feature_names_and_summary():
    from expertsim.train.utils import FEATURE_NAMES, ws_feature_summary
    assert FEATURE_NAMES == ("max_x", "max_y", "center_x", "center_y", "nonzero")
    ws = np.zeros((2, 3, 5))
    ws[0, 0] = [1.0, 10.0, 100.0, 1000.0, 10000.0]
    ws[1, 0] = [3.0, 30.0, 300.0, 3000.0, 30000.0]
    ws[0, 1] = [2.0, 0.0, 0.0, 0.0, 8.0]
    ws[1, 1] = [4.0, 0.0, 0.0, 0.0, 0.0]
    ws[0, 2] = [0.5, 1.5, 2.5, 3.5, 4.5]
    ws[1, 2] = [0.5, 1.5, 2.5, 3.5, 4.5]
    mean, std, exp = ws_feature_summary(ws)
    assert mean.shape == (5,) and std.shape == (5,) and exp.shape == (2, 5)
    assert np.array_equal(mean, [2.0, 20.0, 200.0, 2000.0, 20000.0])
    assert np.array_equal(std, [1.0, 10.0, 100.0, 1000.0, 10000.0])
    assert np.array_equal(exp[0], [3.0, 0.0, 0.0, 0.0, 4.0])
    assert np.array_equal(exp[1], [0.5, 1.5, 2.5, 3.5, 4.5])
    with pytest.raises(ValueError):
        ws_feature_summary(np.zeros((2, 1, 5)))
    with pytest.raises(ValueError):
        ws_feature_summary(np.zeros((3, 5)))


def test_eval_features_defaults_off_and_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    assert load_config().train.get("eval_features", None) is False
    cfg = load_config(overrides=["train.eval_features=true"])
    assert cfg.train.eval_features is True and not cfg.train.eval_on_device

    class Loader:
        def __iter__(self):
            raise AssertionError("the loader was read before the configuration was checked")

    with pytest.raises(ValueError, match="eval_on_device"):
        evaluate_epoch(None, Loader(), 0, cfg, "cpu")
