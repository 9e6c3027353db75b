"""CPU half of the sliced Wasserstein distance (expertsim/train/sliced.py): the numpy restatement against the committed
record, the bound helpers against numpy's own fp64 product, the host half `summary`, the argument checks that run
before any launch, and the no-fallback rule."""
import numpy as np
import pytest
import torch

import sliced_refs as R


@pytest.mark.parametrize("shape", R.RECORD_SHAPES)
def test_restatement_reproduces_the_record(shape):
    h, w = shape
    g = R.golden()
    key = f"c{h}x{w}"
    theta, table, summ, counts, _ = R.record_case(h, w)
    assert g[f"{key}_theta16"].dtype == np.float16 and np.array_equal(g[f"{key}_theta16"].astype(np.float64), theta)
    assert g[f"{key}_w"].shape == (R.RECORD_E + 1, R.RECORD_P)
    assert np.array_equal(g[f"{key}_w"], table)                                    # scipy's table, to the bit
    assert np.array_equal(g[f"{key}_counts"], counts)
    want = g[f"{key}_summary"]
    assert np.array_equal(np.isnan(want), np.isnan(summ)) and np.isnan(want[:, 2]).all()
    live = ~np.isnan(want)
    err = np.abs(summ[live] - want[live]) / np.abs(want[live])
    print(f"{key}: worst summary error {err.max() / R.U:.3g} u of 4 u allowed")
    assert (err <= 4 * R.U).all()
    norms = np.sqrt((theta * theta).sum(axis=1))
    assert np.abs(norms - 1).max() <= 2.0 ** -11


@pytest.mark.parametrize("shape", [(1, 1), (6, 5), (44, 44)])
def test_projection_bound_holds_for_numpy_own_product(shape):
    h, w = shape
    x, theta = R.images(h, w, 65), R.normal_theta(17, h * w)
    ref, absum = R.project_ref(x, theta)
    got = x.reshape(65, -1).astype(np.float64) @ theta.T
    bound = R.project_bound(h * w, absum)
    err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
    worst = float((err / np.where(bound > 0, bound, 1.0)).max())
    print(f"numpy fp64 product {shape}: worst error / bound {worst:.3g}")
    assert (err <= bound).all()
    assert (bound[x.reshape(65, -1).any(axis=1)] > 0).all() and (got[1] == 0).all()   # image 1 is all zero


def test_direction_bound_holds_for_numpy_own_normalisation():
    rng = np.random.default_rng(5)
    for d in (1, 5, 30, 1936):
        draws = rng.standard_normal((8, d + d % 2)).astype(np.float32)
        ref = R.directions_ref(draws, d)
        v = draws[:, :d].astype(np.float64)
        got = v / np.sqrt((v * v).sum(axis=1, keepdims=True))
        err = np.abs((got.astype(np.longdouble) - ref).astype(np.float64))
        bound = R.direction_bound(d, ref)
        print(f"numpy fp64 normalisation d={d}: worst error / bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all()


def test_summary_nan_rules_and_values():
    from expertsim.train.sliced import summary
    rng = np.random.default_rng(3)
    w = np.abs(rng.standard_normal((4, 16)))
    w[2] = 0.0                                                                     # what the kernel writes there
    counts = np.array([[50, 50], [49, 49], [0, 0], [1, 1]])
    moments = np.stack([w.mean(axis=1), w.var(axis=1, ddof=1)])
    got = summary(moments, w.max(axis=1), counts, 16)
    want = R.summary_ref(w, counts)
    assert set(got) == {f"{n}{s}" for n in ("swd", "swd_err", "swd_max") for s in ("", "_0", "_1", "_2")}
    for i, name in enumerate(("swd", "swd_err", "swd_max")):
        assert got[name] == want[i, 0] and got[f"{name}_0"] == want[i, 1] and got[f"{name}_2"] == want[i, 3]
        assert np.isnan(got[f"{name}_1"])                                          # empty: NaN, not the kernel's 0
    one_sided = summary(moments, w.max(axis=1), np.array([[50, 0], [0, 3], [1, 1], [1, 1]]), 16)
    assert np.isnan(one_sided["swd"]) and np.isnan(one_sided["swd_max_0"]) and np.isfinite(one_sided["swd_1"])
    single = summary(np.array([[0.5], [np.nan]]), np.array([0.5]), np.array([[9, 9]]), 1, per_expert=False)
    assert single == pytest.approx({"swd": 0.5, "swd_err": np.nan, "swd_max": 0.5}, nan_ok=True)
    assert np.isnan(single["swd_err"]) and set(single) == {"swd", "swd_err", "swd_max"}


def test_problem_count_check():
    from expertsim.train.sliced import check_problems
    check_problems(4, 256)
    check_problems(1, 1024)
    check_problems(32, 1)
    with pytest.raises(ValueError, match="segments"):
        check_problems(33, 1)
    with pytest.raises(ValueError, match="65535"):
        check_problems(65, 1024)
    with pytest.raises(ValueError, match="65535"):
        check_problems(64, 1024)                         # 65536
    with pytest.raises(ValueError, match="n_proj"):
        check_problems(1, 1025)
    with pytest.raises(ValueError, match="n_proj"):
        check_problems(1, 0)


def test_eval_sliced_needs_eval_on_device():
    from expertsim.config import load_config
    from expertsim.train.loop import evaluate_epoch
    cfg = load_config()
    assert cfg.train.eval_sliced is False and cfg.train.eval_sliced_proj == 256
    cfg = load_config(overrides=["train.eval_sliced=true"])

    class Moe:
        n_experts = 1

        def eval(self):
            raise AssertionError("the check comes before the model is touched")
    with pytest.raises(ValueError, match="train.eval_sliced needs train.eval_on_device"):
        evaluate_epoch(Moe(), [], 0, cfg, torch.device("cpu"))


def test_no_cpu_fallback():
    from expertsim import hip
    from expertsim.train import sliced as S
    x = torch.zeros(4, 3, 3)
    theta = torch.zeros(2, 9, dtype=torch.float64)
    for call in (lambda: S.directions(4, 9, device="cpu") if not torch.cuda.is_available() else S.project(x, theta),
                 lambda: S.project(x, theta), lambda: S.sliced_device(x, x), lambda: S.sliced(x, x, n_proj=4),
                 lambda: S.sliced(x, x, directions=theta)):
        with pytest.raises(hip.HipError):
            call()
    assert S.SLICED_STREAM not in (0x51D00001, 0x51D00002)
    from expertsim.models.moe import MoEWrapper
    assert S.SLICED_STREAM not in (MoEWrapper.SIM_NOISE_STREAM, MoEWrapper.SIM_GUMBEL_STREAM)
