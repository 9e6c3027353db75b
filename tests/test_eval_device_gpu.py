"""Device-side evaluation: ws_across_experts_device / ws_summary against the reference's goldens, and
MoEWrapper.evaluate_device / loop.evaluate_epoch(train.eval_on_device) end to end.

Tolerances: the golden WS means <= 1e-4 relative and their std over repetitions <= 1e-4 x the mean
(test_eval_gpu.py::test_joint_ws_matches_reference's own: the generated sums carry the fp32 conv
error).  Metrics recomputed on the host from the device sums differ from the device's only by the
summation order inside each distance: every distance is within 2 (nu + nv) 2^-52 relative of scipy's
(test_wasserstein_gpu.py) with nu + nv <= 2 N, and a mean of non-negative numbers inherits the largest
relative error of its terms, so the means hold 2 (2 N) 2^-52 relative (the mean's own few roundings,
~1e-16, are far inside); the stds 1e-12 x ws_mean absolute.
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from golden_utils import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = "cuda"


def wasserstein_distance(u, v):
    """scipy's, imported at first use: a module-level scipy import would run at collection, for every
    run of the suite, and its tens of thousands of long-lived objects change when the cyclic garbage
    collector runs in the tests collected before this file."""
    from scipy.stats import wasserstein_distance as ref
    return ref(u, v)


def running_stats(n, expert):
    i = np.arange(n, dtype=np.float64)
    return ((0.1 * np.sin(0.37 * i + expert)).astype(np.float32),
            (0.75 + 0.25 * np.cos(0.11 * i + 2 * expert)).astype(np.float32))


def _set_running_stats(gens):
    with torch.no_grad():
        for e, g in enumerate(gens):
            for m in g.modules():
                if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                    mean, var = running_stats(m.num_features, e)
                    m.running_mean.copy_(torch.from_numpy(mean))
                    m.running_var.copy_(torch.from_numpy(var))


# ------------------------------------------------------------------------------------------ golden
@pytest.mark.parametrize("arch", ["neutron", "proton"])
def test_ws_across_experts_device_matches_reference(arch):
    from expertsim.config import inject_shared, load_config
    from expertsim.models import build_model
    from expertsim.train import utils as U
    z = np.load(os.path.join(GOLDEN_DIR, f"eval_{arch}.npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    cfg = inject_shared(load_config(overrides=[f"model.architecture={arch}", "train.precision=fp32"]))
    torch.manual_seed(meta["seed"])
    g0 = build_model(f"{arch}.generator", cfg.model.generator, DEV)
    gens = [g0, copy.deepcopy(g0)]
    _set_running_stats(gens)
    assign, cond, ch_org = z["assign"], z["cond"], z["ch_org"]
    idx = [np.where(assign == e)[0] for e in range(2)]
    rows, pos = torch.from_numpy(z["ws/noise"]), 0
    R, N = meta["n_calc"], len(assign)
    ch_gen = torch.full((R, N, 5), float("nan"), dtype=torch.float64, device=DEV)
    for j in range(R):                      # the reference's draw order: repetition, expert, batch
        for e, ix in enumerate(idx):
            s = U.generator_channel_sums(1024, len(ix), 10, torch.device(DEV), torch.from_numpy(cond[ix]).to(DEV),
                                         gens[e], input_noise=rows[pos:pos + len(ix)])
            pos += len(ix)
            ch_gen[j, torch.as_tensor(ix, device=DEV)] = s
    assert pos == rows.shape[0] and bool(torch.isfinite(ch_gen).all())
    ws = U.ws_across_experts_device(torch.from_numpy(np.asarray(ch_org, dtype=np.float64)).to(DEV), ch_gen,
                                    torch.from_numpy(assign.astype(np.int32)).to(DEV), 2)
    assert ws.shape == (R, 3, 5) and ws.is_cuda
    m, s, me, se = U.ws_summary(ws.cpu().numpy())
    scale = float(z["ws/mean"])
    np.testing.assert_allclose(m, scale, rtol=1e-4)
    np.testing.assert_allclose(me, z["ws/mean_exp"], rtol=1e-4)
    np.testing.assert_allclose(s, float(z["ws/std"]), rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(se, z["ws/std_exp"], rtol=0, atol=1e-4 * scale)


# -------------------------------------------------------------------------------------- end to end
def _moe(precision="fp32", E=3, extra=()):
    from expertsim.config import load_config
    from expertsim.train.loop import setup_moe_system
    cfg = load_config(overrides=["model.architecture=neutron", "dataset.input_image_shape=[44,44]",
                                 f"model.n_experts={E}", f"train.precision={precision}",
                                 "model.router.diff_strength=1e-6", *extra])
    torch.manual_seed(3)
    moe = setup_moe_system(cfg, torch.device(DEV))
    _set_running_stats(moe.generators)
    moe.eval()
    return moe, cfg


def _batch(n=96):
    from expertsim.utils.synthetic import make_batch
    b = make_batch(n, "neutron", seed=11)
    return b, torch.from_numpy(b["real_images"]), torch.from_numpy(b["cond"]).to(DEV)


def _metric_keys(E):
    return {"ws_mean", "ws_std", *[f"ws_mean_{i}" for i in range(E)], *[f"ws_std_{i}" for i in range(E)], "epoch"}


def _host_metrics(det, E):
    """calculate_joint_ws_across_experts' arithmetic with scipy on the host copies of the device sums."""
    real, gen, expert = (det[k].cpu().numpy() for k in ("sums_real", "sums_gen", "expert"))
    R = gen.shape[0]
    ws, ws_exp = np.zeros((R, 5)), np.zeros((R, E, 5))
    for j in range(R):
        for i in range(5):
            ws[j][i] = wasserstein_distance(real[:, i], gen[j][:, i])
            for e in range(E):
                ix = np.where(expert == e)[0]
                if len(ix) == 0:
                    continue
                ws_exp[j][e][i] = wasserstein_distance(real[ix, i], gen[j][ix, i])
    runs, exp_runs = ws.mean(axis=1), ws_exp.mean(axis=2)
    return runs.mean(), runs.std(), exp_runs.mean(axis=0), exp_runs.std(axis=0)


def test_evaluate_device_end_to_end():
    from expertsim import hip
    E, N, seed = 3, 96, 17
    moe, cfg = _moe("fp32", E)
    moe.eval_batch_size = 48                      # two chunks
    b, x, cond = _batch(N)
    t = lambda k: torch.from_numpy(b[k])
    host = moe.evaluate(7, cond, x, t("true_positions"), t("std"), t("intensity"), cfg, torch.device(DEV))
    plain = moe.evaluate_device(7, cond, x, cfg, seed=seed)
    assert set(plain) == set(host) == _metric_keys(E)
    det = moe.evaluate_device(7, cond, x, cfg, seed=seed, details=True)
    assert set(det) == _metric_keys(E) | {"sums_real", "sums_gen", "expert", "ws"}
    assert det["sums_gen"].shape == (2, N, 5) and det["ws"].shape == (2, E + 1, 5) and det["expert"].shape == (N,)
    assert all(det[k] == plain[k] for k in _metric_keys(E))                # rerun: bitwise
    sim0 = moe.simulate(cond, seed=seed, sums=True)
    assert torch.equal(det["sums_gen"][0], sim0["sums"]) and torch.equal(det["expert"], sim0["expert"])
    noise1 = torch.empty(N, moe.noise_dim, dtype=torch.float32, device=DEV)
    hip.call("es_randn_dev", hip.ptr(noise1), noise1.numel(), seed + 1, moe.SIM_NOISE_STREAM, None, 0, 0,
             hip.stream_ptr())
    sim1 = moe.simulate(cond, seed=seed, noise=noise1, sums=True)
    assert torch.equal(sim1["expert"], sim0["expert"])                     # every repetition routes alike
    assert torch.equal(det["sums_gen"][1], sim1["sums"]) and not torch.equal(sim1["sums"], sim0["sums"])
    m, s, me, se = _host_metrics(det, E)
    rel = 2 * (2 * N) * 2.0 ** -52
    print(f"evaluate_device: ws_mean {det['ws_mean']!r} host {m!r}; ws_std {det['ws_std']!r} host {s!r}; "
          f"counts {np.bincount(det['expert'].cpu().numpy(), minlength=E).tolist()}")
    assert abs(det["ws_mean"] - m) <= rel * m and abs(det["ws_std"] - s) <= 1e-12 * m
    for e in range(E):
        assert abs(det[f"ws_mean_{e}"] - me[e]) <= rel * me[e]
        assert abs(det[f"ws_std_{e}"] - se[e]) <= 1e-12 * m
    again = moe.evaluate_device(7, cond, x, cfg, seed=seed, details=True)
    assert all(again[k] == det[k] for k in _metric_keys(E))
    assert all(torch.equal(again[k], det[k]) for k in ("sums_real", "sums_gen", "expert", "ws"))
    moved = moe.evaluate_device(7, cond, x, cfg, seed=seed, sample_offset=96, details=True)
    assert not torch.equal(moved["sums_gen"], det["sums_gen"])


def test_evaluate_device_empty_expert():
    E = 3
    moe, cfg = _moe("fp32", E)
    _, x, cond = _batch(96)
    with torch.no_grad():
        moe.router._modules["fc_layers"]._modules["6"].bias[1] = -1e4
    moe.router.invalidate()
    out = moe.evaluate_device(7, cond, x, cfg, seed=4, routing="argmax", details=True)
    counts = np.bincount(out["expert"].cpu().numpy(), minlength=E)
    print(f"argmax routing with expert 1 biased away: counts {counts.tolist()}")
    assert counts[1] == 0
    assert out["ws_mean_1"] == 0.0 and out["ws_std_1"] == 0.0
    for k in ("ws_mean", "ws_std", "ws_mean_0", "ws_std_0", "ws_mean_2", "ws_std_2"):
        assert np.isfinite(out[k]) and out[k] > 0, k


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_evaluate_epoch_on_device(precision):
    from torch.utils.data import DataLoader, TensorDataset

    from expertsim.train.loop import evaluate_epoch
    moe, cfg = _moe(precision, 3, extra=("train.eval_on_device=true",))
    b, x, _ = _batch(96)
    ds = TensorDataset(x, x, torch.from_numpy(b["cond"]), torch.from_numpy(b["std"]),
                       torch.from_numpy(b["intensity"]), torch.from_numpy(b["true_positions"]))
    cap0, rep0 = moe.sim_captures, moe.sim_replays
    out = evaluate_epoch(moe, DataLoader(ds, batch_size=48), epoch=7, cfg=cfg, device=torch.device(DEV))
    assert set(out) == _metric_keys(3) - {"epoch"}
    assert all(np.isfinite(v) and v >= 0 for v in out.values())
    assert out["ws_mean"] > 0
    # one chunk program (48 rows) serves both repetitions of both batches: 1 capture, 3 replays
    assert (moe.sim_captures - cap0, moe.sim_replays - rep0) == (1, 3)


def test_evaluate_device_single_expert():
    moe, cfg = _moe("fp32", 1)
    _, x, cond = _batch(96)
    out = moe.evaluate_device(7, cond, x, cfg, seed=2, details=True)
    assert set(out) == _metric_keys(1) | {"sums_real", "sums_gen", "expert", "ws"}
    assert int(out["expert"].abs().sum()) == 0
    assert out["ws_mean_0"] == out["ws_mean"] and out["ws_std_0"] == out["ws_std"] and out["ws_mean"] > 0
