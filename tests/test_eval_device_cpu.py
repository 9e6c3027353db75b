"""Host side of the device evaluation (no GPU): ws_summary's arithmetic, the bindings of the Wasserstein
entry points, the config switch, and the loud failure of evaluate_device off the HIP device."""
import ctypes as C

import numpy as np
import pytest
import torch


def test_ws_summary_is_the_reference_closing_arithmetic():
    from expertsim.train.utils import ws_summary
    rng = np.random.default_rng(0)
    a = rng.gamma(2.0, 30.0, (3, 4, 5))                 # [n_calc, 1 + E, channels]
    ws, ws_exp = a[:, 0].copy(), a[:, 1:].copy()        # the reference's two arrays (train/utils.py:117-176)
    ws_runs, ws_exp_runs = ws.mean(axis=1), ws_exp.mean(axis=2)
    m, s, me, se = ws_summary(a)
    assert m == ws_runs.mean() and s == ws_runs.std()
    np.testing.assert_array_equal(me, ws_exp_runs.mean(axis=0))
    np.testing.assert_array_equal(se, ws_exp_runs.std(axis=0))
    assert me.shape == (3,) and se.shape == (3,)
    with pytest.raises(ValueError):
        ws_summary(np.zeros((3, 5)))


def test_wasserstein_bindings_and_path_boundary():
    from expertsim import hip
    lib = hip.lib()
    assert hip._SIGS["es_wasserstein_1d_workspace"][0] is C.c_size_t
    assert len(hip._SIGS["es_wasserstein_1d"][1]) == 18
    assert lib.es_wasserstein_lds_max() == hip.WS_LDS_MAX
    L = hip.WS_LDS_MAX
    assert lib.es_wasserstein_1d_workspace(6, 5, L // 2, L - L // 2) == 0          # sorted in LDS
    need = lib.es_wasserstein_1d_workspace(6, 5, L // 2, L - L // 2 + 1)           # padded to 2 L values
    assert need == 6 * 5 * 2 * L * 9
    assert lib.es_wasserstein_1d_workspace(1, 1, 2 ** 19, 2 ** 19) == 2 ** 20 * 9


def test_wasserstein_1d_device_needs_the_device():
    from expertsim import hip
    from expertsim.train.utils import wasserstein_1d_device, ws_across_experts_device
    u = torch.zeros(4, 5, dtype=torch.float64)
    with pytest.raises(hip.HipError):
        wasserstein_1d_device(u, u)
    with pytest.raises(hip.HipError):
        ws_across_experts_device(u, u[None], torch.zeros(4, dtype=torch.int32), 1)


def test_eval_on_device_defaults_off():
    from expertsim.config import load_config
    assert load_config().train.get("eval_on_device", None) is False
    assert load_config(overrides=["train.eval_on_device=true"]).train.eval_on_device is True


def test_evaluate_device_raises_off_the_hip_device():
    from expertsim import hip
    from expertsim.config import inject_shared, load_config
    from expertsim.models import build_model
    from expertsim.models.moe import MoEWrapper
    cfg = inject_shared(load_config(overrides=["model.architecture=neutron", "model.n_experts=1"]))
    torch.manual_seed(0)
    parts = [build_model(f"neutron.{k}", getattr(cfg.model, k), "cpu") for k in ("generator", "discriminator", "aux_reg")]
    router = build_model("router_v1", cfg.model.router, "cpu")
    moe = MoEWrapper(*parts, router, 1, cfg, image_shape=(44, 44))
    with pytest.raises(hip.HipError):
        moe.evaluate_device(7, torch.zeros(4, 9), torch.zeros(4, 44, 44), cfg)
