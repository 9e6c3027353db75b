"""Host-side checks of the simulation path (no GPU): the C ABI of the four new entry points and
es_affine_t, their ctypes bindings, the CLI flags and the chunk / random-offset plan of
MoEWrapper.simulate."""
import ctypes as C
import os
import re

import pytest

from conftest import REPO

HEADER = os.path.join(REPO, "include", "expertsim_hip.h")
NEW = ("es_bn_fold", "es_bn_fold_batch", "es_conv2d_fwd_affine", "es_sim_finish")


def _prototype(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)
    assert m, f"{name} is not declared in the header"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_entry_points_and_affine_struct():
    src = open(HEADER).read()
    for name in NEW:
        _prototype(name)
    m = re.search(r"typedef struct \{([^}]*)\}\s*es_affine_t;", src)
    assert m, "es_affine_t missing"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    assert fields == ["const float* scale", "const float* shift", "int act", "float slope"]
    # the reference call sites the issue asks the comments to cite
    assert "neutron/generator.py:13-36" in src and "train/utils.py:179-266" in src


def test_bindings_match_the_header_arity():
    from expertsim import hip
    for name in NEW:
        res, args = hip._SIGS[name]
        assert res is C.c_int
        assert len(args) == len(_prototype(name)), name
    lib = hip.lib()
    for name in NEW:
        assert hasattr(lib, name)
    assert C.sizeof(hip.Affine) == lib.es_struct_size(9) == 24
    assert hip.Affine in hip._ABI_STRUCTS


def test_cli_flags_and_unchanged_defaults():
    import cli
    d = cli.parse_args([])
    assert (d.config, d.override, d.max_steps_per_epoch) == (None, [], None)
    assert d.simulate is False and d.checkpoint is None and d.cond is None and d.num_samples is None
    assert d.out is None and d.seed == 0 and d.sim_batch_size is None
    a = cli.parse_args(["--simulate", "--checkpoint", "ck", "--cond", "c.npy", "--out", "o.npz", "--seed", "7",
                        "--sim-batch-size", "16", "-o", "model.n_experts=3"])
    assert a.simulate and (a.checkpoint, a.cond, a.out, a.seed, a.sim_batch_size) == ("ck", "c.npy", "o.npz", 7, 16)
    assert a.override == ["model.n_experts=3"]
    assert cli.parse_args(["--simulate", "--num-samples", "40"]).num_samples == 40


def test_chunk_and_offset_plan():
    from expertsim.models.moe import simulate_plan
    plan = simulate_plan(200, 64, sample_offset=0, noise_dim=10, n_experts=3)
    assert [p[0] for p in plan] == [0, 64, 128, 192]
    assert [p[1] for p in plan] == [64, 64, 64, 8]
    assert [p[2] for p in plan] == [0, 640, 1280, 1920] and all(p[2] % 2 == 0 for p in plan)
    assert [p[3] for p in plan] == [0, 192, 384, 576]
    # a sample's offsets depend on sample_offset + index only: the second chunk of one plan is the
    # first chunk of the plan that starts there
    assert simulate_plan(64, 64, sample_offset=64, noise_dim=10, n_experts=3)[0][2:] == plan[1][2:]
    assert simulate_plan(200, 200)[0][:3] == (0, 200, 0)
    assert simulate_plan(0, 64) == []
    # es_randn_dev draws pairs: a chunk may not start at an odd element
    with pytest.raises(ValueError):
        simulate_plan(10, 3, noise_dim=5)
    assert [p[2] for p in simulate_plan(10, 3, noise_dim=4)] == [0, 12, 24, 36]
