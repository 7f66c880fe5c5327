"""CPU: the surface of the hidden-512 MLPBase update (``mrl_mappo_mlp_update`` with ``MRL_MLPBASE_H512``, ``MappoOptimizerH512`` and
``mappo_update_h512`` on an ``MlpBasePolicyH512``) that needs no GPU -- the workspace formula, the Python refusals, and the
conditions of the inputs of every case of tests/test_gpu_mlpbase_h512_update.py."""
import ctypes

import pytest
import torch

import mlpbase_h512_update_cases as cases
import mlpbase_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import (CnnRecord, MappoOptimizer, MappoOptimizerH512, MlpBasePolicy, MlpBasePolicyH512,
                                                         MlpBaseRecord, mappo_update_h512)


def sized(lib, layer_N, width, rows=1, hidden=512 | _lib.MLPBASE_H512_HIDDEN):
    out = ctypes.c_uint64(7)
    return lib.mrl_mappo_mlp_workspace_bytes(7, hidden, layer_N, 4, width, rows, ctypes.byref(out)), out.value


@pytest.mark.parametrize("layer_N", (1, 2))
def test_workspace_formula_stops_growing_at_one_slab(hip_lib, layer_N):
    for width, rows in ((1, 1), (33, 1), (65, 6), (cases.SLAB - 64, 1), (cases.SLAB, 2)):
        assert sized(hip_lib, layer_N, width, rows) == (0, cases.workspace_bytes(layer_N, width, rows)), (width, rows)
    assert sized(hip_lib, layer_N, cases.SLAB - 64)[1] < sized(hip_lib, layer_N, cases.SLAB)[1]
    assert sized(hip_lib, layer_N, cases.SLAB)[1] == sized(hip_lib, layer_N, cases.SLAB + 33)[1] == sized(hip_lib, layer_N, (1 << 32) - 1)[1]
    assert sized(hip_lib, layer_N, 33, hidden=512) == (1, 7) and sized(hip_lib, layer_N, 0) == (1, 7)
    assert sized(hip_lib, 3, 33) == (1, 7) and sized(hip_lib, layer_N, 33, hidden=64 | _lib.MLPBASE_H512_HIDDEN) == (1, 7)
    out = ctypes.c_uint64(7)
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 512 | _lib.MLPBASE_H512_HIDDEN, layer_N, 4, 33, 1, 2, ctypes.byref(out)) == 1


def test_python_surface_and_refusals(hip_lib):
    wide, other, plain = MlpBasePolicyH512(2, "cpu"), MlpBasePolicyH512(2, "cpu"), MlpBasePolicy(device="cpu")
    optimizer = MappoOptimizerH512(wide, lr=3e-4, critic_lr=7e-4)
    assert (optimizer.lr, optimizer.critic_lr, optimizer.step) == (3e-4, 7e-4, 0)
    assert optimizer.exp_avg.shape == optimizer.exp_avg_sq.shape == wide.params.shape == (sum(cases.h512.SIZES[2]),)
    assert optimizer.workspace_bytes(65, 3) == sized(hip_lib, 2, 65, 3)[1]
    with pytest.raises(ValueError, match="MlpBasePolicyH512"):
        MappoOptimizerH512(plain)
    record, values, indices = MlpBaseRecord(2, 3, 2, "cpu"), torch.zeros((2, 3, 2)), torch.zeros((1, 4), dtype=torch.int32)
    for policy, opt, rec, ring, match in ((wide, MappoOptimizerH512(other), record, None, "mappo_update_h512"),
                                          (plain, MappoOptimizer(plain), record, None, "mappo_update_h512"),
                                          (wide, optimizer, record, torch.zeros(1), "ring must be None"),
                                          (wide, optimizer, CnnRecord(2, 3, 2, "cpu"), None, "MlpBaseRecord")):
        with pytest.raises(ValueError, match=match):
            mappo_update_h512(policy, opt, rec, ring, values, values, indices)
    assert optimizer.step == 0


@pytest.mark.parametrize("case", cases.PARITY + cases.CROSSING, ids=lambda c: "-".join(str(x) for x in c))
def test_input_conditions_of_every_gpu_case(case):
    """conditions, not measurements, on the very batches the GPU file uses: no sample within KINK of a kink of the loss, a quarter
    of the samples ratio-clipped and a quarter value-clipped, and every row names the constant observation row"""
    fixed = cases.fixed(*case, rows=2 if case in cases.CROSSING else 1)
    exact, width = fixed["twin"], case[1]
    assert exact["kink"] > twin.KINK, exact["kink"]
    assert (fixed["indices"] >= 0).all() and (fixed["indices"] < len(fixed["batch"].obs)).all()
    assert (fixed["indices"] == cases.beam.CONSTANT_ROW).any(axis=1).all() and len(set(fixed["batch"].obs[cases.beam.CONSTANT_ROW])) == 1
    if width >= 24:
        b = exact["branches"]
        assert b["ratio_clipped"] >= 0.25 and b["value_clipped"] >= 0.25, b
    if case[2] == "dead":  # nothing passes fc1's ReLU: feature_norm's, fc1's weight and bias gradients are exactly zero in the reference too
        assert all(not exact["grad"][at:at + cases.DEAD].any() and exact["grad"][at + cases.DEAD:].any() for at in (0, cases.actor_size(case[0])))
    assert fixed["params"].size == sum(cases.h512.SIZES[case[0]])
