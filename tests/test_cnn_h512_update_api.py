"""CPU: the surface of the hidden-512 MAPPO update (``mrl_mappo_h512_update``, ``MappoOptimizerH512``, ``mappo_update_h512``) that
needs no GPU -- symbols, the workspace formula, the Python refusals, the old entry points' refusals of 512, and the conditions of
the inputs of every case of tests/test_gpu_cnn_h512_update.py."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

import cnn_h512_update_cases as cases
import mappo_twin as twin
from madrona_rl_envs_playground_amd import _lib, simulators
from madrona_rl_envs_playground_amd.simulators import (CnnGruPolicy, CnnPolicy, CnnRecord, MappoOptimizer, MappoOptimizerH512, mappo_update,
                                                         mappo_update_h512)


def h512_bytes(lib, w, h, f, width, rows, out):
    """the size query of the layered update: the library exports no new symbol, the width travels as 512 | MRL_MAPPO_H512_HIDDEN"""
    return lib.mrl_mappo_workspace_bytes(w, h, f, 512 | _lib.MAPPO_H512_HIDDEN, width, rows, out)


def sized(lib, key, width, rows=1):
    w, h, _, f = cases.shapes.shape(key)
    out = ctypes.c_uint64(0)
    return h512_bytes(lib, w, h, f, width, rows, ctypes.byref(out)), out.value


def test_symbols_and_signatures(hip_lib):
    assert hip_lib.mrl_abi_version() == 4
    assert (_lib.MAPPO_H512, _lib.MAPPO_H512_HIDDEN) == (32, 0x1000) and not hasattr(hip_lib, "mrl_mappo_h512_update")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mrl_envs.h")).read()
    assert "MRL_MAPPO_H512 = 32 }" in header and "MRL_MAPPO_H512_HIDDEN = 0x1000 }" in header
    assert simulators.mappo_update_h512 is mappo_update_h512 and simulators.MappoOptimizerH512 is MappoOptimizerH512
    assert inspect.signature(mappo_update_h512) == inspect.signature(mappo_update)
    assert inspect.signature(MappoOptimizerH512.__init__) == inspect.signature(MappoOptimizer.__init__)
    policy = CnnPolicy(5, 4, 26, hidden=512, device="cpu")
    optimizer = MappoOptimizerH512(policy, lr=3e-4, critic_lr=7e-4)
    assert (optimizer.lr, optimizer.critic_lr, optimizer.step, optimizer.betas, optimizer.eps) == (3e-4, 7e-4, 0, (0.9, 0.999), 1e-5)
    assert optimizer.exp_avg.shape == optimizer.exp_avg_sq.shape == policy.params.shape
    assert optimizer.workspace_bytes(65, 3) == sized(hip_lib, "cramped_room", 65, 3)[1]


@pytest.mark.parametrize("key", sorted({case[0] for case in cases.PARITY}))
def test_workspace_formula_stops_growing_at_one_slab(hip_lib, key):
    for width, rows in ((1, 1), (33, 1), (65, 6), (cases.SLAB - 64, 1), (cases.SLAB, 2)):
        assert sized(hip_lib, key, width, rows) == (0, cases.workspace_bytes(key, width, rows)), (width, rows)
    assert sized(hip_lib, key, cases.SLAB - 64)[1] < sized(hip_lib, key, cases.SLAB)[1]
    assert sized(hip_lib, key, cases.SLAB)[1] == sized(hip_lib, key, cases.SLAB + 33)[1] == sized(hip_lib, key, (1 << 32) - 1)[1]


def test_sizer_refusals(hip_lib):
    out = ctypes.c_uint64(0)
    assert h512_bytes(hip_lib, 5, 4, 26, 0, 1, ctypes.byref(out)) == 1
    assert h512_bytes(hip_lib, 2, 4, 26, 33, 1, ctypes.byref(out)) == 1
    assert h512_bytes(hip_lib, 5, 4, 26, 33, 1, None) == 1
    assert h512_bytes(hip_lib, 12, 5, 26, 33, 1, ctypes.byref(out)) == 1
    message = hip_lib.mrl_last_error().decode()
    assert "LDS image of 203872 bytes" in message and "163840" in message


def test_python_refusals_and_the_old_refusals_still_standing(hip_lib):
    wide, plain = CnnPolicy(5, 4, 26, hidden=512, device="cpu"), CnnPolicy(5, 4, 26, device="cpu")
    with pytest.raises(ValueError, match="hidden = 512"):
        MappoOptimizerH512(plain)
    with pytest.raises(ValueError, match="hidden = 512"):
        MappoOptimizerH512(CnnGruPolicy(5, 4, 26, device="cpu"))
    with pytest.raises(ValueError, match="device update.*64 only"):
        MappoOptimizer(wide)
    record = CnnRecord(2, 3, 2, "cpu")
    ring = torch.zeros((3, 3, 2, 4, 5, 26), dtype=torch.int8)
    values = torch.zeros((2, 3, 2))
    indices = torch.zeros((1, 4), dtype=torch.int32)
    optimizer = MappoOptimizerH512(wide)
    for policy, opt in ((wide, MappoOptimizer(plain)), (plain, MappoOptimizer(plain)), (wide, MappoOptimizerH512(CnnPolicy(5, 4, 26, hidden=512, device="cpu"))),
                        (CnnGruPolicy(5, 4, 26, device="cpu"), optimizer)):
        with pytest.raises(ValueError, match="mappo_update_h512"):
            mappo_update_h512(policy, opt, record, ring, values, values, indices)
    with pytest.raises(ValueError, match="the MappoOptimizer made for it"):
        mappo_update(wide, optimizer, record, ring, values, values, indices)
    with pytest.raises(ValueError, match="CnnRecord"):
        mappo_update_h512(wide, optimizer, object(), ring, values, values, indices)
    assert optimizer.step == 0
    # the old C entry points refuse the width as before
    out = ctypes.c_uint64(7)
    assert hip_lib.mrl_mappo_workspace_bytes(5, 4, 26, 512, 33, 1, ctypes.byref(out)) == 1 and out.value == 7
    assert b"hidden must be 64" in hip_lib.mrl_last_error()
    assert hip_lib.mrl_mappo_bank_workspace_bytes(5, 4, 26, 512, 33, 1, 2, ctypes.byref(out)) == 1 and out.value == 7


@pytest.mark.parametrize("case", cases.PARITY + cases.CROSSING, ids=lambda c: "-".join(str(x) for x in c))
def test_input_conditions_of_every_gpu_case(case):
    """conditions, not measurements, on the very batches the GPU file uses: no sample within KINK of a kink of the loss, a quarter
    of the samples ratio-clipped and a quarter value-clipped.  (The hidden-64 cases also keep every pre-activation away from 0; with
    33 x (256 npos + 1024) of them per net no batch does that here, and d, float32 on the CPU against the twin, carries the same
    near-zero units.)"""
    fixed = cases.fixed(*case)
    exact, width = fixed["twin"], case[1]
    assert exact["kink"] > twin.KINK, exact["kink"]
    assert (fixed["indices"] >= 0).all() and (fixed["indices"] < len(fixed["batch"].ring)).all()
    if width > len(fixed["batch"].ring):
        assert len(np.unique(fixed["indices"])) <= twin.DISTINCT
    if width >= 24:
        b = exact["branches"]
        assert b["ratio_clipped"] >= 0.25 and b["value_clipped"] >= 0.25, b
    assert fixed["params"].size == sum(p.numel() for p in cases.shapes.make_module(case[0]).parameters())


@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_integer_construction_is_exact_at_512(key):
    case = cases.integer_case(key)
    assert case["bound"] < 2 ** 24 and case["indices"].shape[1] == 64
    assert len(np.unique(case["grad"])) > 8
    with cases.width_512():
        exact = twin.row(case["params"], key, case["batch"], case["indices"][0], case["cfg"])
    assert np.array_equal(exact["grad"][cases.actor_size(key):], case["grad"].astype(np.float64))
    w, h, _, f = cases.shapes.shape(key)
    assert (key == "simple/1p") == ((9 * f) % 2 == 1)
