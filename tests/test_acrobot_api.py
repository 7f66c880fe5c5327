"""CPU: Acrobot is declared, bound and exported like the other games, its random policy stays in {0, 1, 2}, and there is no
CPU execution mode behind it."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def test_header_binding_and_library_have_the_create_call(hip_lib):
    from madrona_rl_envs_playground_amd import _lib
    header = open(os.path.join(REPO, "include", "mrl_envs.h")).read()
    assert re.search(r"\bint mrl_acrobot_create\(int gpu_id, uint32_t num_worlds, mrl_sim \*\*out\);", header)
    assert "mrl_acrobot_create" in _lib.SYMBOLS
    assert hasattr(hip_lib, "mrl_acrobot_create")
    assert re.search(r"MRL_GAME_ACROBOT = 6\b", header) and re.search(r"#define MRL_ACROBOT_MAX_STEPS 500\b", header)
    slots = re.findall(r"MRL_ACROBOT_([A-Z_]+) = (\d+)", header)
    assert slots == [("RESET", "0"), ("ACTION", "1"), ("STATE", "2"), ("REWARD", "3"), ("WORLD_ID", "4"), ("RESET_COUNT", "5"),
                     ("SCAN_TIMEOUT", "6"), ("SHARD_COUNT", "7"), ("EPISODE_LENGTH", "8")]
    assert hip_lib.mrl_abi_version() == 4  # additive: the ABI version stays


def test_null_out_pointer_is_refused(hip_lib):
    assert hip_lib.mrl_acrobot_create(0, 4, None) == 1  # MRL_ERR_INVALID


def test_random_policy_is_uniform_over_three_torques():
    from madrona_rl_envs_playground_amd.simulators import random_acrobot_action, random_hash
    world = np.arange(100000)
    seen = np.zeros(3, np.int64)
    for step in (0, 1, 77, 2 ** 31):
        a = random_acrobot_action(12345678901234, step, world)
        assert a.dtype == np.int32 and a.min() >= 0 and a.max() <= 2
        h = random_hash(12345678901234, step, world, np.zeros_like(world)).astype(np.uint64)
        assert np.array_equal(a, ((h * np.uint64(3)) >> np.uint64(32)).astype(np.int32))
        seen += np.bincount(a, minlength=3)
    assert np.abs(seen / seen.sum() - 1 / 3).max() < 0.01


def test_cpu_mode_raises_and_the_reference_name_is_an_alias():
    from madrona_rl_envs_playground_amd import envs, simulators
    assert simulators.AcrobatSimulator is simulators.AcrobotSimulator
    with pytest.raises(NotImplementedError):
        simulators.AcrobotSimulator(exec_mode=simulators.ExecMode.CPU, gpu_id=0, num_worlds=4)
    assert envs.AcrobotMadronaTorch and envs.AcrobotMadronaNumpy
    with pytest.raises(ValueError, match="observation"):
        envs.AcrobotMadronaTorch(4, 0, observation="pixels")
