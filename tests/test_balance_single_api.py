"""No GPU: the surface of single-agent PPO on the balance beam -- ``BalanceGym`` and its spaces, ``MlpPolicy(7, 4,
observation="beam")``, the update's workspace size and shape refusals for (7, 4) -- and the two conditions the GPU tests of
tests/test_gpu_balance_single.py rest on: draws near a boundary of the twin's CDF are rare for their seed, and no sample of
an update case lies within 1e-5 of a kink of the loss."""
import ctypes
import inspect

import numpy as np
import pytest

import balance_single_cases as cases
import policy_twin
import ppo_twin
from madrona_rl_envs_playground_amd import _lib, simulators


def workspace_bytes(lib, width, rows=1, shape=(cases.D, 64, cases.A)):
    out = ctypes.c_uint64(0)
    rc = lib.mrl_ppo_workspace_bytes(shape[0], shape[1], shape[2], width, rows, ctypes.byref(out))
    return rc, out.value


def test_balance_gym_imports_with_the_references_spaces():
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceGym, BalanceMadronaTorch  # the script's first import
    assert BalanceMadronaTorch is not None
    assert list(inspect.signature(BalanceGym.__init__).parameters)[:4] == ["self", "num_envs", "gpu_id", "debug_compile"]
    assert inspect.signature(BalanceGym.__init__).parameters["debug_compile"].default is True
    assert inspect.signature(BalanceGym.__init__).parameters["record_episode_statistics"].default is False
    for space in (BalanceGym.observation_space, BalanceGym.single_observation_space):
        assert np.array_equal(space.nvec, cases.NVEC) and tuple(space.shape) == (7,)
    for space in (BalanceGym.action_space, BalanceGym.single_action_space):
        assert space.n == 4 and tuple(space.shape) == ()
    assert list(inspect.signature(BalanceGym.rollout).parameters) == ["self", "policy", "num_steps", "seed", "first_step", "out", "greedy"]
    for name in ("step", "reset", "close"):
        assert callable(getattr(BalanceGym, name))
    assert "hash" in BalanceGym.rollout.__doc__ and "generator" in BalanceGym.rollout.__doc__  # the stated departure


def test_beam_policy_shape(hip_lib):
    assert _lib.OBS_BALANCE == 2 and "MRL_OBS_BALANCE = 2" in open(_lib.HEADER).read()
    assert hip_lib.mrl_mlp_policy_num_params(7, 64, 4) == 9669
    policy = simulators.MlpPolicy(7, 4, observation="beam", device="cpu")
    assert policy.params.numel() == 9669 and (policy.obs_dim, policy.num_actions, policy.hidden, policy.observation) == (7, 4, 64, "beam")
    agent = cases.agent(1.0)
    assert sum(p.numel() for p in agent.parameters()) == 9669
    loaded = simulators.MlpPolicy.from_module(agent, observation="beam")
    assert np.array_equal(loaded.params.numpy(), cases.params(1.0))
    for shape in ((4, 2), (7, 3), (6, 4)):
        with pytest.raises(ValueError, match="beam"):
            simulators.MlpPolicy(*shape, observation="beam", device="cpu")
    with pytest.raises(ValueError, match="beam"):
        simulators.MlpPolicy(7, 4, hidden=32, observation="beam", device="cpu")
    with pytest.raises(ValueError, match="observation"):
        simulators.MlpPolicy(7, 4, observation="pixels", device="cpu")
    with pytest.raises(ValueError, match="beam"):
        simulators.MlpPolicy.from_module(policy_twin.make_agent(4, 2, 3), observation="beam")


def test_workspace_bytes_for_the_beams_shape(hip_lib):
    rc, one = workspace_bytes(hip_lib, 64)
    assert rc == _lib.MRL_OK and one > 9669 * 4
    size = lambda width: workspace_bytes(hip_lib, width)[1]  # noqa: E731
    tile, saturation = ppo_twin.tile_size(size), ppo_twin.saturation(size)
    # the tile and the cap are the kernel's, not the shape's
    small = lambda width: workspace_bytes(hip_lib, width, 1, (4, 64, 2))[1]  # noqa: E731
    assert (tile, saturation) == (ppo_twin.tile_size(small), ppo_twin.saturation(small))
    sizes = [1, tile, tile + 1, 3 * tile + 5, saturation - tile, saturation - tile + 1, saturation, saturation + 5, 1 << 24, (1 << 32) - 1]
    got = [size(width) for width in sizes]
    assert got == sorted(got)
    assert got[0] == got[1] < got[2] < got[3] < got[4] < got[5], "one more partial vector per tile up to the cap"
    assert got[5] == got[-1], "and none beyond it"
    assert size(saturation + 5) > small(saturation + 5), "9669 parameters against 9155"


def test_shape_refusals_list_four_shapes(hip_lib):
    four = "(4, 2), (4, 3), (6, 3), (7, 4)"
    for shape in ((7, 64, 3), (5, 64, 4), (7, 64, 2), (4, 64, 4), (7, 32, 4)):
        rc, _ = workspace_bytes(hip_lib, 64, 1, shape)
        message = hip_lib.mrl_last_error().decode()
        assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_workspace_bytes" in message and four in message, (shape, message)
        desc = _lib.MlpPolicyDesc(0, shape[0], shape[1], shape[2], 0, 0)
        opt = _lib.PpoOptimizerDesc(4096, 4096, 4096, 0)
        batch = _lib.PpoBatch(4096, 4096, 4096, 4096, 4096, 4096, 128)
        cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, 3)
        rc = hip_lib.mrl_ppo_update(ctypes.byref(desc), ctypes.byref(opt), ctypes.byref(batch), 4096, 1, 64, ctypes.byref(cfg), 4096,
                                    1 << 40, None, None, 0, None)
        message = hip_lib.mrl_last_error().decode()
        assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_update" in message and four in message, (shape, message)
    # a call with nothing of the beam's shape keeps the words it always had
    assert workspace_bytes(hip_lib, 64, 1, (5, 64, 2))[0] == _lib.MRL_ERR_INVALID
    message = hip_lib.mrl_last_error().decode()
    assert "(6, 3) and minibatch_size" in message and "(7, 4)" not in message


def test_obs_alignment_of_the_beams_rows(hip_lib):
    """(7, 4) rows are 28 bytes: a 4-byte boundary is enough and anything less is refused in new words that name all four shapes;
    with these dummy addresses an accepted call gets as far as the next check that fails."""
    desc = _lib.MlpPolicyDesc(0, 7, 64, 4, 0, 0)
    opt = _lib.PpoOptimizerDesc(4096, 4096, 4096, 0)
    cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, 3)

    def call(obs, workspace_bytes):
        batch = _lib.PpoBatch(obs, 4096, 4096, 4096, 4096, 4096, 128)
        rc = hip_lib.mrl_ppo_update(ctypes.byref(desc), ctypes.byref(opt), ctypes.byref(batch), 4096, 1, 64, ctypes.byref(cfg), 4096,
                                    workspace_bytes, None, None, 0, None)
        return rc, hip_lib.mrl_last_error().decode()

    for off in (1, 2, 3):
        rc, message = call(4096 + off, 1 << 40)
        assert rc == _lib.MRL_ERR_INVALID and "4-byte boundary" in message and "(7, 4)" in message and "(6, 3)" in message, message
    for off in (4, 8, 12):
        rc, message = call(4096 + off, 0)
        assert rc == _lib.MRL_ERR_INVALID and "workspace of 0 bytes" in message, message


@pytest.mark.parametrize("scale", cases.SCALES)
def test_draws_near_a_boundary_are_rare_for_the_seed_of_the_gpu_tests(scale):
    """The GPU parity test may leave out world-steps whose u lies within 1e-5 of a boundary of the twin's CDF, at most 0.5 % of
    them.  With u on the 2^-24 grid and three boundaries that is an expected 3 * 2e-5 * T * N = 0.5 cases at the largest size:
    counted here, with the twin alone, for the draws the GPU tests use, on observations from the space's ranges."""
    n, t = max(cases.SIZES), cases.ROWS
    weights = cases.params(scale)
    u = policy_twin.draws(cases.SEED, 0, t, n).reshape(-1)
    obs = cases.observations(t * n, np.random.default_rng(11))
    assert obs.min() == 0 and np.array_equal(obs.max(axis=0), cases.NVEC - 1)
    result = policy_twin.act(weights, obs, u, cases.A)
    near = (np.abs(u[:, None] - result["cdf"]) < 1e-5).any(axis=1)
    print(f"beam scale {scale}: {int(near.sum())} of {near.size} draws within 1e-5 of a boundary")
    assert near.mean() <= 0.005
    # every action is drawn, and the scaled actor has left uniform
    assert set(result["actions"].tolist()) == {0, 1, 2, 3}
    if scale == 100.0:
        assert np.abs(np.exp(result["logp"]) - 0.25).max() > 0.1


def test_partner_draws_are_uniform_over_the_four_moves():
    """seat 1's moves, ``random_balance_action(seed, step, world, 1)``: the four moves in equal shares (binomial, 8200 draws: a
    share is within 5 sigma = 0.024 of a quarter), and another stream than the ego's u"""
    worlds = np.arange(max(cases.SIZES))
    moves = np.stack([simulators.random_balance_action(cases.SEED, k, worlds, 1) for k in range(cases.ROWS)])
    assert moves.dtype == np.int32 and moves.min() == 0 and moves.max() == 3
    shares = np.bincount(moves.reshape(-1), minlength=4) / moves.size
    assert np.abs(shares - 0.25).max() < 0.024
    ego = np.stack([simulators.random_balance_action(cases.SEED, k, worlds, 0) for k in range(cases.ROWS)])
    assert (moves != ego).mean() > 0.5


@pytest.mark.parametrize("scale", cases.SCALES)
def test_no_sample_of_an_update_case_lies_on_a_kink(scale, hip_lib):
    size = lambda width: workspace_bytes(hip_lib, width)[1]  # noqa: E731
    tile, saturation = ppo_twin.tile_size(size), ppo_twin.saturation(size)
    for name in cases.UPDATE_SIZES:
        width = cases.resolve(name, tile, saturation)
        fixed = cases.fixed_case(scale, width)
        assert fixed["batch"].obs.shape == (ppo_twin.BATCH, 7) and np.array_equal(fixed["batch"].obs, np.round(fixed["batch"].obs))
        assert fixed["twin"]["kink"] > ppo_twin.KINK, (scale, width, fixed["twin"]["kink"])
        if width >= 63:
            for branch, share in fixed["twin"]["branches"].items():
                assert 0.1 <= share <= 0.9, (scale, width, branch, share)
        assert ppo_twin.row_margins(fixed["twin"], fixed["f32"])["grad"] > 0  # the unit of the GPU test's margin
