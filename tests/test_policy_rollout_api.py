"""CPU: the ends of mrl_rollout_policy / mrl_gae that need no GPU -- the symbols, the parameter count and order, the
``MlpPolicy`` round trip, the sampling grid, the refusals that are decided before any device call, and the float64 twins
(tests/policy_twin.py) the GPU tests compare against."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import policy_twin as twin
from madrona_rl_envs_playground_amd import _lib, simulators

GPU_CASES = twin.GPU_CASES


def reference_shaped_agent(obs_dim, num_actions):
    """The trainer's Agent (scripts/cartpole_train_torch.py:105-121) by shape, built here and not by the package."""
    nn = torch.nn

    class Agent(nn.Module):
        def __init__(self):
            super().__init__()
            self.critic = nn.Sequential(nn.Linear(obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 1))
            self.actor = nn.Sequential(nn.Linear(obs_dim, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, num_actions))

    torch.manual_seed(7)
    return Agent()


def test_symbols_are_declared_and_bound(hip_lib):
    for name in ("mrl_mlp_policy_num_params", "mrl_rollout_policy", "mrl_gae"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    header = open(_lib.HEADER).read()
    for word in ("MRL_OBS_RAW = 0", "MRL_OBS_ACROBOT_GYM = 1", "MRL_POLICY_GREEDY = 1", "typedef struct mrl_mlp_policy",
                 "typedef struct mrl_rollout_buffers", "#define MRL_ABI_VERSION 4"):
        assert word in header, word
    assert (_lib.OBS_RAW, _lib.OBS_ACROBOT_GYM, _lib.POLICY_GREEDY, _lib.ABI_VERSION) == (0, 1, 1, 4)
    # the structs as the header lays them out (LP64)
    assert ctypes.sizeof(_lib.MlpPolicyDesc) == 32 and _lib.MlpPolicyDesc.obs_dim.offset == 8 and _lib.MlpPolicyDesc.flags.offset == 24
    assert ctypes.sizeof(_lib.RolloutBuffers) == 80 and _lib.RolloutBuffers.num_steps.offset == 72
    assert [f[0] for f in _lib.RolloutBuffers._fields_[:9]] == list(simulators.Rollout._fields)


@pytest.mark.parametrize("obs_dim, num_actions", [(4, 2), (4, 3), (6, 3)])
def test_parameter_count_and_order_are_the_reference_agents(obs_dim, num_actions, hip_lib):
    agent = reference_shaped_agent(obs_dim, num_actions)
    assert hip_lib.mrl_mlp_policy_num_params(obs_dim, 64, num_actions) == sum(p.numel() for p in agent.parameters())
    policy = simulators.MlpPolicy.from_module(agent)
    assert policy.params.dtype == torch.float32 and policy.params.device.type == "cpu"
    assert torch.equal(policy.params, torch.nn.utils.parameters_to_vector(agent.parameters()).detach())
    assert (policy.obs_dim, policy.num_actions, policy.hidden, policy.observation) == (obs_dim, num_actions, 64, "state")
    # the twin's view of the same vector
    nets = twin.split(policy.params.numpy(), obs_dim, num_actions)
    assert np.array_equal(nets["critic"][0][0], agent.critic[0].weight.detach().double().numpy())
    assert np.array_equal(nets["actor"][2][1], agent.actor[4].bias.detach().double().numpy())


def test_from_module_and_module_round_trip_bit_for_bit():
    agent = reference_shaped_agent(4, 2)
    policy = simulators.MlpPolicy.from_module(agent)
    again = policy.module()
    assert isinstance(again, simulators.MlpAgent)
    assert list(again.state_dict()) == list(agent.state_dict())
    for name, value in agent.state_dict().items():
        assert again.state_dict()[name].numpy().tobytes() == value.numpy().tobytes(), name
    # load_ copies in place: the tensor the kernel reads does not move
    before = policy.params.data_ptr()
    with torch.no_grad():
        agent.actor[4].bias.add_(1.0)
    assert policy.load_(agent) is policy and policy.params.data_ptr() == before
    assert torch.equal(policy.params[-2:], agent.actor[4].bias.detach())
    # the update phase's interface
    x = torch.zeros(3, 4)
    action, logprob, entropy, value = again.get_action_and_value(x)
    assert action.shape == (3,) and logprob.shape == (3,) and entropy.shape == (3,) and value.shape == (3, 1)
    assert torch.equal(again.get_value(x), again.critic(x))


def test_from_module_refuses_other_shapes():
    nn = torch.nn
    agent = reference_shaped_agent(4, 2)
    agent.actor = nn.Sequential(nn.Linear(4, 64), nn.ReLU(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 2))
    with pytest.raises(ValueError, match="actor"):
        simulators.MlpPolicy.from_module(agent)
    agent = reference_shaped_agent(4, 2)
    agent.critic[4] = nn.Linear(64, 2)
    with pytest.raises(ValueError, match="layers"):
        simulators.MlpPolicy.from_module(agent)
    with pytest.raises(ValueError, match="num_actions"):
        simulators.MlpPolicy(4, 3, device="cpu").load_(reference_shaped_agent(4, 2))
    with pytest.raises(ValueError, match="observation"):
        simulators.MlpPolicy(4, 2, observation="pixels", device="cpu")


def test_sample_u_lies_on_the_float32_grid():
    worlds = np.arange(4096)
    for seed, step in ((0, 0), (GPU_CASES["cartpole"][0], 31), (2 ** 63 + 5, 2 ** 31)):
        u = simulators.sample_u(seed, step, worlds)
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        scaled = u.astype(np.float64) * 2.0 ** 24
        assert np.array_equal(scaled, np.round(scaled))
        assert np.array_equal(scaled.astype(np.uint32), simulators.random_hash(seed, step, worlds, np.zeros_like(worlds)) >> np.uint32(8))
    assert 0.45 < simulators.sample_u(1, 0, worlds).mean() < 0.55


def test_calls_that_are_refused_before_any_device_work(hip_lib):
    assert hip_lib.mrl_rollout_policy(None, None, None, 0, 0, None) == _lib.MRL_ERR_INVALID
    assert b"null simulator" in hip_lib.mrl_last_error()
    assert hip_lib.mrl_gae(None, None, None, None, None, 4, 4, 0.99, 0.95, None, None, 0, None) == _lib.MRL_ERR_INVALID
    assert b"mrl_gae" in hip_lib.mrl_last_error()


def test_python_surface():
    for cls_name, module in (("CartpoleMadronaTorch", "cartpole_env"), ("AcrobotMadronaTorch", "acrobot_env")):
        env = getattr(__import__(f"madrona_rl_envs_playground_amd.envs.{module}", fromlist=[cls_name]), cls_name)
        assert list(inspect.signature(env.rollout).parameters) == ["self", "policy", "num_steps", "seed", "first_step", "out", "greedy"]
    assert list(inspect.signature(simulators._Simulator.rollout_policy).parameters) == \
        ["self", "policy", "num_steps", "seed", "first_step", "out", "greedy"]
    assert list(inspect.signature(simulators.gae).parameters) == ["rollout", "gamma", "gae_lambda"]
    assert simulators.Rollout._fields == ("obs", "actions", "logprobs", "values", "rewards", "dones", "next_obs", "next_value", "next_done")


def _observations(kind, count, rng):
    if kind == "cartpole":  # within the termination thresholds, velocities of a few units
        return rng.uniform(-1, 1, (count, 4)) * np.array([2.4, 3.0, 0.21, 3.0])
    state = rng.uniform(-1, 1, (count, 4)) * np.array([np.pi, np.pi, 4 * np.pi, 9 * np.pi])
    return state if kind == "acrobot" else twin.observe_gym(state)


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("kind, obs_dim, num_actions", [("cartpole", 4, 2), ("acrobot", 4, 3), ("acrobot_gym", 6, 3)])
def test_twin_agrees_with_torch_float32(kind, obs_dim, num_actions, scale):
    """The twin against torch's float32 forward of the same module.  Bound, from the formats: a float32 dot product of n
    terms is within n * 2^-24 * sum |term| of the exact one; the three layers have D, 64 and 64 terms, tanh does not
    expand errors, the last layer's rows have norm <= 1 (critic) or 0.01 * scale (actor), so |error| <= (D + 128 + 8) * 2^-24 *
    (the largest |input| + 64) * max(1, 0.01 * scale): a few 1e-4 at worst for Acrobot's velocities.  What is measured is two
    orders below that."""
    rng = np.random.default_rng(5)
    agent = twin.make_agent(obs_dim, num_actions, twin.AGENT_SEED, actor_scale=scale)
    params = simulators.MlpPolicy.from_module(agent).params.numpy()
    obs = _observations(kind, 4096, rng).astype(np.float32)
    u = rng.uniform(0, 1, len(obs))
    result = twin.act(params, obs, u, num_actions)
    d_value, d_logp = twin.margins(agent, params, obs, result["actions"])
    bound = (obs_dim + 136) * 2.0 ** -24 * (np.abs(obs).max() + 64) * max(1.0, 0.01 * scale)
    print(f"{kind} scale {scale}: torch float32 is {d_value:.3g} (values) and {d_logp:.3g} (log-probs) from the twin, bound {bound:.3g}")
    assert 0 < d_value <= bound and 0 < d_logp <= bound
    # the twin's own consistency: probabilities sum to one, the action counts the boundaries reached, greedy is the mode
    p = np.exp(result["logp"])
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-12)
    assert np.array_equal(result["greedy"], p.argmax(axis=1))
    assert np.array_equal(result["actions"], (u[:, None] >= np.cumsum(p, axis=1)[:, :-1]).sum(axis=1))
    if scale == 100.0:
        assert np.abs(p - 1.0 / num_actions).max() > 0.1  # the probabilities have left uniform


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("kind, obs_dim, num_actions", [("cartpole", 4, 2), ("acrobot", 4, 3), ("acrobot_gym", 6, 3)])
def test_draws_near_a_boundary_are_rare_for_the_seeds_of_the_gpu_tests(kind, obs_dim, num_actions, scale):
    """The GPU parity test may leave out world-steps whose u lies within 1e-5 of a boundary of the twin's CDF, at most 0.5 %
    of them.  With u on the 2^-24 grid that is an expected (A - 1) * 2e-5 * T * N < 1.4 cases: counted here, with the twin alone,
    for the draws the GPU tests use, on observations from the environments' ranges."""
    seed, n, t = GPU_CASES[kind.split("_")[0]]
    rng = np.random.default_rng(11)
    agent = twin.make_agent(obs_dim, num_actions, twin.AGENT_SEED, actor_scale=scale)
    params = simulators.MlpPolicy.from_module(agent).params.numpy()
    u = twin.draws(seed, 0, t, n).reshape(-1)
    cdf = twin.act(params, _observations(kind, t * n, rng), u, num_actions)["cdf"]
    near = (np.abs(u[:, None] - cdf) < 1e-5).any(axis=1)
    print(f"{kind} scale {scale}: {int(near.sum())} of {near.size} draws within 1e-5 of a boundary")
    assert near.sum() <= 8 and near.mean() < 0.005


@pytest.mark.parametrize("num_steps", [1, 32])
def test_gae_twin_agrees_with_the_trainers_loop(num_steps):
    """float64 twin against the loop on float32 torch tensors: |values| of a few units summed over up to 32 discounted steps
    stay below ~100, and each of the ~6 float32 operations per step rounds by at most 2^-24 of that: 32 * 6 * 2^-24 * 100 ~
    1e-3 is the bound; and exactly equal in float64."""
    rng = np.random.default_rng(num_steps)
    case = twin.gae_case(num_steps, 257, rng)
    adv, ret = twin.gae(*case, 0.99, 0.95)
    adv32, ret32 = twin.gae_loop_torch(*[torch.from_numpy(a) for a in case], 0.99, 0.95)
    assert adv32.dtype == torch.float32
    d = max(np.abs(adv32.numpy() - adv).max(), np.abs(ret32.numpy() - ret).max())
    print(f"T = {num_steps}: the float32 loop is {d:.3g} from the twin")
    assert 0 < d < 1e-3
    adv64, ret64 = twin.gae_loop_torch(*[torch.from_numpy(a).double() for a in case], 0.99, 0.95)
    assert np.allclose(adv64.numpy(), adv, rtol=0, atol=1e-12) and np.allclose(ret64.numpy(), ret, rtol=0, atol=1e-12)
    # a world done at every step never bootstraps: its advantage is reward - value
    assert np.array_equal(adv[:, 0], case[0][:, 0].astype(np.float64) - case[1][:, 0].astype(np.float64))
