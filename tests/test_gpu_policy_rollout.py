"""GPU: ``rollout_policy`` (mrl_policy_act in front of the ordinary step) and ``gae`` (mrl_gae) for Cartpole and Acrobot.

Sizes: one lane, the tails of a wavefront (63), of a 256-thread workgroup (257) and of the step kernels' 4-worlds-per-lane
grid (1025).  Cartpole runs T = 32 rows, inside which episodes end; Acrobot first takes 495 random steps, so that the
500-step truncation and the re-seeding fall inside its T = 16.  Agents are initialised as the reference's trainer does
(tests/policy_twin.py); the second set has the actor's last layer times 100.

Margins: the policy's numbers are compared with the float64 twin fed the GPU's OWN observations, within 8 x d, d being the
largest distance between torch's float32 CPU forward and the twin over the same inputs, per kind of number (the factor
covers another summation order over 64 terms and the device's tanh / exp / log against the host's).  Actions must be the
twin's except where u lies within 1e-5 of a boundary of the twin's CDF (at most 0.5 % of the world-steps;
tests/test_policy_rollout_api.py counts them for these seeds).  Everything the environment produces -- observations, rewards,
done flags, final state, episode numbering, statistics -- is bit for bit what a second simulator stepped with the recorded
actions produces (its ACTION tensor excepted, which mrl_step_with_actions does not write: the rollout's must hold the last row).  Each test prints the ratio it measured."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import policy_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AcrobotSimulator, BalanceBeamSimulator, CartpoleSimulator, ExecMode,  # noqa: E402
                                                         MlpPolicy, Rollout, gae)

SIZES = [1, 63, 257, 1025]
SCALES = [1.0, 100.0]
GAMES = ["cartpole", "acrobot"]
ACTIONS = {"cartpole": 2, "acrobot": 3}
ROWS = {game: twin.GPU_CASES[game][2] for game in GAMES}
SEED = {game: twin.GPU_CASES[game][0] for game in GAMES}
ACROBOT_MAX_STEPS = 500
STATS = ("episode_return_tensor", "episode_steps_tensor", "last_episode_return_tensor", "last_episode_steps_tensor",
         "episode_totals_tensor")


def prepare(game, n):
    if game == "cartpole":
        return CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    sim = AcrobotSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    sim.rollout_random(495, seed=5)
    return sim


def cpu(t):
    return (t.to_torch() if hasattr(t, "to_torch") else t).cpu().numpy().copy()


def snapshot(sim):
    names = ["observation_tensor", "reset_tensor", "action_tensor", "reward_tensor", "reset_count_tensor", "scan_timeout_tensor"]
    if isinstance(sim, AcrobotSimulator):
        names.append("episode_length_tensor")
    return {name: cpu(getattr(sim, name)()) for name in names}


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def same_simulator(got, want, what):
    """two snapshots, one of a simulator that was stepped with caller-owned actions: mrl_step_with_actions leaves the ACTION
    tensor alone, a rollout leaves its last row there (checked where the rows are at hand)"""
    for name in want:
        if name != "action_tensor":
            same_bits(got[name], want[name], f"{what}: {name}")


def next_episode_state(sim):
    """Where the episode counter stands, read through a forced restart of world 0 (it changes that world: the last use)."""
    mask = np.zeros(sim.num_worlds, np.uint8)
    mask[0] = 1
    sim.reset_worlds(mask)
    return cpu(sim.observation_tensor())[0]


def make_policy(game, scale, observation="state"):
    agent = twin.make_agent(6 if observation == "gym" else 4, ACTIONS[game], twin.AGENT_SEED, actor_scale=scale)
    return agent, MlpPolicy.from_module(agent, observation=observation, device="cuda:0")


def to_numpy(rollout):
    return Rollout(*[cpu(t) for t in rollout])


def replay(game, n, actions, stats=False):
    """A second simulator stepped with the recorded actions: what it shows after every step, and where it ends."""
    sim = prepare(game, n)
    if stats:
        sim.enable_episode_stats()
    device_actions = torch.from_numpy(actions).cuda()
    state, reward, reset, length = [], [], [], []
    for k in range(actions.shape[0]):
        if game == "acrobot":
            length.append(sim.episode_length_tensor().to_torch().clone())
        sim.step_with_actions(device_actions[k])
        state.append(sim.observation_tensor().to_torch().clone())
        reward.append(sim.reward_tensor().to_torch().clone())
        reset.append(sim.reset_tensor().to_torch().clone())
    out = {"state": cpu(torch.stack(state)), "reward": cpu(torch.stack(reward))[:, :, 0], "reset": cpu(torch.stack(reset))[:, :, 0],
           "length_before": cpu(torch.stack(length))[:, :, 0] if length else None, "final": snapshot(sim),
           "stats": {name: cpu(getattr(sim, name)()) for name in STATS} if stats else None}
    out["next_episode"] = next_episode_state(sim)
    sim.close()
    return out


@functools.lru_cache(maxsize=None)
def collected(game, n, scale):
    """One rollout per (game, size, weights), shared by the tests below and left unchanged by them."""
    sim = prepare(game, n)
    agent, policy = make_policy(game, scale)
    start = snapshot(sim)
    rollout = to_numpy(sim.rollout_policy(policy, ROWS[game], seed=SEED[game]))
    final = snapshot(sim)
    next_episode = next_episode_state(sim)
    sim.close()
    return {"agent": agent, "params": policy.params.cpu().numpy(), "start": start, "rollout": rollout, "final": final,
            "next_episode": next_episode}


def check_policy_parity(what, agent, params, rollout, seed, first_step=0):
    """teacher-forced: the twin on the GPU's own observation rows"""
    num_actions = int(agent.actor[4].out_features)
    steps, n, d = rollout.obs.shape
    obs = rollout.obs.reshape(-1, d)
    got_actions = rollout.actions.reshape(-1)
    assert got_actions.min() >= 0 and got_actions.max() < num_actions
    u = twin.draws(seed, first_step, steps, n).reshape(-1)
    want = twin.act(params, obs, u, num_actions)
    closing = twin.act(params, rollout.next_obs, np.zeros(n), num_actions)
    every_obs = np.concatenate([obs, rollout.next_obs])
    d_value = twin.margins(agent, params, every_obs, np.zeros(len(every_obs), np.int32))[0]
    d_logp = twin.margins(agent, params, obs, got_actions)[1]
    rows = np.arange(len(obs))
    err_value = max(np.abs(rollout.values.reshape(-1) - want["values"]).max(), np.abs(rollout.next_value - closing["values"]).max())
    err_logp = np.abs(rollout.logprobs.reshape(-1) - want["logp"][rows, got_actions]).max()
    near = (np.abs(u[:, None] - want["cdf"]) < 1e-5).any(axis=1)
    wrong = (got_actions != want["actions"]) & ~near
    print(f"{what}: values {err_value:.3g} from the twin = {err_value / d_value:.2f} d (d = {d_value:.3g}); log-probs {err_logp:.3g} = "
          f"{err_logp / d_logp:.2f} d (d = {d_logp:.3g}); {int(near.sum())} of {near.size} draws left out, {int(wrong.sum())} actions differ")
    assert d_value > 0 and d_logp > 0
    assert err_value <= 8 * d_value, f"values are {err_value / d_value:.2f} d from the twin"
    assert err_logp <= 8 * d_logp, f"log-probs are {err_logp / d_logp:.2f} d from the twin"
    assert near.mean() <= 0.005
    assert not wrong.any()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_teacher_forced_policy_parity(game, n, scale, hip_lib):
    c = collected(game, n, scale)
    check_policy_parity(f"{game} n={n} scale={scale}", c["agent"], c["params"], c["rollout"], SEED[game])
    if scale == 100.0 and n >= 257:  # the second set does leave uniform
        assert np.abs(np.exp(c["rollout"].logprobs) - 1.0 / ACTIONS[game]).max() > 0.05


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_environment_parity(game, n, scale, hip_lib):
    c = collected(game, n, scale)
    r, steps = c["rollout"], ROWS[game]
    other = replay(game, n, r.actions)
    # row 0 is the tensors as they stood at the call
    same_bits(r.obs[0], c["start"]["observation_tensor"], "obs[0]")
    same_bits(r.dones[0], (c["start"]["reset_tensor"][:, 0] != 0).astype(np.float32), "dones[0]")
    for k in range(steps):
        after_obs = r.obs[k + 1] if k + 1 < steps else r.next_obs
        after_done = r.dones[k + 1] if k + 1 < steps else r.next_done
        same_bits(after_obs, other["state"][k], f"observation after step {k}")
        same_bits(r.rewards[k], other["reward"][k], f"rewards[{k}]")
        same_bits(after_done, (other["reset"][k] != 0).astype(np.float32), f"done flag after step {k}")
    same_simulator(c["final"], other["final"], "after the rollout")
    same_bits(c["final"]["action_tensor"][:, 0], r.actions[-1], "the ACTION tensor after the rollout")
    same_bits(c["next_episode"], other["next_episode"], "the episode counter")
    assert int(c["final"]["scan_timeout_tensor"][0]) == 0
    finished = np.concatenate([r.dones[1:], r.next_done[None]]) != 0
    if game == "cartpole":
        assert finished.any(), "no Cartpole world finished inside the window"
    else:
        truncated = finished & (other["length_before"] == ACROBOT_MAX_STEPS)
        assert truncated.any(), "no Acrobot world was truncated inside the window"
        print(f"acrobot n={n}: {int(truncated.sum())} truncated, {int(finished.sum())} finished")


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", SIZES)
def test_gym_observation(n, scale, hip_lib):
    """observation="gym": the six values against float64 from STATE within 8 x d of their own kind (d: torch's float32 CPU
    cos / sin of the same states against float64), and the policy's parity on those rows"""
    agent, policy = make_policy("acrobot", scale, observation="gym")
    sim = prepare("acrobot", n)
    start = snapshot(sim)
    r = to_numpy(sim.rollout_policy(policy, ROWS["acrobot"], seed=SEED["acrobot"]))
    final = snapshot(sim)
    sim.close()
    other = replay("acrobot", n, r.actions)
    states = np.concatenate([start["observation_tensor"][None], other["state"]])  # before step 0 ... after the last
    got = np.concatenate([r.obs, r.next_obs[None]]).reshape(-1, 6)
    want = twin.observe_gym(states.reshape(-1, 4))
    s32 = torch.from_numpy(states.reshape(-1, 4))
    host32 = torch.stack([torch.cos(s32[:, 0]), torch.sin(s32[:, 0]), torch.cos(s32[:, 1]), torch.sin(s32[:, 1])], dim=1).double().numpy()
    d = np.abs(host32 - want[:, :4]).max()
    err = np.abs(got[:, :4] - want[:, :4]).max()
    print(f"gym n={n} scale={scale}: cos / sin {err:.3g} from float64 = {err / d:.2f} d (d = {d:.3g})")
    assert d > 0 and err <= 8 * d
    same_bits(got[:, 4:], states.reshape(-1, 4)[:, 2:], "the velocities")
    same_simulator(final, other["final"], "after the rollout")
    same_bits(final["action_tensor"][:, 0], r.actions[-1], "the ACTION tensor after the rollout")
    check_policy_parity(f"gym n={n} scale={scale}", agent, policy.params.cpu().numpy(), r, SEED["acrobot"])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_greedy_takes_the_first_arg_max(game, n, hip_lib):
    agent, policy = make_policy(game, 100.0)
    sim = prepare(game, n)
    r = to_numpy(sim.rollout_policy(policy, ROWS[game], seed=SEED[game], greedy=True))
    values, logits = twin.forward(policy.params.cpu().numpy(), r.obs.reshape(-1, 4), ACTIONS[game])
    ordered = np.sort(logits, axis=1)
    clear = ordered[:, -1] - ordered[:, -2] > 1e-5  # (a float32 logit is not told from its neighbour below that)
    assert clear.mean() >= 0.995
    got = r.actions.reshape(-1)
    assert np.array_equal(got[clear], logits.argmax(axis=1)[clear])
    logp = logits - logits.max(axis=1, keepdims=True)
    logp -= np.log(np.exp(logp).sum(axis=1, keepdims=True))
    assert np.abs(r.logprobs.reshape(-1) - logp[np.arange(len(got)), got]).max() < 1e-5
    # all logits equal: the FIRST arg-max, and log(1 / A) written all the same
    with torch.no_grad():
        agent.actor[4].weight.zero_()
    policy.load_(agent)
    r = to_numpy(sim.rollout_policy(policy, 4, seed=1, greedy=True))
    assert not r.actions.any()
    # (0 - 0) - log(A) with sum e = A exactly: the device's logf and the host's are each within an ulp (2^-23 at log 3) of log(A)
    assert np.abs(r.logprobs.astype(np.float64) + np.log(ACTIONS[game])).max() <= 2.0 ** -23
    sim.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_same_seed_same_bits_and_first_step_continues_a_stream(game, n, hip_lib):
    c = collected(game, n, 100.0)
    steps, half = ROWS[game], ROWS[game] // 2
    _, policy = make_policy(game, 100.0)
    sim = prepare(game, n)
    first = sim.rollout_policy(policy, half, seed=SEED[game])
    a = to_numpy(first)
    again = sim.rollout_policy(policy, half, seed=SEED[game], first_step=half, out=first)
    assert all(x is y for x, y in zip(again, first))  # `out` is filled, not replaced
    b = to_numpy(again)
    final = snapshot(sim)
    sim.close()
    whole = c["rollout"]
    for name in ("obs", "actions", "logprobs", "values", "rewards", "dones"):
        same_bits(np.concatenate([getattr(a, name), getattr(b, name)]), getattr(whole, name), name)
    for name in ("next_obs", "next_value", "next_done"):
        same_bits(getattr(b, name), getattr(whole, name), name)
    same_bits(a.next_obs, whole.obs[half], "next_obs of the first half")
    same_bits(a.next_done, whole.dones[half], "next_done of the first half")
    same_bits(a.next_value, whole.values[half], "next_value of the first half")
    for name in final:
        same_bits(final[name], c["final"][name], f"final {name}")
    # another seed is another stream
    if n >= 63:
        other = prepare(game, n)
        r = to_numpy(other.rollout_policy(policy, steps, seed=SEED[game] + 1))
        other.close()
        assert not np.array_equal(r.actions, whole.actions)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("game", GAMES)
def test_episode_statistics_and_graph_capture_mode(game, n, hip_lib):
    c = collected(game, n, 1.0)
    _, policy = make_policy(game, 1.0)
    # with the statistics enabled: the five tensors of a simulator that replays the actions
    sim = prepare(game, n)
    sim.enable_episode_stats()
    r = to_numpy(sim.rollout_policy(policy, ROWS[game], seed=SEED[game]))
    stats = {name: cpu(getattr(sim, name)()) for name in STATS}
    sim.close()
    for got, want, name in zip(r, c["rollout"], Rollout._fields):
        same_bits(got, want, f"{name} with statistics enabled")
    other = replay(game, n, r.actions, stats=True)
    for name in STATS:
        same_bits(stats[name], other["stats"][name], name)
    assert stats["episode_totals_tensor"][:, 0].sum() == (np.concatenate([r.dones[1:], r.next_done[None]]) != 0).sum()
    # after prepare_graph_capture (run eagerly): the same results
    sim = prepare(game, n)
    sim.prepare_graph_capture()
    r = to_numpy(sim.rollout_policy(policy, ROWS[game], seed=SEED[game]))
    final = snapshot(sim)
    sim.close()
    for got, want, name in zip(r, c["rollout"], Rollout._fields):
        same_bits(got, want, f"{name} after prepare_graph_capture")
    for name in ("observation_tensor", "reset_tensor", "action_tensor", "reward_tensor"):
        same_bits(final[name], c["final"][name], f"final {name}")


def test_zero_steps_writes_the_closing_row_only(hip_lib):
    agent, policy = make_policy("cartpole", 1.0)
    sim = prepare("cartpole", 63)
    before = snapshot(sim)
    r = to_numpy(sim.rollout_policy(policy, 0))
    assert r.obs.shape == (0, 63, 4) and r.actions.shape == (0, 63)
    same_bits(r.next_obs, before["observation_tensor"], "next_obs")
    assert not r.next_done.any()
    want = twin.forward(policy.params.cpu().numpy(), r.next_obs, 2)[0]
    assert np.abs(r.next_value - want).max() <= 8 * twin.margins(agent, policy.params.cpu().numpy(), r.next_obs, np.zeros(63, np.int32))[0]
    after = snapshot(sim)
    for name in before:
        same_bits(before[name], after[name], name)
    sim.close()


@pytest.mark.parametrize("num_steps", [1, 32])
@pytest.mark.parametrize("n", SIZES)
def test_gae(n, num_steps, hip_lib):
    """against the float64 twin within 8 x the float32 torch loop's own distance from it"""
    case = twin.gae_case(num_steps, n, np.random.default_rng(100 * n + num_steps))
    rewards, values, dones, next_value, next_done = case
    want_adv, want_ret = twin.gae(*case, 0.99, 0.95)
    adv32, ret32 = twin.gae_loop_torch(*[torch.from_numpy(a) for a in case], 0.99, 0.95)
    d = max(np.abs(adv32.numpy() - want_adv).max(), np.abs(ret32.numpy() - want_ret).max())
    empty = torch.empty(0, device="cuda:0")
    rollout = Rollout(empty, empty, empty, torch.from_numpy(values).cuda(), torch.from_numpy(rewards).cuda(),
                      torch.from_numpy(dones).cuda(), empty, torch.from_numpy(next_value).cuda(), torch.from_numpy(next_done).cuda())
    adv, ret = gae(rollout, 0.99, 0.95)
    err = max(np.abs(cpu(adv) - want_adv).max(), np.abs(cpu(ret) - want_ret).max())
    print(f"gae n={n} T={num_steps}: {err:.3g} from the twin, d = {d:.3g}" + (f" ({err / d:.2f} d)" if d else ""))
    assert adv.shape == (num_steps, n) and ret.shape == (num_steps, n) and adv.dtype == torch.float32
    assert err <= 8 * d  # (d is 0 only where float32 was exact, and the kernel runs the same IEEE operations in the same order)
    # a world done at every step never bootstraps
    assert np.abs(cpu(adv)[:, 0] - (rewards[:, 0].astype(np.float64) - values[:, 0])).max() <= 8 * d


def _raw_call(sim, policy, steps, drop=None, no_policy=False, no_buffers=False, no_params=False):
    """mrl_rollout_policy through ctypes with one pointer missing -> (return code, message)"""
    n, device = sim.num_worlds, "cuda:0"
    shapes = Rollout((steps, n, 4), (steps, n), (steps, n), (steps, n), (steps, n), (steps, n), (n, 4), (n,), (n,))
    tensors = [torch.zeros(shape, dtype=torch.int32 if name == "actions" else torch.float32, device=device)
               for name, shape in zip(Rollout._fields, shapes)]
    pointers = [None if name == drop else t.data_ptr() for name, t in zip(Rollout._fields, tensors)]
    desc = _lib.MlpPolicyDesc(None if no_params else policy.params.data_ptr(), 4, 64, policy.num_actions, _lib.OBS_RAW, 0)
    buffers = _lib.RolloutBuffers(*pointers, steps)
    L = _lib.lib()
    rc = L.mrl_rollout_policy(sim._handle, None if no_policy else ctypes.byref(desc), None if no_buffers else ctypes.byref(buffers),
                              0, 0, None)
    torch.cuda.synchronize()
    return rc, L.mrl_last_error().decode()


@pytest.mark.parametrize("game", GAMES)
def test_refusals(game, hip_lib):
    n = 63
    _, good = make_policy(game, 1.0)
    sim, clean = prepare(game, n), prepare(game, n)
    refused = []

    def refuse(call, what):
        with pytest.raises(_lib.MrlError) as info:
            call()
        assert str(info.value), what
        refused.append(what)

    dev = "cuda:0"
    refuse(lambda: sim.rollout_policy(MlpPolicy(4, ACTIONS[game], hidden=32, device=dev), 2), "hidden != 64")
    refuse(lambda: sim.rollout_policy(MlpPolicy(4, 5 - ACTIONS[game], device=dev), 2), "the other game's num_actions")
    refuse(lambda: sim.rollout_policy(MlpPolicy(4, ACTIONS[game], observation="gym", device=dev), 2), "(4, gym)")
    refuse(lambda: sim.rollout_policy(MlpPolicy(6, ACTIONS[game], observation="state", device=dev), 2), "(6, raw)")
    refuse(lambda: sim.rollout_policy(MlpPolicy(5, ACTIONS[game], device=dev), 2), "obs_dim 5")
    if game == "cartpole":
        refuse(lambda: sim.rollout_policy(MlpPolicy(6, 2, observation="gym", device=dev), 2), "(6, gym) on Cartpole")
    for kwargs in ([dict(drop=name) for name in Rollout._fields] + [dict(no_policy=True), dict(no_buffers=True), dict(no_params=True)]):
        rc, message = _raw_call(sim, good, 2, **kwargs)
        assert rc == _lib.MRL_ERR_INVALID and "null" in message, kwargs
    for name in ("next_obs", "next_value", "next_done"):  # needed even for zero steps
        rc, message = _raw_call(sim, good, 0, drop=name)
        assert rc == _lib.MRL_ERR_INVALID and message
    assert _raw_call(sim, good, 0, drop="obs")[0] == _lib.MRL_OK  # ... the (T, ...) arrays are not
    # a capturing stream, wherever mrl_step refuses one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=dev)
    out = sim.rollout_policy(good, 2)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                sim.rollout_policy(good, 2, out=out)
            scratch.add_(0)
    torch.cuda.synchronize()
    # the simulator still steps normally: it is where a clean one is after the same two steps
    clean.step_sequence(out.actions.view(2, n, 1))
    same_simulator(snapshot(sim), snapshot(clean), "after the refusals")
    # (with the same actions: the rollout left its last row in sim's ACTION tensor, step_sequence leaves clean's alone)
    sim.step_with_actions(out.actions[0])
    clean.step_with_actions(out.actions[0])
    same_simulator(snapshot(sim), snapshot(clean), "a step after the refusals")
    assert len(refused) == (6 if game == "cartpole" else 5)
    # a rank of an exchanged batch
    sim.exchange_create(1, 0)
    refuse(lambda: sim.rollout_policy(good, 2), "after mrl_exchange_create")
    sim.step_with_actions(out.actions[1])
    clean.step_with_actions(out.actions[1])
    same_simulator(snapshot(sim), snapshot(clean), "a step after the last refusal")
    sim.close()
    clean.close()


def test_other_games_are_refused(hip_lib):
    sim = BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=8)
    before = cpu(sim.observation_tensor())
    with pytest.raises(_lib.MrlError, match="Cartpole and Acrobot"):
        sim.rollout_policy(MlpPolicy(4, 2, device="cuda:0"), 2)
    same_bits(cpu(sim.observation_tensor()), before, "the balance beam's observations")
    sim.step()
    torch.cuda.synchronize()
    sim.close()


@pytest.mark.parametrize("game", GAMES)
def test_env_wrapper_passes_its_observation_mode(game, hip_lib):
    from madrona_rl_envs_playground_amd.envs.acrobot_env import AcrobotMadronaTorch
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    if game == "cartpole":
        env = CartpoleMadronaTorch(63, 0)
        _, policy = make_policy(game, 1.0)
    else:
        env = AcrobotMadronaTorch(63, 0, observation="gym")
        _, policy = make_policy(game, 1.0, observation="gym")
        with pytest.raises(ValueError, match="observes"):
            env.rollout(make_policy(game, 1.0)[1], 2)
    first = env.reset().clone()
    r = env.rollout(policy, 3, seed=9)
    assert r.obs.shape == (3, 63) + tuple(env.single_observation_space.shape)
    assert torch.allclose(r.obs[0], first, rtol=0, atol=1e-6)
    assert torch.allclose(r.next_obs, env.reset(), rtol=0, atol=1e-6)
    advantages, returns = gae(r, 0.99, 0.95)
    assert advantages.shape == (3, 63) and torch.equal(returns, advantages + r.values)
    env.close()
