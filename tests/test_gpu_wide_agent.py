"""GPU: ``mrl_agent_act`` / ``mrl_agent_credit`` / ``mrl_gae_active`` and ``CleanPPOAgent`` on Hanabi and the balance beam.

Forward cases (tests/wide_twin.py, CASES x WEIGHTS): the test WRITES the case's inputs -- state / observation rows, masks, the
activity flags -- into the simulator's own tensors (they are what the kernels read, in place, in their element types and at
their strides), so the CPU tests know every input without a simulator.  Sizes 1, 31, 33, 65, 257: one row, the tails around a
32-row tile, two tiles and a tail, more than one workgroup per net; the balance beam's K = 7 is the ragged first layer, Hanabi
`full` the 658 / 783-wide one.

Margins: values and log-probs within 8 d of the float64 twin, d = torch float32's distance from the twin on the same inputs,
the largest over the sizes of a game at the same weight set.  Actions must be the twin's except where u
lies within 1e-5 of a boundary (tests/test_wide_agent_api.py counts those rows: at most 1 %).  Each test prints its ratios."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wide_twin as twin  # noqa: E402
from conftest import load_golden  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs.hanabi_env import config_choice  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AgentRecord, BalanceBeamSimulator, CartpoleSimulator, ExecMode,  # noqa: E402
                                                         HanabiSimulator, WidePolicy, agent_act, agent_credit, gae_active)

DEV = torch.device("cuda", 0)
WEIGHTS = sorted(twin.WEIGHTS)
TENSORS = ("done_tensor", "active_agent_tensor", "observation_tensor", "agent_state_tensor", "action_mask_tensor", "reward_tensor")


def make_sim(game, n):
    if game == "balance":
        return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    c = config_choice[game[len("hanabi_"):]]
    return HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, colors=c["colors"], ranks=c["ranks"], players=c["players"],
                           max_information_tokens=c["max_information_tokens"], max_life_tokens=c["max_life_tokens"])


def cpu(t):
    return (t.to_torch() if hasattr(t, "to_torch") else t).cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def snapshot(sim):
    return {name: cpu(getattr(sim, name)()) for name in TENSORS}


def new_record(sim, game, num_steps, logits=False):
    d, s, a = twin.dims(game)
    return AgentRecord(num_steps, sim.num_worlds, d, s, a, sim.observation_tensor().to_torch().dtype,
                       sim.agent_state_tensor().to_torch().dtype, DEV, logits=logits)


def write_inputs(sim, game, inputs, player):
    d, s, a = twin.dims(game)
    sim.agent_state_tensor().to_torch()[player, :, :s] = torch.from_numpy(inputs["state"]).to(DEV)
    sim.action_mask_tensor().to_torch()[player, :, :a] = torch.from_numpy(inputs["mask"]).to(DEV)
    sim.active_agent_tensor().to_torch()[player] = torch.from_numpy(inputs["active"]).to(DEV)
    torch.cuda.synchronize()
    same_bits(cpu(sim.observation_tensor())[player][:, :d], inputs["obs"], "the observation is the head of the state row")


RECORDED = ("obs", "states", "action_masks", "active", "actions", "logprobs", "values", "dones", "rewards", "last_active", "new_game",
            "next_done", "logits")


def record_arrays(record):
    return {name: cpu(getattr(record, name)) for name in RECORDED}


@functools.lru_cache(maxsize=None)
def forward_case(game, n, weights):
    """One case, run once and shared: the default act, the same again, ALL_ROWS and GREEDY, each into row 1 of a fresh record."""
    seed = twin.case_seed(game, n, weights)
    player = n % 2
    agent = twin.make_agent(game, weights)
    policy = WidePolicy.from_module(agent, device=DEV)
    inputs = twin.case_inputs(game, n, seed)
    sim = make_sim(game, n)
    write_inputs(sim, game, inputs, player)
    runs = {}
    for name, kwargs in (("default", {}), ("again", {}), ("all_rows", {"all_rows": True}), ("greedy", {"greedy": True})):
        record = new_record(sim, game, 2, logits=True)
        record.next_done[:] = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.uint8)).to(DEV)
        record.new_game.fill_(1)
        record.rewards.fill_(5.0)
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, record, row=1, seed=seed, step=0, **kwargs)
        torch.cuda.synchronize()
        runs[name] = record_arrays(record)
        runs[name]["action_tensor"] = cpu(sim.action_tensor())
    sim.close()
    u = twin.draws(seed, 0, n, player)
    return {"agent": agent, "inputs": inputs, "runs": runs, "u": u, "player": player,
            "twin": twin.act(twin.flat(agent), inputs["obs"], inputs["state"], inputs["mask"], u)}


@functools.lru_cache(maxsize=None)
def margins(game, weights):
    """d of a game at one weight set: the largest over its sizes (a scalar-like quantity; DESIGN.md sections 13 and 14)"""
    agent = twin.make_agent(game, weights)
    per_size = [twin.margins(agent, twin.case_inputs(g, n, twin.case_seed(g, n, weights))) for g, n in twin.CASES if g == game]
    return max(m[0] for m in per_size), max(m[1] for m in per_size)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_forward_pass_and_head(game, n, weights, hip_lib):
    c = forward_case(game, n, weights)
    got, want, inputs = c["runs"]["default"], c["twin"], c["inputs"]
    active, legal, rows = inputs["active"] != 0, inputs["mask"] != 0, np.arange(n)
    d_logp = margins(game, weights)[1]
    actions = got["actions"][1]
    err_logp = np.abs(got["logprobs"][1].astype(np.float64) - want["logp"][rows, actions])[active].max()  # teacher-forced
    print(f"{game} n={n} {weights}: log-probs {err_logp / d_logp:.2f} d (d = {d_logp:.3e})")
    assert err_logp <= 8 * d_logp
    assert legal[rows, actions][active].all()
    keep = active & ~twin.near_boundary(want["cdf"], c["u"])
    assert keep.sum() >= active.sum() - 0.01 * n
    assert np.array_equal(actions[keep], want["actions"][keep])
    # inactive rows
    for name in ("actions", "logprobs", "values"):
        assert (got[name][1][~active] == 0).all(), name
    player_actions = got["action_tensor"][c["player"], :, 0]
    same_bits(player_actions, actions, "the ACTION tensor")
    assert (got["action_tensor"][1 - c["player"]] == -7).all()  # the other seat is not this agent's
    # the record: copies in the inputs' own element types, inactive rows included; row 0 untouched
    same_bits(got["obs"][1], inputs["obs"], "recorded obs")
    same_bits(got["states"][1], inputs["state"], "recorded states")
    same_bits(got["action_masks"][1], legal.astype(np.uint8), "recorded masks")
    same_bits(got["active"][1], active.astype(np.uint8), "recorded active")
    same_bits(got["dones"][1], (rows % 3 == 0).astype(np.float32), "dones = next_done")
    assert not got["next_done"].any() and (got["rewards"][1] == 0).all() and (got["rewards"][0] == 5).all()
    same_bits(got["last_active"], np.where(active, 1, 0).astype(np.int32), "last_active")
    same_bits(got["new_game"], np.where(active, 0, 1).astype(np.uint8), "new_game")
    assert not got["obs"][0].any() and not got["active"][0].any()
    # the same seed gives the same bits
    for name in RECORDED:
        same_bits(c["runs"]["again"][name], got[name], f"{name} of a second run")


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_values_within_8_d_of_the_twin(game, n, weights, hip_lib):
    """The critic's values of the active rows, and of every row under ALL_ROWS, against the float64 twin.

    d is 4.5 - 9.3e-9, about one ulp of a value of 0.07: this is the test that tells where the bias is added.  A chain begun
    at the bias measured 6.2 - 16.8 d here (512 products of 2e-4 each rounded at the ulp of a bias of 0.07); with the bias
    added to the finished sum an MI355X measures 0.15 - 2.81 d."""
    c = forward_case(game, n, weights)
    active = c["inputs"]["active"] != 0
    d_value = margins(game, weights)[0]
    err = max(np.abs(c["runs"]["default"]["values"][1] - c["twin"]["values"])[active].max(),
              np.abs(c["runs"]["all_rows"]["values"][1] - c["twin"]["values"]).max())
    print(f"{game} n={n} {weights}: values {err / d_value:.2f} d (d = {d_value:.3e}, err = {err:.3e})")
    assert err <= 8 * d_value


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_all_rows_and_greedy(game, n, weights, hip_lib):
    c = forward_case(game, n, weights)
    default, every, greedy, inputs = c["runs"]["default"], c["runs"]["all_rows"], c["runs"]["greedy"], c["inputs"]
    active, legal, rows = inputs["active"] != 0, inputs["mask"] != 0, np.arange(n)
    for name in ("actions", "logprobs", "values"):
        same_bits(every[name][1][active], default[name][1][active], f"{name} of the active rows under ALL_ROWS")
    same_bits(every["logits"][active], default["logits"][active], "logits")
    d_logp = margins(game, weights)[1]
    assert np.abs(every["logprobs"][1].astype(np.float64) - c["twin"]["logp"][rows, every["actions"][1]]).max() <= 8 * d_logp
    assert legal[rows, every["actions"][1]].all()
    same_bits(every["active"][1], active.astype(np.uint8), "ALL_ROWS records the real flags")
    # GREEDY: the first legal arg-max of the device's own logits
    a = legal.shape[1]
    first = np.where(legal, greedy["logits"][:, :a], -np.inf).argmax(axis=1)
    assert np.array_equal(greedy["actions"][1][active], first[active])
    same_bits(greedy["values"][1], default["values"][1], "values under GREEDY")


def test_operand_maps_with_exact_integers(hip_lib):
    """Integer weights and 0 / 1 inputs whose every partial sum is an integer below 2^24: float32 is exact whatever the order,
    so a wrong lane map, a transposed tile or a dropped k shows as a wrong integer.  Logits and values are compared bit for bit."""
    game, n, player = "hanabi_very_small", 65, 1
    d, s, a = twin.dims(game)
    rng = np.random.default_rng(99)
    policy = WidePolicy(d, s, a, device=DEV)
    layers, flat = {}, []
    for name, first, out in (("critic", s, 1), ("actor", d, a)):
        layers[name] = []
        for k, (rows, cols) in enumerate(((512, first), (512, 512), (512, 512), (out, 512))):
            density = 1.0 if k == 0 else 1.0 / 32
            w = (rng.integers(-2, 3, size=(rows, cols)) * (rng.uniform(size=(rows, cols)) < density)).astype(np.int64)
            w += (np.arange(rows)[:, None] % 3 == 0) & (np.arange(cols)[None, :] % 7 == 0)  # (asymmetric in row and column)
            b = rng.integers(-3, 4, size=rows).astype(np.int64)
            layers[name].append((w, b))
            flat += [w.reshape(-1), b]
    policy.params.copy_(torch.from_numpy(np.concatenate(flat).astype(np.float32)))
    inputs = twin.case_inputs(game, n, 4242)
    exact = {}
    for name, x in (("critic", inputs["state"].astype(np.int64)), ("actor", inputs["obs"].astype(np.int64))):
        for k, (w, b) in enumerate(layers[name]):
            assert (np.abs(x) @ np.abs(w).T + np.abs(b)).max() < 2 ** 24
            x = x @ w.T + b
            if k < 3:
                x = np.maximum(x, 0)
        exact[name] = x
    assert len(np.unique(exact["actor"])) > n and exact["actor"].std(axis=0).min() > 0 and exact["actor"].std(axis=1).min() > 0
    sim = make_sim(game, n)
    write_inputs(sim, game, inputs, player)
    record = new_record(sim, game, 1, logits=True)
    agent_act(sim, player, policy, record, row=0, seed=1, step=0, all_rows=True)
    torch.cuda.synchronize()
    same_bits(cpu(record.logits)[:, :a], exact["actor"].astype(np.float32), "logits")
    same_bits(cpu(record.values)[0], exact["critic"][:, 0].astype(np.float32), "values")
    sim.close()


def collect(game, n, num_steps, prepare=None, seed=77):
    """``num_steps`` steps of both seats under one policy each, recorded; the ACTION tensor in front of every step."""
    sim = make_sim(game, n)
    if prepare:
        prepare(sim)
    policies = [WidePolicy.from_module(twin.make_agent(game, w, seed=21 + p), device=DEV) for p, w in enumerate(WEIGHTS)]
    records = [new_record(sim, game, num_steps) for _ in range(2)]
    trace = {"actions": [], "before": [], "rewards": [], "dones": [], "after": []}
    for t in range(num_steps):
        trace["before"].append(snapshot(sim))
        for p in range(2):
            agent_act(sim, p, policies[p], records[p], row=t, seed=seed, step=t)
        trace["actions"].append(sim.action_tensor().to_torch().clone())
        sim.step()
        rewards, dones = sim.reward_tensor().to_torch(), sim.done_tensor().to_torch()
        for p in range(2):
            agent_credit(records[p], rewards[p], dones)
        trace["rewards"].append(cpu(rewards))
        trace["dones"].append(cpu(dones))
        trace["after"].append(snapshot(sim))
    torch.cuda.synchronize()
    out = {"records": [dict(record_arrays_no_logits(r), running_rewards=cpu(r.running_rewards), totals=cpu(r.totals)) for r in records],
           "trace": trace, "actions": [cpu(x) for x in trace["actions"]]}
    sim.close()
    return out


def record_arrays_no_logits(record):
    return {name: cpu(getattr(record, name)) for name in RECORDED if name != "logits"}


@pytest.mark.parametrize("game", ["balance", "hanabi_very_small"])
def test_environment_parity_recording_and_credit(game, hip_lib):
    n, num_steps = 33, 16
    d, s, a = twin.dims(game)
    c = collect(game, n, num_steps)
    # a second simulator stepped with the recorded actions sees the same things
    other = make_sim(game, n)
    for t in range(num_steps):
        other.step_with_actions(c["trace"]["actions"][t])
        now = snapshot(other)
        for name in TENSORS:
            same_bits(now[name], c["trace"]["after"][t][name], f"{name} after step {t}")
    other.close()
    finished = sum(int(x.sum()) for x in c["trace"]["dones"])
    if game == "balance":
        assert finished > 0
    for p in range(2):
        rec, numpy_rec, returns = c["records"][p], twin.new_record(num_steps, n), []
        for t in range(num_steps):
            before = c["trace"]["before"][t]
            active = before["active_agent_tensor"][p] != 0
            legal = before["action_mask_tensor"][p][:, :a] != 0
            same_bits(rec["obs"][t], before["observation_tensor"][p][:, :d], f"obs row {t}")
            same_bits(rec["states"][t], before["agent_state_tensor"][p][:, :s], f"states row {t}")
            same_bits(rec["action_masks"][t], legal.astype(np.uint8), f"masks row {t}")
            same_bits(rec["actions"][t], c["actions"][t][p, :, 0], f"actions row {t}")
            assert legal[np.arange(n), rec["actions"][t]][active].all() and (rec["actions"][t][~active] == 0).all()
            twin.book(numpy_rec, t, active)
            returns.append(twin.credit(numpy_rec, c["trace"]["rewards"][t][p], c["trace"]["dones"][t]))
        for name in ("active", "dones", "rewards", "last_active", "new_game", "next_done", "running_rewards"):
            same_bits(rec[name], numpy_rec[name], f"player {p}: {name}")
        assert rec["totals"][:, 0].sum() == finished == numpy_rec["totals"][:, 0].sum()
        assert np.array_equal(rec["totals"][:, 2:], numpy_rec["totals"][:, 2:])
        assert abs(rec["totals"][0, 1] - numpy_rec["totals"][0, 1]) <= 8 * twin.sum_margin(np.concatenate(returns))


def test_credit_over_several_blocks(hip_lib):
    """2500 worlds = three blocks of totals; per-world arrays bit for bit, the sum within 8 d, d = a float32 running sum's
    distance from the float64 total of the same returns."""
    n, num_steps = 2500, 4
    rng = np.random.default_rng(3)
    record = AgentRecord(num_steps, n, 1, 1, 1, torch.int8, torch.int8, DEV)
    numpy_rec = twin.new_record(num_steps, n)
    numpy_rec["last_active"][:] = rng.integers(0, num_steps, size=n)
    numpy_rec["new_game"][:] = rng.uniform(size=n) < 0.3
    record.last_active.copy_(torch.from_numpy(numpy_rec["last_active"]))
    record.new_game.copy_(torch.from_numpy(numpy_rec["new_game"]))
    finished = []
    for k in range(6):
        rewards = rng.normal(size=n).astype(np.float32)
        dones = (rng.uniform(size=n) < 0.2).astype(np.int32)
        if k % 2:
            dones[1024:2048] = 0  # (a block with nothing finished leaves its row of the totals alone)
        agent_credit(record, torch.from_numpy(rewards).to(DEV), torch.from_numpy(dones).to(DEV))
        finished.append(twin.credit(numpy_rec, rewards, dones))
    torch.cuda.synchronize()
    for name in ("rewards", "last_active", "new_game", "next_done", "running_rewards"):
        same_bits(cpu(getattr(record, name)), numpy_rec[name], name)
    totals = cpu(record.totals)
    assert np.array_equal(totals[:, 0], numpy_rec["totals"][:, 0]) and np.array_equal(totals[:, 2:], numpy_rec["totals"][:, 2:])
    every = np.concatenate(finished)
    d = twin.sum_margin(every)
    err = np.abs(totals[:, 1] - numpy_rec["totals"][:, 1]).max()
    print(f"sum of returns: {err:.3e} from the restatement, d = {d:.3e}")
    assert d > 0 and err <= 8 * d
    assert record.episode_totals()[0] == len(every)


def run_gae(rewards, values, dones, active, next_done, next_value, next_active, gamma, gae_lambda):
    num_steps, n = rewards.shape
    record = AgentRecord(num_steps, n, 1, 1, 1, torch.int8, torch.int8, DEV)
    for name, array, dtype in (("rewards", rewards, np.float32), ("values", values, np.float32), ("dones", dones, np.float32),
                               ("active", active, np.uint8), ("next_done", next_done, np.uint8), ("next_value", next_value, np.float32),
                               ("next_active", next_active, np.uint8)):
        getattr(record, name).copy_(torch.from_numpy(np.ascontiguousarray(array).astype(dtype)))
    adv, ret = gae_active(record, gamma, gae_lambda)
    torch.cuda.synchronize()
    return cpu(adv), cpu(ret), cpu(record.active)


@pytest.mark.parametrize("regime,n", [(regime, n) for n in (5, 70) for regime in ("coupled", "together")])
def test_gae_active_equals_the_reference_fixture(regime, n, hip_lib):
    g = load_golden("cleanppo_gae.npz")
    f = {k[len(f"{regime}_{n}_"):]: v for k, v in g.items() if k.startswith(f"{regime}_{n}_")}
    adv, ret, active = run_gae(f["before_rewards"], f["before_values"], f["before_dones"], f["before_active"], f["before_next_done"],
                               f["next_value"], f["activity"][8], float(f["gamma"]), float(f["gae_lambda"]))
    same_bits(adv, f["advantages"], "advantages")
    same_bits(ret, f["returns"], "returns")
    same_bits(active != 0, f["active_after"], "active afterwards")


@pytest.mark.parametrize("coupled", [False, True])
def test_gae_active_over_several_workgroups(coupled, hip_lib):
    n, num_steps = 700, 8
    rng = np.random.default_rng(12 + coupled)
    active = rng.uniform(size=(num_steps, n)) < 0.5
    next_active = rng.uniform(size=n) < 0.5
    if not coupled:
        next_active[:] = True
    else:
        active[:, 5], next_active[5] = False, False  # a world that never acts: the coupling holds at every step
    rewards = rng.choice([1.0, -1.0, 0.0], size=(num_steps, n)).astype(np.float32)
    values = rng.normal(scale=3.0, size=(num_steps, n)).astype(np.float32)
    dones = (rng.uniform(size=(num_steps, n)) < 0.1).astype(np.float32)
    next_done = rng.uniform(size=n) < 0.1
    next_value = rng.normal(scale=3.0, size=n).astype(np.float32)
    want = twin.gae_active(rewards, values, dones, active, next_done, next_value, next_active, 0.99, 0.95)
    got = run_gae(rewards, values, dones, active, next_done, next_value, next_active, 0.99, 0.95)
    same_bits(got[0], want[0], "advantages")
    same_bits(got[1], want[1], "returns")
    same_bits(got[2] != 0, want[2], "active afterwards")


def test_one_full_update(hip_lib):
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent
    n, num_steps, game = 33, 8, "hanabi_very_small"
    torch.manual_seed(0)
    env = HanabiMadrona(n, 0, config=config_choice["very_small"])
    ego = CleanPPOAgent(env, "ego", DEV, num_updates=2, verbose=False, num_steps=num_steps, seed=5)
    partner = CleanPPOAgent(env.getDummyEnv(1), "partner", DEV, num_updates=2, verbose=False, num_steps=num_steps)
    env.add_partner_agent(partner, player_num=1)
    assert (ego.seat, partner.seat) == (0, 1) and ego.seed == 5 and partner.seed != 5
    obs = env.reset()
    for _ in range(num_steps):
        action = ego.get_action(obs)
        assert action.shape == (n, 1) and action.data_ptr() == env.static_actions[0].data_ptr()
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    torch.cuda.synchronize()
    assert ego.global_step == num_steps and partner.global_step == num_steps and ego.updates == 1
    before = ego.policy.params.clone()
    old_agent = twin.make_agent(game, "orthogonal")
    torch.nn.utils.vector_to_parameters(before.cpu(), old_agent.parameters())
    ego.get_action(obs)  # the update boundary: bootstrap value, advantages, the epochs, then row 0 of the next rollout
    torch.cuda.synchronize()
    assert ego.updates == 2 and ego.step == 0
    after = ego.policy.params
    assert not torch.equal(after, before) and torch.isfinite(after).all()
    assert torch.equal(after, torch.nn.utils.parameters_to_vector(ego.agent.parameters()))
    for key, value in ego.last_losses.items():
        assert np.isfinite(value) or key == "explained_variance", key
    assert ego.last_losses["samples"] > 1 and ego.last_losses["learning_rate"] == 2.5e-4
    # the act behind the update read the new parameters: row 0 holds their values, not the old ones'
    r = ego.record
    active = cpu(r.active)[0] != 0
    inputs = {"obs": cpu(r.obs)[0], "state": cpu(r.states)[0], "mask": cpu(r.action_masks)[0]}
    new_agent = twin.make_agent(game, "orthogonal")
    torch.nn.utils.vector_to_parameters(after.cpu(), new_agent.parameters())
    values = cpu(r.values)[0]
    new_twin = twin.forward(twin.flat(new_agent), inputs["obs"], inputs["state"], twin.dims(game)[2])[0]
    old_twin = twin.forward(twin.flat(old_agent), inputs["obs"], inputs["state"], twin.dims(game)[2])[0]
    # float32 rounding keeps the forward pass within K eps sum |x w| ~ 512 x 6e-8 x 0.1 = 3e-6 of the twin; four Adam steps of
    # 2.5e-4 on every weight move a value by far more
    assert np.abs(values - new_twin)[active].max() <= 1e-5 < 1e-4 <= np.abs(values - old_twin)[active].max()
    env.close()


def test_graph_capture_mode_and_episode_statistics_leave_the_results_alone(hip_lib):
    for game in ("balance", "hanabi_very_small"):
        plain = collect(game, 33, 4)
        for prepare in (lambda sim: sim.prepare_graph_capture(), lambda sim: sim.enable_episode_stats()):
            other = collect(game, 33, 4, prepare=prepare)
            for t in range(4):
                same_bits(other["actions"][t], plain["actions"][t], f"{game}: actions of step {t}")
                for name in TENSORS:
                    same_bits(other["trace"]["after"][t][name], plain["trace"]["after"][t][name], f"{game}: {name} after step {t}")
            for p in range(2):
                for name in ("logprobs", "values", "rewards", "running_rewards"):
                    same_bits(other["records"][p][name], plain["records"][p][name], name)


def raw_act(sim, player=0, policy="good", record="good", row=0, flags=0, workspace="good", drop=None, num_actions=4):
    good_policy = WidePolicy(7, 7, 4, device=DEV)
    rec = AgentRecord(2, sim.num_worlds, 7, 7, 4, torch.int32, torch.int32, DEV)
    desc = good_policy.desc()
    desc.num_actions = num_actions
    if policy == "no_params":
        desc.params_dev = None
    struct = rec.struct
    if drop:
        setattr(struct, drop, None)
    rc = _lib.lib().mrl_agent_act(sim._handle, player, ctypes.byref(desc) if policy != "none" else None,
                                  ctypes.byref(struct) if record == "good" else None, row, 0, 0, flags,
                                  rec.workspace.data_ptr() if workspace == "good" else None, None)
    torch.cuda.synchronize()
    return rc, _lib.lib().mrl_last_error().decode()


def test_refusals(hip_lib):
    n = 33
    sim, clean = make_sim("balance", n), make_sim("balance", n)
    assert raw_act(sim)[0] == _lib.MRL_OK and raw_act(clean)[0] == _lib.MRL_OK
    refusals = [dict(policy="none"), dict(policy="no_params"), dict(workspace="none"), dict(num_actions=65), dict(num_actions=0),
                dict(num_actions=5), dict(player=2), dict(row=2), dict(record="none", flags=_lib.AGENT_VALUE_ONLY)]
    refusals += [dict(drop=name) for name in _lib.AGENT_RECORD_BUFFERS if name != "logits"]
    for kwargs in refusals:
        rc, message = raw_act(sim, **kwargs)
        assert rc == _lib.MRL_ERR_INVALID and message.startswith("mrl_agent_act"), kwargs
    assert raw_act(sim, drop="logits")[0] == _lib.MRL_OK  # (optional)
    policy = WidePolicy(7, 7, 4, device=DEV)
    record = new_record(sim, "balance", 2)
    # a wrong game
    cartpole = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=8)
    with pytest.raises(_lib.MrlError, match="Hanabi and the balance beam"):
        agent_act(cartpole, 0, policy, workspace=record.workspace)
    cartpole.close()
    # NULL pointers of the other two calls
    L = _lib.lib()
    assert L.mrl_agent_credit(None, None, None, n, 0, None) == _lib.MRL_ERR_INVALID
    assert L.mrl_agent_credit(ctypes.byref(record.struct), None, record.actions.data_ptr(), n, 0, None) == _lib.MRL_ERR_INVALID
    assert L.mrl_agent_credit(ctypes.byref(record.struct), record.rewards.data_ptr(), record.actions.data_ptr(), n + 1, 0, None) == \
        _lib.MRL_ERR_INVALID
    assert L.mrl_gae_active(None, None, None, 0.99, 0.95, None, None, 0, None) == _lib.MRL_ERR_INVALID
    assert L.mrl_gae_active(ctypes.byref(record.struct), record.next_value.data_ptr(), record.next_active.data_ptr(), 0.99, 0.95, None,
                            record.returns.data_ptr(), 0, None) == _lib.MRL_ERR_INVALID
    # a capturing stream, wherever mrl_step refuses one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                agent_act(sim, 0, policy, record, row=0)
            scratch.add_(0)
    torch.cuda.synchronize()
    # the simulator still steps normally: it is where a clean one is
    actions = sim.action_tensor().to_torch().clone()
    sim.step()
    clean.step_with_actions(actions)
    for name in TENSORS:
        same_bits(cpu(getattr(sim, name)()), cpu(getattr(clean, name)()), name)
    # a rank of an exchanged batch
    sim.exchange_create(1, 0)
    with pytest.raises(_lib.MrlError, match="mrl_exchange_create"):
        agent_act(sim, 0, policy, record, row=0)
    sim.close()
    clean.close()
