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
from madrona_rl_envs_playground_amd.simulators import (AgentRecord, BalanceBeamSimulator, CartpoleSimulator, ExecMode,  # noqa: E402
                                                         HanabiSimulator, WidePolicy, agent_act, agent_credit, gae_active)

DEV = torch.device("cuda", 0)
WEIGHTS = sorted(twin.WEIGHTS)
TENSORS = ("done_tensor", "active_agent_tensor", "observation_tensor", "agent_state_tensor", "action_mask_tensor", "reward_tensor")


def make_sim(game, n):
    """"balance", a named Hanabi game, or "hanabi_<id>" of tests/hanabi_configs.py"""
    if game == "balance":
        return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    c = twin.config_of(game)
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


def check_forward_pass_and_head(game, n, weights, d_logp):
    """The default act of one forward case against the twin and the inputs; ``d_logp``: the case's margin.  Returns the ratio."""
    c = forward_case(game, n, weights)
    got, want, inputs = c["runs"]["default"], c["twin"], c["inputs"]
    active, legal, rows = inputs["active"] != 0, inputs["mask"] != 0, np.arange(n)
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
    return err_logp / d_logp


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_forward_pass_and_head(game, n, weights, hip_lib):
    check_forward_pass_and_head(game, n, weights, margins(game, weights)[1])


def check_values(game, n, weights, d_value):
    """The critic's values of the active rows, and of every row under ALL_ROWS, within 8 ``d_value`` of the twin.  Returns the ratio."""
    c = forward_case(game, n, weights)
    active = c["inputs"]["active"] != 0
    err = max(np.abs(c["runs"]["default"]["values"][1] - c["twin"]["values"])[active].max(),
              np.abs(c["runs"]["all_rows"]["values"][1] - c["twin"]["values"]).max())
    print(f"{game} n={n} {weights}: values {err / d_value:.2f} d (d = {d_value:.3e}, err = {err:.3e})")
    assert err <= 8 * d_value
    return err / d_value


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_values_within_8_d_of_the_twin(game, n, weights, hip_lib):
    """The critic's values of the active rows, and of every row under ALL_ROWS, against the float64 twin.

    d is 4.5 - 9.3e-9, about one ulp of a value of 0.07: this is the test that tells where the bias is added.  A chain begun
    at the bias measured 6.2 - 16.8 d here (512 products of 2e-4 each rounded at the ulp of a bias of 0.07); with the bias
    added to the finished sum an MI355X measures 0.15 - 2.81 d."""
    check_values(game, n, weights, margins(game, weights)[0])


def check_all_rows_and_greedy(game, n, weights, d_logp):
    """ALL_ROWS and GREEDY of one forward case against its default act.  Returns the ratio of the log-probs under ALL_ROWS."""
    c = forward_case(game, n, weights)
    default, every, greedy, inputs = c["runs"]["default"], c["runs"]["all_rows"], c["runs"]["greedy"], c["inputs"]
    active, legal, rows = inputs["active"] != 0, inputs["mask"] != 0, np.arange(n)
    for name in ("actions", "logprobs", "values"):
        same_bits(every[name][1][active], default[name][1][active], f"{name} of the active rows under ALL_ROWS")
    same_bits(every["logits"][active], default["logits"][active], "logits")
    err_logp = np.abs(every["logprobs"][1].astype(np.float64) - c["twin"]["logp"][rows, every["actions"][1]]).max()
    print(f"{game} n={n} {weights}: log-probs under ALL_ROWS {err_logp / d_logp:.2f} d (d = {d_logp:.3e})")
    assert err_logp <= 8 * d_logp
    assert legal[rows, every["actions"][1]].all()
    same_bits(every["active"][1], active.astype(np.uint8), "ALL_ROWS records the real flags")
    # GREEDY: the first legal arg-max of the device's own logits
    a = legal.shape[1]
    first = np.where(legal, greedy["logits"][:, :a], -np.inf).argmax(axis=1)
    assert np.array_equal(greedy["actions"][1][active], first[active])
    same_bits(greedy["values"][1], default["values"][1], "values under GREEDY")
    return err_logp / d_logp


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CASES)
def test_all_rows_and_greedy(game, n, weights, hip_lib):
    check_all_rows_and_greedy(game, n, weights, margins(game, weights)[1])


def check_operand_maps(game, n, player):
    """Integer weights (``twin.integer_layers``) and 0 / 1 inputs whose every partial sum is an integer below 2^24: float32 is exact
    whatever the order, so a wrong lane map, a transposed tile or a dropped k shows as a wrong integer.  Logits and values of
    every row (ALL_ROWS) are compared bit for bit."""
    d, s, a = twin.dims(game)
    layers = twin.integer_layers(d, s, a)
    policy = WidePolicy(d, s, a, device=DEV)
    policy.params.copy_(torch.from_numpy(twin.integer_params(layers)))
    inputs = twin.case_inputs(game, n, twin.INTEGER_SEED)
    values, logits, bound = twin.integer_forward(layers, inputs["obs"], inputs["state"])
    assert bound < 2 ** 24
    assert len(np.unique(logits)) > n and logits.std(axis=0).min() > 0 and logits.std(axis=1).min() > 0
    sim = make_sim(game, n)
    write_inputs(sim, game, inputs, player)
    record = new_record(sim, game, 1, logits=True)
    agent_act(sim, player, policy, record, row=0, seed=1, step=0, all_rows=True)
    torch.cuda.synchronize()
    same_bits(cpu(record.logits)[:, :a], logits.astype(np.float32), "logits")
    assert not cpu(record.logits)[:, a:].any()
    same_bits(cpu(record.values)[0], values.astype(np.float32), "values")
    sim.close()


def test_operand_maps_with_exact_integers(hip_lib):
    """Integer weights and 0 / 1 inputs whose every partial sum is an integer below 2^24: float32 is exact whatever the order,
    so a wrong lane map, a transposed tile or a dropped k shows as a wrong integer.  Logits and values are compared bit for bit."""
    check_operand_maps("hanabi_very_small", 65, 1)


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


@pytest.mark.parametrize("game", ["hanabi_very_small", "hanabi_k5r4i8l3", "hanabi_k1r5i1l1"])
def test_one_full_update(game, hip_lib):
    """A rollout of ``CleanPPOAgent``, its update, and the act behind it.  k5r4i8l3: code variant 0, 542 / 642 wide, 19 actions;
    k1r5i1l1: no deck, episodes of two moves."""
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent
    n, num_steps = 33, 8
    d, s, a = twin.dims(game)
    torch.manual_seed(0)
    env = HanabiMadrona(n, 0, config=twin.config_of(game))
    ego = CleanPPOAgent(env, "ego", DEV, num_updates=2, verbose=False, num_steps=num_steps, seed=5)
    partner = CleanPPOAgent(env.getDummyEnv(1), "partner", DEV, num_updates=2, verbose=False, num_steps=num_steps)
    env.add_partner_agent(partner, player_num=1)
    assert (ego.seat, partner.seat) == (0, 1) and ego.seed == 5 and partner.seed != 5
    assert (ego.policy.obs_dim, ego.policy.state_dim, ego.policy.num_actions) == (d, s, a)
    obs = env.reset()
    for _ in range(num_steps):
        action = ego.get_action(obs)
        assert action.shape == (n, 1) and action.data_ptr() == env.static_actions[0].data_ptr()
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    torch.cuda.synchronize()
    assert ego.global_step == num_steps and partner.global_step == num_steps and ego.updates == 1
    assert ego.record.obs.shape == (num_steps, n, d) and ego.record.states.shape == (num_steps, n, s)
    assert ego.record.action_masks.shape == (num_steps, n, a)
    before = ego.policy.params.clone()
    old_agent = twin.make_agent(game, "orthogonal")
    torch.nn.utils.vector_to_parameters(before.cpu(), old_agent.parameters())
    ego.get_action(obs)  # the update boundary: bootstrap value, advantages, the epochs, then row 0 of the next rollout
    torch.cuda.synchronize()
    assert ego.updates == 2 and ego.step == 0
    after = ego.policy.params
    assert not torch.equal(after, before) and torch.isfinite(after).all()
    assert torch.equal(after, torch.nn.utils.parameters_to_vector(ego.agent.parameters()))
    at = after.data_ptr()
    for p in ego.agent.parameters():  # views of policy.params: the optimizer's step is what the kernels read
        assert p.untyped_storage().data_ptr() == after.untyped_storage().data_ptr() and p.data_ptr() == at
        at += 4 * p.numel()
    assert at == after.data_ptr() + 4 * after.numel()
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
    new_twin = twin.forward(twin.flat(new_agent), inputs["obs"], inputs["state"], a)[0]
    old_twin = twin.forward(twin.flat(old_agent), inputs["obs"], inputs["state"], a)[0]
    err_new, err_old = np.abs(values - new_twin)[active].max(), np.abs(values - old_twin)[active].max()
    if game == "hanabi_very_small":
        # float32 rounding keeps the forward pass within K eps sum |x w| ~ 512 x 6e-8 x 0.1 = 3e-6 of the twin; four Adam steps of
        # 2.5e-4 on every weight move a value by far more
        assert err_new <= 1e-5 < 1e-4 <= err_old
    else:
        # d: torch float32 against the twin on the recorded rows, at the new parameters; 100 x 8 d is the margin of
        # test_rollout_reads_the_updated_parameters
        d_value = twin.margins(new_agent, {name: x[active] for name, x in inputs.items()})[0]
        print(f"{game}: values of row 0 {err_new / d_value:.2f} d from the twin at the new parameters, {err_old / d_value:.0f} d from "
              f"the twin at the old ones (d = {d_value:.3e})")
        assert d_value > 0 and err_new <= 8 * d_value and err_old > 100 * 8 * d_value
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


# ---------------------------------------------------------------- modes, sizes and head edges beside the default act
#
# Past one pass of the world list, MRL_AGENT_VALUE_ONLY, an act without a record, draws at the ends of the 2^-24 grid, a world
# with no legal action, policies narrower than the simulator's rows, the workspace's bounds, a side stream.  Margins: d as
# above, the largest over the sizes of a game at a weight set, here over CASES and LARGE_CASES together; bound 8 d.

EVERY_BUFFER = RECORDED + ("running_rewards", "totals", "first_step", "next_value", "next_active", "advantages", "returns")


def every_buffer(record):
    return {name: cpu(getattr(record, name)) for name in EVERY_BUFFER if getattr(record, name) is not None}


@functools.lru_cache(maxsize=None)
def margins_of_every_size(game, weights):
    agent = twin.make_agent(game, weights)
    sizes = [n for g, n in twin.CASES if g == game] + [n for g, n, _, _ in twin.LARGE_CASES if g == game]
    per_size = [twin.margins(agent, twin.case_inputs(game, n, twin.case_seed(game, n, weights))) for n in sizes]
    return max(m[0] for m in per_size), max(m[1] for m in per_size)


def world_list(workspace, n):
    """the list of computed worlds an act left in its workspace and its length (the layout: csrc/wide_policy.hpp)"""
    raw = workspace.cpu().numpy()
    rows_bytes = (4 * n + 255) // 256 * 256 + 256
    count = int(raw[rows_bytes - 256:rows_bytes - 252].copy().view(np.uint32)[0])
    assert count <= n
    return raw[:4 * n].copy().view(np.uint32)[:count], count


def prepared_record(sim, game, num_steps, n, dims=None):
    """a record whose per-world state is not the initial one, so that what an act writes and what it leaves alone both show"""
    d, s, a = dims or twin.dims(game)
    record = AgentRecord(num_steps, n, d, s, a, sim.observation_tensor().to_torch().dtype, sim.agent_state_tensor().to_torch().dtype, DEV,
                         logits=True)
    record.next_done[:] = torch.from_numpy((np.arange(n) % 3 == 0).astype(np.uint8)).to(DEV)
    record.new_game.fill_(1)
    record.rewards.fill_(5.0)
    record.running_rewards.fill_(3.0)
    return record


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n,player,step", twin.LARGE_CASES)
def test_more_than_one_pass_of_the_world_list(game, n, player, step, weights, hip_lib):
    """Everything test_forward_pass_and_head and test_values_within_8_d_of_the_twin assert, past 1024 worlds and at a step other
    than 0, and the world list itself.  An MI355X measures log-probs 0.97 - 1.30 d and values 1.15 - 1.82 d."""
    seed = twin.case_seed(game, n, weights)
    agent = twin.make_agent(game, weights)
    policy = WidePolicy.from_module(agent, device=DEV)
    inputs = twin.case_inputs(game, n, seed)
    sim = make_sim(game, n)
    write_inputs(sim, game, inputs, player)
    runs = {}
    for name, kwargs in (("default", {}), ("again", {}), ("all_rows", {"all_rows": True})):
        record = prepared_record(sim, game, 2, n)
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, record, row=1, seed=seed, step=step, **kwargs)
        torch.cuda.synchronize()
        runs[name] = record_arrays(record)
        runs[name]["action_tensor"] = cpu(sim.action_tensor())
        runs[name]["list"] = world_list(record.workspace, n)
    sim.close()
    u = twin.draws(seed, step, n, player)
    want = twin.act(twin.flat(agent), inputs["obs"], inputs["state"], inputs["mask"], u)
    got, every = runs["default"], runs["all_rows"]
    active, legal, rows = inputs["active"] != 0, inputs["mask"] != 0, np.arange(n)
    assert active[1024:].any() and not active[:1024].all()  # (the last pass adds to the list; the list is not every world)
    # the world list: ascending, complete, its length beside it
    listed, count = got["list"]
    assert count == active.sum() and np.array_equal(listed, np.flatnonzero(active))
    listed, count = every["list"]
    assert count == n and np.array_equal(listed, rows)
    d_value, d_logp = margins_of_every_size(game, weights)
    actions = got["actions"][1]
    assert legal[rows, actions][active].all() and legal[rows, every["actions"][1]].all()
    err_logp = max(np.abs(got["logprobs"][1].astype(np.float64) - want["logp"][rows, actions])[active].max(),
                   np.abs(every["logprobs"][1].astype(np.float64) - want["logp"][rows, every["actions"][1]]).max())
    err_value = max(np.abs(got["values"][1] - want["values"])[active].max(), np.abs(every["values"][1] - want["values"]).max())
    print(f"{game} n={n} {weights}: log-probs {err_logp / d_logp:.2f} d (d = {d_logp:.3e}), values {err_value / d_value:.2f} d "
          f"(d = {d_value:.3e})")
    assert err_logp <= 8 * d_logp
    assert err_value <= 8 * d_value
    near = twin.near_boundary(want["cdf"], u)
    assert (active & ~near).sum() >= active.sum() - 0.01 * n
    assert np.array_equal(actions[active & ~near], want["actions"][active & ~near])
    assert np.array_equal(every["actions"][1][~near], want["actions"][~near])
    for name in ("actions", "logprobs", "values"):
        assert (got[name][1][~active] == 0).all(), name
        same_bits(every[name][1][active], got[name][1][active], f"{name} of the active rows under ALL_ROWS")
    same_bits(every["logits"][active], got["logits"][active], "logits")
    for run in (got, every):
        same_bits(run["action_tensor"][player, :, 0], run["actions"][1], "the ACTION tensor")
        assert (run["action_tensor"][1 - player] == -7).all()
        same_bits(run["obs"][1], inputs["obs"], "recorded obs")
        same_bits(run["states"][1], inputs["state"], "recorded states")
        same_bits(run["action_masks"][1], legal.astype(np.uint8), "recorded masks")
        same_bits(run["active"][1], active.astype(np.uint8), "recorded active")
        same_bits(run["dones"][1], (rows % 3 == 0).astype(np.float32), "dones = next_done")
        assert not run["next_done"].any() and (run["rewards"][1] == 0).all() and (run["rewards"][0] == 5).all()
        same_bits(run["last_active"], np.where(active, 1, 0).astype(np.int32), "last_active")
        same_bits(run["new_game"], np.where(active, 0, 1).astype(np.uint8), "new_game")
        assert not run["obs"][0].any() and not run["states"][0].any() and not run["action_masks"][0].any() and not run["active"][0].any()
    for name in RECORDED:
        same_bits(runs["again"][name], got[name], f"{name} of a second run")


@pytest.mark.parametrize("game,n", [("hanabi_very_small", 65), ("balance", 33)])
def test_value_only_writes_the_bootstrap_value_and_nothing_else(game, n, hip_lib):
    weights, player, num_steps, step = "orthogonal", 1, 2, 5
    seed = twin.case_seed(game, n, weights)
    agent = twin.make_agent(game, weights)
    policy = WidePolicy.from_module(agent, device=DEV)
    earlier, inputs = twin.case_inputs(game, n, seed), twin.case_inputs(game, n, seed + 1)
    active = inputs["active"] != 0
    assert not np.array_equal(earlier["active"], inputs["active"]) and not np.array_equal(earlier["state"], inputs["state"])
    sim = make_sim(game, n)
    write_inputs(sim, game, earlier, player)
    record = prepared_record(sim, game, num_steps, n)
    sim.action_tensor().to_torch().fill_(-7)
    agent_act(sim, player, policy, record, row=1, seed=seed, step=step)
    record.next_done[:] = torch.from_numpy((np.arange(n) % 2 == 0).astype(np.uint8)).to(DEV)
    record.next_value.fill_(9.0)
    record.next_active.fill_(9)
    torch.cuda.synchronize()
    before, action_before = every_buffer(record), cpu(sim.action_tensor())
    assert before["logits"].any() and before["next_done"].any() and (action_before[player] != -7).any()
    write_inputs(sim, game, inputs, player)
    results = {}
    for all_rows in (False, True):
        agent_act(sim, player, policy, record, row=num_steps, seed=seed, step=step, value_only=True, all_rows=all_rows)
        torch.cuda.synchronize()
        after = every_buffer(record)
        for name in EVERY_BUFFER:
            if name not in ("next_value", "next_active"):
                same_bits(after[name], before[name], f"{name} across a VALUE_ONLY act (all_rows={all_rows})")
        same_bits(cpu(sim.action_tensor()), action_before, "the ACTION tensor across a VALUE_ONLY act")
        same_bits(after["next_active"], active.astype(np.uint8), "next_active")
        results[all_rows] = after["next_value"]
        record.next_value.fill_(9.0)
        record.next_active.fill_(9)
    # the same kernels on the same list: the values row of a recorded act on these inputs
    recorded = {}
    for all_rows in (False, True):
        other = prepared_record(sim, game, num_steps, n)
        agent_act(sim, player, policy, other, row=0, seed=seed, step=step, all_rows=all_rows)
        torch.cuda.synchronize()
        recorded[all_rows] = cpu(other.values)[0]
    sim.close()
    want = twin.forward(twin.flat(agent), inputs["obs"], inputs["state"], twin.dims(game)[2])[0]
    d_value = margins_of_every_size(game, weights)[0]
    same_bits(results[False][active], recorded[False][active], "next_value of the active worlds")
    assert (results[False][~active] == 0).all() and active.any() and not active.all()
    same_bits(results[True], recorded[True], "next_value under ALL_ROWS")
    err = max(np.abs(results[False] - want)[active].max(), np.abs(results[True] - want).max())
    print(f"{game} n={n} VALUE_ONLY: values {err / d_value:.2f} d (d = {d_value:.3e})")
    assert err <= 8 * d_value


@pytest.mark.parametrize("game,n", [("hanabi_very_small", 65), ("balance", 33)])
def test_an_act_without_a_record(game, n, hip_lib):
    """get_action(record=False), a partner in evaluation: the same actions as the recorded act, into the ACTION tensor alone"""
    weights, player, step = "peaked", 0, 4
    seed = twin.case_seed(game, n, weights)
    policy = WidePolicy.from_module(twin.make_agent(game, weights), device=DEV)
    inputs = twin.case_inputs(game, n, seed)
    active = inputs["active"] != 0
    sim = make_sim(game, n)
    write_inputs(sim, game, inputs, player)
    workspace = torch.empty(int(_lib.lib().mrl_agent_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    for kwargs in ({}, {"all_rows": True}, {"greedy": True}):
        record = prepared_record(sim, game, 1, n)
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, record, row=0, seed=seed, step=step, **kwargs)
        torch.cuda.synchronize()
        recorded = cpu(record.actions)[0]
        same_bits(cpu(sim.action_tensor())[player, :, 0], recorded, "the ACTION tensor of the recorded act")
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, None, seed=seed, step=step, workspace=workspace, **kwargs)
        torch.cuda.synchronize()
        got = cpu(sim.action_tensor())
        same_bits(got[player, :, 0], recorded, f"the actions without a record {kwargs}")
        if "all_rows" not in kwargs:
            assert (got[player, :, 0][~active] == 0).all()
        assert recorded[active].any() and (got[1 - player] == -7).all()
    sim.close()


def test_draws_at_the_ends_of_the_grid(hip_lib):
    """u = 1 - 2^-24 over a mask whose last four actions are illegal: the exact cumulative sum reaches 1 at the last legal action, a
    float32 one may stay below u and count on into the illegal tail -- the head's last-legal fallback.  u = 0 over three
    illegal leading actions: the empty boundaries are passed.  near_boundary flags these rows, so the general comparison skips
    them; here the action is compared exactly."""
    game, n, weights = twin.EDGE_GAME, twin.EDGE_N, "orthogonal"
    agent = twin.make_agent(game, weights)
    params = twin.flat(agent)
    policy = WidePolicy.from_module(agent, device=DEV)
    d_logp = margins_of_every_size(game, weights)[1]
    sim = make_sim(game, n)
    record = prepared_record(sim, game, 1, n)
    fallback, worst = 0, 0.0
    for kind, seed, player, world, variant, want in twin.edge_rows():
        inputs = twin.edge_inputs(kind, seed, world, variant)
        write_inputs(sim, game, inputs, player)
        agent_act(sim, player, policy, record, row=0, seed=seed, step=0)
        torch.cuda.synchronize()
        action, logprob = int(cpu(record.actions)[0, world]), float(cpu(record.logprobs)[0, world])
        assert action == want, (kind, seed, player, world, variant, action)
        u = twin.draws(seed, 0, n, player)
        out = twin.act(params, inputs["obs"], inputs["state"], inputs["mask"], u)
        assert twin.near_boundary(out["cdf"], u)[world] and u[world] == twin.EDGE_U[kind]
        worst = max(worst, abs(logprob - out["logp"][world, want]))
        if kind == "top":  # would the device's own logits, summed in float32 without the fallback, have left the legal actions?
            raw = twin.head32(cpu(record.logits)[world:world + 1], inputs["mask"][world:world + 1], u[world:world + 1])[0]
            fallback += int(inputs["mask"][world, raw] == 0)
    sim.close()
    print(f"edge draws: log-probs {worst / d_logp:.2f} d (d = {d_logp:.3e}); the unguarded float32 count over the device's logits is "
          f"illegal in {fallback} of 48 top-draw rows")
    assert worst <= 8 * d_logp
    assert fallback >= 1  # (else nothing here went through the fallback)


@pytest.mark.parametrize("game,n", [("hanabi_very_small", 65), ("balance", 33)])
def test_a_world_with_no_legal_action(game, n, hip_lib):
    weights, player, step = "orthogonal", 1, 2
    seed = twin.case_seed(game, n, weights)
    agent = twin.make_agent(game, weights)
    policy = WidePolicy.from_module(agent, device=DEV)
    inputs = twin.case_inputs(game, n, seed)
    active = inputs["active"] != 0
    world = int(np.flatnonzero(active)[len(np.flatnonzero(active)) // 2])
    assert 0 < world < n - 1
    emptied = {**inputs, "mask": inputs["mask"].copy()}
    emptied["mask"][world] = 0
    sim = make_sim(game, n)
    runs = {}
    for name, case, kwargs in (("normal", inputs, {}), ("emptied", emptied, {}), ("greedy", emptied, {"greedy": True})):
        write_inputs(sim, game, case, player)
        record = prepared_record(sim, game, 1, n)
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, record, row=0, seed=seed, step=step, **kwargs)
        torch.cuda.synchronize()
        runs[name] = record_arrays(record)
        runs[name]["action_tensor"] = cpu(sim.action_tensor())
    sim.close()
    others = np.arange(n) != world
    for name in ("actions", "logprobs", "values"):
        same_bits(runs["emptied"][name][0][others], runs["normal"][name][0][others], f"{name} of the other worlds")
    same_bits(runs["emptied"]["logits"], runs["normal"]["logits"], "logits")
    same_bits(runs["emptied"]["action_tensor"][player, :, 0][others], runs["normal"]["action_tensor"][player, :, 0][others], "ACTION")
    assert not runs["emptied"]["action_masks"][0][world].any() and runs["normal"]["action_masks"][0][world].any()
    d_value = margins_of_every_size(game, weights)[0]
    want = twin.forward(twin.flat(agent), inputs["obs"], inputs["state"], twin.dims(game)[2])[0][world]
    for name in ("emptied", "greedy"):
        run = runs[name]
        assert run["actions"][0][world] == 0 and run["action_tensor"][player, world, 0] == 0, name
        assert np.isneginf(run["logprobs"][0][world]), name
        err = abs(float(run["values"][0][world]) - want)
        print(f"{game} n={n} no legal action ({name}): value {err / d_value:.2f} d (d = {d_value:.3e})")
        assert err <= 8 * d_value
        assert np.isfinite(run["logprobs"][0][others]).all()


@pytest.mark.parametrize("game,d,s,a", twin.NARROW_CASES)
def test_policies_narrower_than_the_rows_with_exact_integers(game, d, s, a, hip_lib):
    """D, S, A below the simulator's row widths: first layers of K = 1 (one padded product), 2, 65 (a chunk and an odd tail of
    one), 64, 5, and a mask row whose stride is not A.  Integer weights as in test_operand_maps_with_exact_integers: logits and
    values bit for bit.  A world whose legal actions all lie at A or beyond has no legal action.  In the A = 15 case two
    outputs share weights and bias: GREEDY takes the lower index of the tie, the higher where the lower is masked off."""
    n, player, seed, step = twin.NARROW_N, 1, 31, 6
    tie = twin.TIE if a == 15 else None
    layers = twin.integer_layers(d, s, a, tie=tie)
    policy = WidePolicy(d, s, a, device=DEV)
    policy.params.copy_(torch.from_numpy(twin.integer_params(layers)))
    full = twin.case_inputs(game, n, 4242)
    beyond = 5  # this world's only legal action is the simulator's last, which the policy does not have unless A is the row's width
    full["mask"][beyond] = 0
    full["mask"][beyond, -1] = 1
    inputs = twin.narrow_inputs(full, d, s, a)
    values, logits, bound = twin.integer_forward(layers, inputs["obs"], inputs["state"])
    assert bound < 2 ** 24
    legal, rows = inputs["mask"] != 0, np.arange(n)
    none = ~legal.any(axis=1)
    assert none[beyond] == (a < full["mask"].shape[1]) and not none.all()
    sim = make_sim(game, n)
    write_inputs(sim, game, full, player)
    assert sim.action_mask_tensor().to_torch().shape[2] >= full["mask"].shape[1]
    record = prepared_record(sim, game, 1, n, dims=(d, s, a))
    sim.action_tensor().to_torch().fill_(-7)
    agent_act(sim, player, policy, record, row=0, seed=seed, step=step, all_rows=True)
    torch.cuda.synchronize()
    got = record_arrays(record)
    same_bits(got["logits"][:, :a], logits.astype(np.float32), "logits")
    assert not got["logits"][:, a:].any()
    same_bits(got["values"][0], values.astype(np.float32), "values")
    same_bits(got["obs"][0], inputs["obs"], "recorded obs: the first D entries")
    same_bits(got["states"][0], inputs["state"], "recorded states: the first S entries")
    same_bits(got["action_masks"][0], legal.astype(np.uint8), "recorded masks: the first A entries")
    same_bits(cpu(sim.action_tensor())[player, :, 0], got["actions"][0], "the ACTION tensor")
    actions = got["actions"][0]
    assert (actions[none] == 0).all() and np.isneginf(got["logprobs"][0][none]).all()
    assert legal[rows, actions][~none].all() and np.isfinite(got["logprobs"][0][~none]).all()
    u = twin.draws(seed, step, n, player)
    want = twin.act(twin.integer_params(layers), inputs["obs"][~none], inputs["state"][~none], inputs["mask"][~none], u[~none])
    keep = ~twin.near_boundary(want["cdf"], u[~none])
    assert keep.sum() >= (~none).sum() - 1
    assert np.array_equal(actions[~none][keep], want["actions"][keep])
    if tie:
        lo, hi = tie
        # legal: what does not beat the tied pair; every third world loses the lower of the two, every third keeps its own mask
        mask = full["mask"].copy()
        for w in rows:
            if w % 3 != 2:
                mask[w, :a] = logits[w] <= logits[w, lo]
                mask[w, lo] = w % 3 != 0
        write_inputs(sim, game, {**full, "mask": mask}, player)
        agent_act(sim, player, policy, record, row=0, seed=seed, step=step, all_rows=True, greedy=True)
        torch.cuda.synchronize()
        greedy, legal = cpu(record.actions)[0], mask[:, :a] != 0
        first = np.where(legal, logits, -np.inf).argmax(axis=1)  # (numpy's arg-max is the first)
        some = legal.any(axis=1)
        assert np.array_equal(greedy[some], first[some]) and (greedy[~some] == 0).all()
        both, lower_off = (rows % 3 == 1) & (first == lo), (rows % 3 == 0) & (first == hi)
        assert both.sum() >= 5 and legal[both][:, hi].all() and lower_off.sum() >= 5 and not legal[lower_off][:, lo].any()
    sim.close()


@pytest.mark.parametrize("n", [33, 1025])
def test_an_act_stays_inside_its_workspace(n, hip_lib):
    """mrl_agent_workspace_bytes(N) bytes between two guards of 4096 bytes: the guards keep their fill, the results are those
    of the record's own workspace."""
    game, weights, player, step, guard = "hanabi_very_small", "orthogonal", 0, 1, 4096
    seed = twin.case_seed(game, 33, weights) + n
    policy = WidePolicy.from_module(twin.make_agent(game, weights), device=DEV)
    sim = make_sim(game, n)
    write_inputs(sim, game, twin.case_inputs(game, n, seed), player)
    size = (int(_lib.lib().mrl_agent_workspace_bytes(n)) + 15) // 16 * 16
    buffer = torch.full((guard + size + guard + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    first = guard + (-(buffer.data_ptr() + guard)) % 16
    middle = buffer[first:first + size]
    assert middle.data_ptr() % 16 == 0 and middle.numel() == size
    results = {}
    for name, workspace in (("own", None), ("guarded", middle)):
        record = prepared_record(sim, game, 1, n)
        sim.action_tensor().to_torch().fill_(-7)
        agent_act(sim, player, policy, record, row=0, seed=seed, step=step, workspace=workspace)
        agent_act(sim, player, policy, record, row=1, seed=seed, step=step, value_only=True, workspace=workspace)
        torch.cuda.synchronize()
        results[name] = every_buffer(record)
        results[name]["action_tensor"] = cpu(sim.action_tensor())
    sim.close()
    whole = buffer.cpu().numpy()
    assert (whole[first - guard:first] == 0xA5).all(), "the guard in front of the workspace was written"
    assert (whole[first + size:first + size + guard] == 0xA5).all(), "the guard behind the workspace was written"
    assert (whole[first:first + size] != 0xA5).any()
    for name in results["own"]:
        same_bits(results["guarded"][name], results["own"][name], f"{name} with a workspace of the caller's")
    assert results["own"]["next_value"].any() and results["own"]["values"].any()


def test_a_side_stream_gives_the_same_bits(hip_lib):
    """a recorded act, a credit, the bootstrap value and the advantage pass under torch.cuda.stream(side)"""
    game, n, weights, player, num_steps = "balance", 33, "orthogonal", 1, 2
    seed = twin.case_seed(game, n, weights)
    policy = WidePolicy.from_module(twin.make_agent(game, weights), device=DEV)
    inputs = twin.case_inputs(game, n, seed)
    rng = np.random.default_rng(8)
    rewards = torch.from_numpy(rng.normal(size=n).astype(np.float32)).to(DEV)
    dones = torch.from_numpy((rng.uniform(size=n) < 0.3).astype(np.int32)).to(DEV)
    sim = make_sim(game, n)
    # the closing observation is every world's: while a world is left without a bootstrap, the advantage pass computes only
    # the worlds being bootstrapped (include/mrl_envs.h), and a world that never acts would leave every advantage at 0
    closing = {**inputs, "active": np.ones(n, np.int32)}

    def run():
        write_inputs(sim, game, inputs, player)
        record = prepared_record(sim, game, num_steps, n)
        sim.action_tensor().to_torch().fill_(-7)
        for t in range(num_steps):
            agent_act(sim, player, policy, record, row=t, seed=seed, step=t)
            agent_credit(record, rewards, dones)
        write_inputs(sim, game, closing, player)
        agent_act(sim, player, policy, record, row=num_steps, seed=seed, step=num_steps, value_only=True)
        gae_active(record, 0.99, 0.95)
        return record

    on_default = run()
    torch.cuda.synchronize()
    want, want_action = every_buffer(on_default), cpu(sim.action_tensor())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = run()
    side.synchronize()
    torch.cuda.synchronize()
    got = every_buffer(on_side)
    for name in want:
        same_bits(got[name], want[name], f"{name} on a side stream")
    same_bits(cpu(sim.action_tensor()), want_action, "the ACTION tensor on a side stream")
    assert want["advantages"].any() and want["totals"][0, 0] > 0 and want["next_value"].any()
    sim.close()
