"""GPU: ``mrl_cnn_act``, ``mrl_rollout_cnn``, ``mrl_mappo_update`` and their bank forms on the kitchens and team sizes of
tests/kitchen_shape_cases.py.  The kernels take W, H, F and P at run time, but had run only where W >= H, P <= 2 and
npos = (W - 2)(H - 2) is 6, 9 or 21; the table's rows each run something first: npos 1 to 4 (waves without a position), 12 and 13
(exactly one round of positions, and a second for wave 0 alone), H = 3, W = 3, W < H, F = 31 and 36 (an odd k1 with 9 slabs of the
conv gradient, and 11 slabs with db_conv on wave 3), seat masks over three and four seats, LDS images within 1.3 KiB of the limit
and past it, an update whose region A is larger than the act's, and two standard layouts.

The exact cases compare with int64 arithmetic bit for bit; the float cases are within 8 d of the float64 twin, d = torch
float32's distance from the twin on the same inputs (tests/test_kitchen_shapes_api.py asserts the conditions and prints every d).
33 worlds throughout.  Each test prints its ratios."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_twin  # noqa: E402
import mappo_twin  # noqa: E402
import kitchen_shape_cases as cases  # noqa: E402
from bank_cases import cpu, same_bits  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnPolicyBank, CnnRecord, ExecMode, MappoBankOptimizer,  # noqa: E402
                                                         MappoOptimizer, OvercookedSimulator, ValueNorm, ValueNormBank, cnn_act,
                                                         cnn_act_bank, mappo_update, mappo_update_bank)

DEV = torch.device("cuda", 0)
RECORDED = ("actions", "logprobs", "values", "rewards", "dones", "next_done", "logits")
MARK, ACTION_MARK = -77, -7
STAT = _lib.MAPPO_STATS.index
N = cases.N


@pytest.fixture(autouse=True)
def table_shapes():
    with cases.shapes():
        yield


def make_sim(key, n=N, horizon=cases.HORIZON):
    return OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **cases.layout_params(key, horizon))


def policy_of(key, weights="trained"):
    return CnnPolicy.from_module(cases.make_module(key, weights), device=DEV)


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def record_arrays(record):
    return {name: cpu(getattr(record, name)) for name in RECORDED if getattr(record, name) is not None}


def marked_record(num_steps, n, p, logits=True):
    """a record whose every cell holds a value no act writes"""
    record = CnnRecord(num_steps, n, p, DEV, logits=logits)
    for name in RECORDED:
        t = getattr(record, name)
        if t is not None:
            t.fill_(MARK)
    return record


def put_observations(sim, obs):
    sim.observation_world_major_tensor().to_torch().copy_(cuda(obs))


def load_case(sim, case):
    """the case's observations into the simulator's own tensor: by stepping, or written"""
    if case["actions"] is None:
        put_observations(sim, case["obs"])
        return
    for acts in case["actions"]:
        sim.step_with_actions(cuda(acts).view(acts.shape[0], acts.shape[1], 1).contiguous())
    torch.cuda.synchronize()
    same_bits(cpu(sim.observation_world_major_tensor()), case["obs"], "the stepped worlds' observations (GPU against the CPU oracle)")


# ---------------------------------------------------------------- act, exact

@pytest.mark.parametrize("key", cases.KEYS)
def test_act_operand_and_index_maps_with_exact_integers(key, hip_lib):
    """Integer weights and inputs whose every partial sum is below 2^24: float32 is exact in any order, so logits and values
    equal the integer computation bit for bit -- a wrong split of the positions over the waves, patch offset, flatten order or K
    tail cannot, and the product behind an odd k1 = 189 or 279 must be exactly zero."""
    w, h, p, f = cases.shape(key)
    layers, obs = cases.integer_case(key)
    values, logits, bound = cnn_twin.integer_forward(layers, cnn_twin.rows_of(obs))
    assert bound < 2 ** 24
    n = obs.shape[0]
    policy = CnnPolicy(w, h, f, device=DEV)
    policy.params.copy_(torch.from_numpy(cnn_twin.integer_params(layers)))
    sim = make_sim(key, n)
    put_observations(sim, obs)
    record = marked_record(1, n, p)
    cnn_act(sim, policy, None, record, row=0, seed=3, step=0, greedy=True)
    torch.cuda.synchronize()
    got = record_arrays(record)
    sim.close()
    same_bits(got["logits"][0].reshape(-1, 6), logits.astype(np.float32), "logits")
    same_bits(got["values"][0].reshape(-1), values.astype(np.float32), "values")
    # head rows TIE are identical and the largest: GREEDY takes the first
    lo, hi = cnn_twin.TIE
    assert (logits[:, lo] == logits[:, hi]).all() and (logits.argmax(axis=1) == lo).all() and (logits[:, hi] == logits.max(axis=1)).all()
    assert (got["actions"][0].reshape(-1) == lo).all()


# ---------------------------------------------------------------- act, float

@functools.lru_cache(maxsize=None)
def forward_case(key, n, weights, inputs):
    """One case, run once and shared: the default act, the same again and GREEDY, each into row 1 of a marked record."""
    seed = cases.case_seed(key, n, weights, inputs)
    module = cases.make_module(key, weights)
    policy = CnnPolicy.from_module(module, device=DEV)
    case = cases.case_inputs(key, n, weights, inputs)
    p = case["obs"].shape[1]
    sim = make_sim(key, n)
    load_case(sim, case)
    runs = {}
    for name, kwargs in (("default", {}), ("again", {}), ("greedy", {"greedy": True})):
        record = marked_record(2, n, p)
        sim.action_tensor().to_torch().fill_(ACTION_MARK)
        cnn_act(sim, policy, None, record, row=1, seed=seed, step=0, **kwargs)
        torch.cuda.synchronize()
        runs[name] = record_arrays(record)
        runs[name]["action_tensor"] = cpu(sim.action_tensor())
    want_done, want_reward = cpu(sim.done_tensor()), cpu(sim.reward_tensor())
    sim.close()
    u = cnn_twin.draws(seed, 0, n, p)
    return {"module": module, "runs": runs, "u": u, "twin": cnn_twin.act(cnn_twin.flat(module), cnn_twin.rows_of(case["obs"]), u), "P": p,
            "done": want_done, "reward": want_reward}


@pytest.mark.parametrize("key,n,weights,inputs", cases.CASES)
def test_forward_pass_and_head(key, n, weights, inputs, hip_lib, oracle_lib):
    c = forward_case(key, n, weights, inputs)
    got, want, p = c["runs"]["default"], c["twin"], c["P"]
    d_value, d_logp = cases.layout_margins(key, weights)
    rows = np.arange(n * p)
    actions = got["actions"][1].reshape(-1)
    err_value = np.abs(got["values"][1].reshape(-1).astype(np.float64) - want["values"]).max()
    err_logp = np.abs(got["logprobs"][1].reshape(-1).astype(np.float64) - want["logp"][rows, actions]).max()  # teacher-forced
    err_logits = np.abs(got["logits"][1].reshape(-1, 6).astype(np.float64) - want["logits"]).max()
    print(f"{key} n={n} {weights} {inputs}: values {err_value / d_value:.2f} d (d = {d_value:.3e}), log-probs {err_logp / d_logp:.2f} d "
          f"(d = {d_logp:.3e}), logits off by {err_logits:.3e}")
    assert err_value <= mappo_twin.FACTOR * d_value
    assert err_logp <= mappo_twin.FACTOR * d_logp
    assert ((actions >= 0) & (actions < 6)).all()
    keep = ~cnn_twin.near_boundary(want["cdf"], c["u"])
    assert keep.sum() >= len(rows) - 0.01 * len(rows)
    assert np.array_equal(actions[keep], want["actions"][keep])
    # the ACTION tensor (P, N, 1) holds the record's actions (N, P)
    same_bits(got["action_tensor"][:, :, 0].T, got["actions"][1], "the ACTION tensor")
    # bookkeeping of a row k > 0: dones = DONE as it stands, rewards[k - 1] = REWARD cast; nothing else of the record moves
    same_bits(got["dones"][1], np.repeat((c["done"] != 0).astype(np.float32)[:, None], p, axis=1), "dones")
    same_bits(got["rewards"][0], c["reward"].T.astype(np.float32), "rewards of the row before")
    for name in ("actions", "logprobs", "values", "dones", "logits"):
        assert (got[name][0] == MARK).all(), name
    assert (got["rewards"][1] == MARK).all() and (got["values"][2] == MARK).all() and (got["next_done"] == MARK).all()
    # the same bits on every run
    for name in got:
        same_bits(c["runs"]["again"][name], got[name], f"second run: {name}")
    # GREEDY: the first arg-max of the logits it recorded, which are the default run's
    greedy = c["runs"]["greedy"]
    same_bits(greedy["logits"], got["logits"], "logits under GREEDY")
    assert np.array_equal(greedy["actions"][1].reshape(-1), greedy["logits"][1].reshape(-1, 6).argmax(axis=1))
    same_bits(greedy["values"], got["values"], "values under GREEDY")


# ---------------------------------------------------------------- seat masks at P = 3 and P = 4

@functools.lru_cache(maxsize=None)
def masked_runs(key):
    """{mask or None: the arrays of one act into row 1 of a marked record over a marked ACTION tensor}; REWARD holds a value per
    (seat, world), so that a reward read at another seat's row shows"""
    masks = {"k4x4p3": (0b101, 0b110, 0b010), "k6x5p4": (0b1010, 0b0111, 0b1001)}[key]
    p = cases.shape(key)[2]
    policy = policy_of(key)
    sim = make_sim(key)
    put_observations(sim, cases.case_inputs(key, N, "trained", "synthetic")["obs"])
    reward = sim.reward_tensor().to_torch()
    reward.copy_((1000 * torch.arange(p, device=DEV).view(p, 1) + torch.arange(N, device=DEV).view(1, N)).view(reward.shape).to(reward.dtype))
    out = {}
    for mask in (None,) + masks:
        record = marked_record(2, N, p)
        sim.action_tensor().to_torch().fill_(ACTION_MARK)
        cnn_act(sim, policy, mask, record, row=1, seed=9, step=4)
        torch.cuda.synchronize()
        out[mask] = record_arrays(record)
        out[mask]["action_tensor"] = cpu(sim.action_tensor())
    sim.close()
    return out


@pytest.mark.parametrize("key,mask", [("k4x4p3", 0b101), ("k4x4p3", 0b110), ("k4x4p3", 0b010),
                                      ("k6x5p4", 0b1010), ("k6x5p4", 0b0111), ("k6x5p4", 0b1001)], ids=lambda v: v if isinstance(v, str) else bin(v))
def test_seat_mask_over_three_and_four_seats(key, mask, hip_lib):
    """The seats of a mask with a gap act exactly as under the full mask -- the draw is hashed from the real seat number, the
    record's cell is (world, seat) of N x P, REWARD is read at seat * N + world -- and every cell of the other seats keeps its
    marker, in the record and in ACTION."""
    p = cases.shape(key)[2]
    runs = masked_runs(key)
    full, alone = runs[None], runs[mask]
    assert (full["actions"][1] >= 0).all() and (full["action_tensor"] != ACTION_MARK).all()
    # the full mask's rewards are REWARD's own rows, seat by seat
    want_reward = (1000 * np.arange(p)[None, :] + np.arange(N)[:, None]).astype(np.float32)
    same_bits(full["rewards"][0], want_reward, "rewards under the full mask")
    for seat in range(p):
        acting = bool((mask >> seat) & 1)
        for name in ("actions", "logprobs", "values", "rewards", "dones", "logits"):
            if acting:
                same_bits(alone[name][:, :, seat], full[name][:, :, seat], f"{key} mask {mask:#b}, seat {seat}: {name}")
            else:
                assert (alone[name][:, :, seat] == MARK).all(), (name, seat)
        if acting:
            same_bits(alone["action_tensor"][seat], full["action_tensor"][seat], f"{key} mask {mask:#b}, seat {seat}: ACTION")
        else:
            assert (alone["action_tensor"][seat] == ACTION_MARK).all(), seat
    same_bits(alone["next_done"], full["next_done"], "next_done (no act writes it)")
    assert (alone["next_done"] == MARK).all()


# ---------------------------------------------------------------- closed loop with three seats

ROLLOUT = ("k4x4p3", N, 12, 5)  # key, worlds, T, horizon: worlds restart inside the rollout, twice


@functools.lru_cache(maxsize=None)
def rollout_case():
    key, n, t, horizon = ROLLOUT
    w, h, p, f = cases.shape(key)
    policy = policy_of(key)
    sim = make_sim(key, n, horizon)
    record = marked_record(t, n, p, logits=False)
    ring = torch.zeros((t + 1, n, p, h, w, f), dtype=torch.int8, device=DEV)
    sim.rollout_cnn(policy, record, ring, seed=21, first_step=100)
    torch.cuda.synchronize()
    out = record_arrays(record)
    out["ring"] = cpu(ring)
    out["final"] = {"obs_own": cpu(sim.observation_world_major_tensor()), "players": cpu(sim.state_players_tensor()),
                    "objects": cpu(sim.state_objects_tensor()), "timestep": cpu(sim.state_timestep_tensor())}
    sim.close()
    return out


def test_rollout_with_three_seats_equals_hand_issued_acts_and_steps(hip_lib, oracle_lib):
    key, n, t, horizon = ROLLOUT
    w, h, p, f = cases.shape(key)
    got = rollout_case()
    policy = policy_of(key)
    sim = make_sim(key, n, horizon)
    record = marked_record(t, n, p, logits=False)
    ring = torch.zeros((t + 1, n, p, h, w, f), dtype=torch.int8, device=DEV)
    ring[0].copy_(sim.observation_world_major_tensor().to_torch())
    for k in range(t):
        cnn_act(sim, policy, None, record, row=k, seed=21, step=100 + k)
        sim.set_observation_output(ring[k + 1])
        sim.step()
    cnn_act(sim, policy, None, record, row=t, value_only=True)
    sim.set_observation_output(None)
    torch.cuda.synchronize()
    by_hand = record_arrays(record)
    for name, value in by_hand.items():
        assert not (value == MARK).any(), name  # every cell of every row was written, all three seats' columns
        same_bits(got[name], value, f"rollout against hand-issued calls: {name}")
    same_bits(got["ring"], cpu(ring), "the observation ring")
    same_bits(got["final"]["players"], cpu(sim.state_players_tensor()), "players' state")
    same_bits(got["final"]["objects"], cpu(sim.state_objects_tensor()), "objects' state")
    same_bits(got["final"]["timestep"], cpu(sim.state_timestep_tensor()), "timestep")
    sim.close()

    # the CPU oracle stepped with the recorded actions: every slot, and the reward and done rows in all three seats' columns
    orc = oracle_lib.OvercookedOracle(cases.layout_params(key, horizon), n)
    same_bits(got["ring"][0].view(np.uint8).reshape(orc.obs.shape), orc.obs, "slot 0")
    finished = 0
    for k in range(t):
        same_bits(got["dones"][k], np.repeat((orc.done != 0).astype(np.float32)[:, None], p, axis=1), f"dones[{k}]")
        assert ((got["actions"][k] >= 0) & (got["actions"][k] < 6)).all()
        orc.step(np.ascontiguousarray(got["actions"][k].T))
        same_bits(got["ring"][k + 1].view(np.uint8).reshape(orc.obs.shape), orc.obs, f"slot {k + 1}")
        assert orc.reward.shape == (p, n)
        same_bits(got["rewards"][k], orc.reward.T.astype(np.float32), f"rewards[{k}]")
        finished += int((orc.done != 0).sum())
    same_bits(got["next_done"], np.repeat((orc.done != 0).astype(np.float32)[:, None], p, axis=1), "next_done")
    assert finished == 2 * n  # every world restarted twice inside the rollout
    same_bits(got["final"]["obs_own"], got["ring"][t], "the simulator's own tensor after the rollout")
    assert not np.array_equal(got["ring"][0], got["ring"][t])
    orc.close()

    # the values and the actions are the twin's on the ring's own slots
    module = cases.make_module(key, "trained")
    d_value = cases.layout_margins(key, "trained")[0]
    for k in range(t + 1):
        u = cnn_twin.draws(21, 100 + k, n, p)
        want = cnn_twin.act(cnn_twin.flat(module), cnn_twin.rows_of(got["ring"][k]), u)
        assert np.abs(got["values"][k].reshape(-1) - want["values"]).max() <= mappo_twin.FACTOR * d_value, k
        if k < t:
            keep = ~cnn_twin.near_boundary(want["cdf"], u)
            assert np.array_equal(got["actions"][k].reshape(-1)[keep], want["actions"][keep]), k


# ---------------------------------------------------------------- the update

class Device:
    """A policy, its optimizer, a ValueNorm and a batch (as a record and a ring) on the GPU."""

    def __init__(self, key, worlds, params, batch, cfg):
        w, h, p, f = cases.shape(key)
        self.cfg = cfg
        self.policy = CnnPolicy(w, h, f, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(params, np.float32)))
        self.optimizer = MappoOptimizer(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        steps = len(batch.ring) // (worlds * p)
        assert steps * worlds * p == len(batch.ring)
        self.record = CnnRecord(steps, worlds, p, DEV)
        self.record.actions.copy_(cuda(batch.actions).view(steps, worlds, p))
        self.record.logprobs.copy_(cuda(batch.logprobs).view(steps, worlds, p))
        self.record.values[:steps].copy_(cuda(batch.values).view(steps, worlds, p))
        self.ring = torch.zeros((steps + 1, worlds, p, h, w, f), dtype=torch.int8, device=DEV)
        self.ring[:steps].copy_(cuda(batch.ring).view(steps, worlds, p, h, w, f))
        self.advantages = cuda(batch.advantages).view(steps, worlds, p)
        self.returns = cuda(batch.returns).view(steps, worlds, p)
        self.value_norm = ValueNorm(DEV, beta=0.99999, epsilon=1e-5)
        self.value_norm.state.copy_(cuda(np.asarray(mappo_twin.STATE0, np.float32)))

    def update(self, indices):
        c = self.cfg
        result = mappo_update(self.policy, self.optimizer, self.record, self.ring, self.advantages, self.returns, cuda(indices),
                              value_norm=self.value_norm if c.valuenorm else None, clip_param=c.clip_param, entropy_coef=c.entropy_coef,
                              value_loss_coef=c.value_loss_coef, max_grad_norm=c.max_grad_norm, huber_delta=c.huber_delta,
                              use_huber_loss=c.huber, use_clipped_value_loss=c.clipped_value, use_max_grad_norm=c.clip_grads,
                              stats=True, grads=True)
        return cpu(result.stats), cpu(result.grads)

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


@pytest.mark.parametrize("key", cases.KEYS)
def test_update_operand_maps_with_exact_integers(key, hip_lib):
    """critic only, every number an integer below 2^24, B = 64: dW_conv (its ragged last slab, 23 or 4 wide at F = 31 and 36),
    dW_fc1 (the positions split over the waves), dW_fc2, dW_head and the biases (db_conv on wave 3 at 11 slabs) bit for bit
    against numpy's integer arithmetic -- the whole gradient, and the three matrices by name"""
    case = cases.update_integer_case(key)
    assert case["bound"] < 2 ** 24
    w, h, p, f = cases.shape(key)
    npos = (w - 2) * (h - 2)
    device = Device(key, mappo_twin.N, case["params"], case["batch"], case["cfg"])
    _, grads = device.update(case["indices"])
    critic = grads[0][mappo_twin.actor_size(key):]
    sizes = [32 * 9 * f, 32, 64 * 32 * npos, 64, 64 * 64, 64, 64, 1]
    assert sum(sizes) == critic.size == case["grad"].size
    at = np.concatenate([[0], np.cumsum(sizes)])
    pieces = dict(zip(("conv", "conv bias", "fc1", "fc1 bias", "fc2", "fc2 bias", "head", "head bias"), zip(at[:-1], at[1:])))
    for name in ("conv", "fc1", "fc2"):
        lo, hi = pieces[name]
        same_bits(critic[lo:hi], case["matrices"][name].reshape(-1).astype(np.float32), f"{key}: the critic's dW of {name}")
    for name, (lo, hi) in pieces.items():
        same_bits(critic[lo:hi], case["grad"][lo:hi].astype(np.float32), f"{key}: the critic's gradient of {name}")
    same_bits(critic, case["grad"].astype(np.float32), "the critic's gradient")


@pytest.mark.parametrize("case", cases.MAPPO_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_update_gradient_and_stats_match_the_twin(hip_lib, case):
    """one row at B = 33: both nets' gradient within 8 d of the float64 twin, d = float32 torch's distance on the same row; every
    scalar stat within 8 x its d pooled over the keys here; clipfrac the twin's count / B"""
    fixed = cases.fixed_case(case)
    exact, single, width = fixed["twin"], fixed["f32"], case[4]
    device = Device(fixed["layout"], fixed["worlds"], fixed["params"], fixed["batch"], fixed["cfg"])
    before = device.state()
    stats, grads = device.update(fixed["indices"])
    d, stat_d = mappo_twin.row_margins(exact, single), cases.stat_margins(case[2])
    na = mappo_twin.actor_size(case[0])
    ratios = {"grad": mappo_twin.distance(grads[0], exact["grad"]) / d["grad"],
              "actor grad": mappo_twin.distance(grads[0][:na], exact["grad"][:na]) / d["grad"],
              "critic grad": mappo_twin.distance(grads[0][na:], exact["grad"][na:]) / d["grad"]}
    for name in mappo_twin.STATS:
        if name != "clipfrac":
            ratios[name] = abs(float(stats[0][STAT(name)]) - exact["stats"][name]) / stat_d[name]
    print(str(case), "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d["grad"])
    count = round(exact["stats"]["clipfrac"] * width)
    assert stats[0][STAT("clipfrac")] == np.float32(np.float64(count) / np.float64(width))
    assert stats[0][STAT("reserved")] == 0
    for name, ratio in ratios.items():
        assert ratio <= mappo_twin.FACTOR, (case, name, ratio)
    after = device.state()
    state32 = single["state"]
    d_state = np.maximum(np.abs(state32 - exact["state"]), np.abs(exact["state"]) * 2.0 ** -24)
    assert (np.abs(after["value_norm"] - exact["state"]) <= mappo_twin.FACTOR * d_state).all()
    assert device.optimizer.step == 1 and not np.array_equal(after["params"], before["params"])


@pytest.mark.parametrize("key", ["k3x3p1", "k8x5p4"])
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, key):
    """the update's forward pass is the act's: on k3x3p1 it runs on another LDS image than the act's (region A grew, act_at moved
    up), on k8x5p4 on the largest one.  On unchanged parameters the ratio is exactly 1, and with the record's own values as
    returns (plain squared error) the value loss is exactly 0."""
    t = 2
    w, h, p, f = cases.shape(key)
    assert (key in cases.REGION_A_GROWS) == (key == "k3x3p1")
    policy = policy_of(key)
    sim = make_sim(key)
    rng = np.random.default_rng(6)
    for _ in range(6):  # the worlds go different ways first (a 3 x 3 kitchen has few states: its one player turns, picks up and puts down)
        sim.step_with_actions(cuda(rng.integers(0, 6, size=(p, N, 1)).astype(np.int32)))
    record = CnnRecord(t, N, p, DEV)
    ring = torch.zeros((t + 1, N, p, h, w, f), dtype=torch.int8, device=DEV)
    sim.rollout_cnn(policy, record, ring, seed=5, first_step=0)
    count = t * N * p
    returns = record.values[:t].clone()
    indices = torch.arange(count, dtype=torch.int32, device=DEV).view(1, count)
    result = mappo_update(policy, MappoOptimizer(policy), record, ring, torch.ones_like(returns), returns, indices, value_norm=None,
                          use_huber_loss=False, use_clipped_value_loss=False)
    stats = cpu(result.stats)[0]
    assert all(len(np.unique(row)) > 1 for row in cpu(record.values))  # no row compares one constant with itself
    assert stats[STAT("ratio")] == 1.0 and stats[STAT("clipfrac")] == 0.0
    assert stats[STAT("value_loss")] == 0.0 and stats[STAT("critic_grad_norm")] == 0.0
    assert stats[STAT("policy_loss")] == -1.0
    sim.close()


# ---------------------------------------------------------------- banks, one shape each

def test_bank_act_with_three_policies_over_three_seats(hip_lib):
    """k4x4p3: every (world, seat) cell names one of three policies; each cell holds the bits of the plain act of that policy"""
    key, k = "k4x4p3", 3
    w, h, p, f = cases.shape(key)
    policies = [CnnPolicy.from_module(cnn_twin.make_module(key, "trained", seed=101 + i), device=DEV) for i in range(k)]
    bank = CnnPolicyBank.from_policies(policies)
    sim = make_sim(key)
    put_observations(sim, cases.case_inputs(key, N, "trained", "synthetic")["obs"])
    rng = np.random.default_rng(12)
    ids = rng.integers(0, k, size=(N, p)).astype(np.int32)
    assert all(len({ids[n, s] for n in range(N)}) == k for s in range(p)) and any(len(set(row)) == k for row in ids)

    def one_act(act):
        record = marked_record(2, N, p)
        sim.action_tensor().to_torch().fill_(ACTION_MARK)
        act(record)
        torch.cuda.synchronize()
        out = record_arrays(record)
        out["action_tensor"] = cpu(sim.action_tensor())
        return out

    ids_row = torch.full((N, p), 9, dtype=torch.int32, device=DEV)
    got = one_act(lambda r: cnn_act_bank(sim, bank, cuda(ids), None, r, ids_row, row=1, seed=17, step=3))
    same_bits(cpu(ids_row), ids, "ids_row")
    plain = [one_act(lambda r, j=j: cnn_act(sim, bank.policy(j), None, r, row=1, seed=17, step=3)) for j in range(k)]
    assert not np.array_equal(plain[0]["values"], plain[1]["values"]) and not np.array_equal(plain[1]["logits"], plain[2]["logits"])
    for j in range(k):
        mine = ids == j
        for name in ("actions", "logprobs", "values", "rewards", "dones", "logits"):
            same_bits(got[name][:, mine], plain[j][name][:, mine], f"policy {j}'s cells: {name}")
        same_bits(got["action_tensor"][:, :, 0].T[mine], plain[j]["action_tensor"][:, :, 0].T[mine], f"policy {j}'s cells: ACTION")
    assert (got["actions"][1] >= 0).all() and (got["next_done"] == MARK).all()
    sim.close()


def test_bank_update_of_two_members_equals_two_plain_updates(hip_lib):
    """k6x5p4: ``mrl_mappo_bank_update`` of both members of a bank of two, two rows of B = 33 each, against the plain update of
    each member -- parameters, moments, ValueNorm rows, stats and gradients bit for bit"""
    key, members, rows = "k6x5p4", 2, 2
    w, h, p, f = cases.shape(key)
    fixed = cases.fixed_case((key, N, "trained", "synthetic", cases.B, "default"))
    batch, size = fixed["batch"], len(fixed["batch"].ring)
    params = torch.stack([cuda(fixed["params"]), cuda(cnn_twin.flat(cnn_twin.make_module(key, "trained", seed=57)).astype(np.float32))])
    indices = cuda(np.stack([mappo_twin.make_indices(rows, cases.B, size, 400 + z) for z in range(members)]).astype(np.int32))
    assert indices.shape == (members, rows, cases.B)
    base = Device(key, N, fixed["params"], batch, fixed["cfg"])  # the record, ring, advantages and returns both runs share
    state0 = cuda(np.asarray(mappo_twin.STATE0, np.float32))

    def bank_of():
        bank = CnnPolicyBank(w, h, f, members, device=DEV)
        bank.params.copy_(params)
        return bank

    options = dict(huber_delta=1.0, max_grad_norm=1.0)
    bank = bank_of()
    optimizer, norms = MappoBankOptimizer(bank), ValueNormBank(members, DEV)
    norms.state.copy_(state0.expand(members, 3))
    result = mappo_update_bank(bank, optimizer, base.record, base.ring, base.advantages, base.returns, indices, norms, stats=True, grads=True,
                               **options)
    torch.cuda.synchronize()
    assert optimizer.step == rows
    got_stats, got_grads = cpu(result.stats), cpu(result.grads)
    other = bank_of()
    for z in range(members):
        policy = other.policy(z)
        plain, value_norm = MappoOptimizer(policy), ValueNorm(DEV)
        value_norm.state.copy_(state0)
        want = mappo_update(policy, plain, base.record, base.ring, base.advantages, base.returns, indices[z].contiguous(), value_norm=value_norm,
                            stats=True, grads=True, **options)
        torch.cuda.synchronize()
        same_bits(got_stats[z], cpu(want.stats), f"member {z}: stats")
        same_bits(got_grads[z], cpu(want.grads), f"member {z}: gradients")
        same_bits(cpu(bank.params[z]), cpu(policy.params), f"member {z}: parameters")
        same_bits(cpu(optimizer.exp_avg[z]), cpu(plain.exp_avg), f"member {z}: exp_avg")
        same_bits(cpu(optimizer.exp_avg_sq[z]), cpu(plain.exp_avg_sq), f"member {z}: exp_avg_sq")
        same_bits(cpu(norms.state[z]), cpu(value_norm.state), f"member {z}: ValueNorm state")
        assert not np.array_equal(cpu(bank.params[z]), cpu(params[z])) and np.isfinite(got_stats[z]).all()
    assert not np.array_equal(got_grads[0], got_grads[1])


# ---------------------------------------------------------------- refusals on a live device

@pytest.mark.parametrize("key", cases.REFUSED_KEYS)
def test_shapes_past_the_lds_limit_are_refused_and_nothing_is_enqueued(hip_lib, key):
    """``mrl_cnn_act``, ``mrl_rollout_cnn`` and ``mrl_mappo_update`` return MRL_ERR_INVALID with the library's message, byte for
    byte, the act's byte count the table's literal; the record, ACTION, the ring, the parameters and the moments keep every bit"""
    L = _lib.lib()
    w, h, p, act_bytes, update_bytes = cases.REFUSED[key]
    f = 5 * p + 16
    t = 2
    assert act_bytes > cases.LDS_LIMIT and update_bytes > cases.LDS_LIMIT
    sim = make_sim(key)
    assert tuple(sim.observation_world_major_tensor().shape) == (N, p, h, w, f)
    policy = CnnPolicy(w, h, f, device=DEV)
    policy.params.normal_(generator=torch.Generator(device=DEV).manual_seed(2))
    params_before = cpu(policy.params)
    record = marked_record(t, N, p)
    sim.action_tensor().to_torch().fill_(ACTION_MARK)
    ws = torch.empty(int(L.mrl_cnn_workspace_bytes(N, p)), dtype=torch.uint8, device=DEV)
    ring = torch.zeros((t + 1, N, p, h, w, f), dtype=torch.int8, device=DEV)
    desc, rec, every_seat = policy.desc(), record.struct, (1 << p) - 1
    needs = f"a {w} x {h} kitchen with {f} channels needs an LDS image of {act_bytes} bytes per workgroup, the limit is {cases.LDS_LIMIT}"

    rc = L.mrl_cnn_act(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), 0, 1, 0, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_cnn_act: {needs}"
    rc = L.mrl_rollout_cnn(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), ring.data_ptr(), 1, 0, None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_rollout_cnn: {needs}"
    # the Python layer hands the same message on
    with pytest.raises(_lib.MrlError) as refused:
        cnn_act(sim, policy, None, record, row=0)
    assert str(refused.value) == f"mrl_cnn_act: {needs}"
    with pytest.raises(_lib.MrlError) as refused:
        sim.rollout_cnn(policy, record, ring)
    assert str(refused.value) == f"mrl_rollout_cnn: {needs}"

    # the update: every array is there, so that the shape is what refuses it
    count, width = t * N * p, cases.B
    exp_avg, exp_avg_sq = torch.full_like(policy.params, 0.25), torch.full_like(policy.params, 0.5)
    advantages, returns = torch.ones((t, N, p), device=DEV), torch.ones((t, N, p), device=DEV)
    indices = torch.arange(width, dtype=torch.int32, device=DEV).view(1, width)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    stats = torch.full((1, len(_lib.MAPPO_STATS)), float(MARK), device=DEV)
    shape = _lib.MappoPolicyDesc(policy.params.data_ptr(), 64, 0, w, h, f)
    opt = _lib.MappoOptimizerDesc(policy.params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), 0)
    batch = _lib.MappoBatch(ring.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(),
                            returns.data_ptr(), advantages.data_ptr(), count)
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1.0 - 0.99999, 1e-5, 0)
    rc = L.mrl_mappo_update(ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), 1, width, ctypes.byref(cfg), None,
                            scratch.data_ptr(), scratch.numel(), stats.data_ptr(), None, 0, None)
    assert rc == _lib.MRL_ERR_INVALID
    assert L.mrl_last_error().decode() == ("mrl_mappo_update: the kitchen's LDS image does not fit one workgroup's 160 KiB "
                                           f"(width {w}, height {h}, channels {f}, hidden 64, minibatch_size {width}, batch size {count})")
    with pytest.raises(_lib.MrlError, match="LDS image does not fit"):
        MappoOptimizer(policy).workspace_bytes(width, 1)

    torch.cuda.synchronize()
    for name, value in record_arrays(record).items():
        assert (value == MARK).all(), name
    assert (cpu(sim.action_tensor()) == ACTION_MARK).all() and not cpu(ring).any() and not cpu(scratch).any()
    same_bits(cpu(policy.params), params_before, "the parameters")
    assert (cpu(exp_avg) == 0.25).all() and (cpu(exp_avg_sq) == 0.5).all() and (cpu(stats) == MARK).all()
    # and the simulator still steps
    sim.step()
    torch.cuda.synchronize()
    sim.close()
