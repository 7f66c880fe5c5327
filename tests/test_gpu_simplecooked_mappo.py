"""GPU: ``mappo_update`` (mrl_mappo_update) on Simplecooked rings against the float64 twin of tests/mappo_twin.py, the closed loop
``env.rollout`` -> ``mappo_advantages`` -> ``mappo_update`` on ``overcooked2_env.OvercookedMadrona``, and the training tool with
``game="simplecooked"``.  The gradient kernel has run only F = 26 (K = 234, even) before: here F = 20 and, with one player,
F = 15 -- K = 135, the padded product of the forward pass and a ragged last slab of dW_conv -- on rows of 375 bytes.

Cases, seeds and inputs: tests/simplecooked_cnn_cases.py; their conditions are asserted by tests/test_simplecooked_cnn_api.py.
Margins: d is, per kind of number, the largest distance of the float32 CPU computation of the same losses from the twin on the
same inputs; the device must be within 8 x d.  For the vector kinds (gradient, parameters, moments) that is the largest over the
elements of the case at hand; a scalar stat's d is pooled over the cases here of its weight set.  Each test prints its ratios."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_twin  # noqa: E402
import mappo_twin as twin  # noqa: E402
import simplecooked_cnn_cases as cases  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs.overcooked2_env import OvercookedMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnRecord, MappoOptimizer, ValueNorm, mappo_advantages,  # noqa: E402
                                                         mappo_update, minibatch_indices)

DEV = torch.device("cuda", 0)
STAT = _lib.MAPPO_STATS.index


@pytest.fixture(autouse=True)
def simplecooked_shapes():
    with cases.shapes():
        yield


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def make_env(key, n, horizon):
    name, players = cases.parse(key)
    return OvercookedMadrona(name, n, 0, horizon=horizon, num_players=players)


class Device:
    """A policy, its optimizer, a ValueNorm and a batch (as a record and a ring) on the GPU."""

    def __init__(self, fixed, step=0, moments=None, cfg=None):
        key, worlds, batch = fixed["layout"], fixed["worlds"], fixed["batch"]
        self.cfg = cfg = cfg or fixed["cfg"]
        w, h, p, f = cases.shape(key)
        self.policy = CnnPolicy(w, h, f, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(fixed["params"], np.float32)))
        self.optimizer = MappoOptimizer(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.optimizer.step = step
        if moments is not None:
            self.optimizer.exp_avg.copy_(cuda(moments[0]))
            self.optimizer.exp_avg_sq.copy_(cuda(moments[1]))
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
        self.value_norm.state.copy_(cuda(np.asarray(twin.STATE0, np.float32)))

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


def check_row(what, got_stats, got_grad, fixed, stat_d):
    """One row of the device against the twin's: the gradient within 8 d of the case, every stat within 8 x its pooled d, clipfrac
    the twin's count / B."""
    exact, single, width = fixed["twin"], fixed["f32"], fixed["indices"].shape[1]
    d = twin.row_margins(exact, single)
    ratios = {"grad": twin.distance(got_grad, exact["grad"]) / d["grad"]}
    for name in twin.STATS:
        if name != "clipfrac":
            off = abs(float(got_stats[STAT(name)]) - exact["stats"][name])
            ratios[name] = off / stat_d[name] if stat_d[name] > 0 else (0.0 if off == 0 else float("inf"))
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d["grad"])
    count = round(exact["stats"]["clipfrac"] * width)
    assert got_stats[STAT("clipfrac")] == np.float32(np.float64(count) / np.float64(width)), what
    assert got_stats[STAT("reserved")] == 0
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)


@pytest.mark.parametrize("case", cases.MAPPO_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_stats_and_step_match_the_twin(hip_lib, oracle_lib, case):
    fixed = cases.fixed_case(case)
    cfg, key, params = fixed["cfg"], fixed["layout"], fixed["params"]
    device = Device(fixed)
    before = device.state()
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(case[2]))
    after = device.state()
    if cfg.valuenorm:
        state32 = fixed["f32"]["state"]
        d = np.maximum(np.abs(state32 - fixed["twin"]["state"]), np.abs(fixed["twin"]["state"]) * 2.0 ** -24)
        assert (np.abs(after["value_norm"] - fixed["twin"]["state"]) <= twin.FACTOR * d).all()
    else:
        same_bits(after["value_norm"], before["value_norm"], "the ValueNorm state without MRL_MAPPO_VALUENORM")
    assert device.optimizer.step == 1
    # the stepped parameters and moments, teacher-forced on the device's own gradient: both nets' clip and Adam from zero moments
    grad, zeros, na = grads[0].astype(np.float64), np.zeros(params.size), twin.actor_size(key)
    ratios = {}
    for net, (sl, lr) in enumerate(((slice(0, na), cfg.lr), (slice(na, None), cfg.critic_lr))):
        _, p32, m32, v32 = twin.clip_adam_torch(params[sl], zeros[sl], zeros[sl], grad[sl], 0, cfg.max_grad_norm, lr, cfg, torch.float32)
        _, p, m, v = twin.clip_adam(params[sl], zeros[sl], zeros[sl], grad[sl], 0, cfg.max_grad_norm, lr, cfg)
        for name, have, want, single in (("params", after["params"][sl], p, p32), ("exp_avg", after["exp_avg"][sl], m, m32),
                                         ("exp_avg_sq", after["exp_avg_sq"][sl], v, v32)):
            off, d = twin.distance(have, want), max(twin.distance(single, want), float(np.abs(want).max()) * 2.0 ** -24)
            # (d = 0: a net whose gradient is zero throughout -- B = 1 on huber_loss's dead branch -- leaves zero moments)
            ratios[f"{name}[{net}]"] = off / d if d > 0 else (0.0 if off == 0 else float("inf"))
    print(str(case), "the step, measured / d:", {k: round(r, 2) for k, r in ratios.items()})
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (case, name, ratio)
    assert not np.array_equal(after["params"], before["params"])
    # two runs give the same bits
    again = Device(fixed)
    stats2, grads2 = again.update(fixed["indices"])
    same_bits(stats2, stats, "stats of a second run")
    same_bits(grads2, grads, "gradients of a second run")
    for name, value in after.items():
        same_bits(again.state()[name], value, f"{name} of a second run")


@pytest.mark.parametrize("key, n", [("simple", 33), ("unident_s", 33), ("random1", 3), ("random1/1p", 3), ("random1/1p", 33), ("simple/1p", 65)])
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, key, n):
    """the update's forward pass is the act's at every new shape, rows at every byte offset included: on unchanged parameters the
    ratio is exactly 1, and with the record's own values as returns (plain squared error) the value loss is exactly 0"""
    t = 2
    p = cases.shape(key)[2]
    policy = CnnPolicy.from_module(cases.make_module(key, "trained"), device=DEV)
    env = make_env(key, n, cases.HORIZON)
    record, ring = env.rollout(policy, t, seed=5, first_step=0)
    count = t * n * p
    returns = record.values[:t].clone()
    indices = torch.arange(count, dtype=torch.int32, device=DEV).view(1, count)
    result = mappo_update(policy, MappoOptimizer(policy), record, ring, torch.ones_like(returns), returns, indices, value_norm=None,
                          use_huber_loss=False, use_clipped_value_loss=False)
    stats = cpu(result.stats)[0]
    assert stats[STAT("ratio")] == 1.0 and stats[STAT("clipfrac")] == 0.0
    assert stats[STAT("value_loss")] == 0.0 and stats[STAT("critic_grad_norm")] == 0.0
    assert stats[STAT("policy_loss")] == -1.0
    env.close()


def test_closed_loop_rollout_update_act(hip_lib):
    """env.rollout -> mappo_advantages -> mappo_update -> env.act on the Simplecooked env: before any update the recomputed
    log-probs are the record's bit for bit (ratio exactly 1, clipfrac 0 on row 0), the gradient on the real ring is the twin's,
    and the act that follows reads the updated tensor in place"""
    key, n, t = "simple", 33, 4
    module = cases.make_module(key, "trained")
    policy = CnnPolicy.from_module(module, device=DEV)
    start = cpu(policy.params)
    env = make_env(key, n, cases.HORIZON)
    record, ring = env.rollout(policy, t, seed=31, first_step=0)
    value_norm = ValueNorm(DEV)
    advantages, returns = mappo_advantages(record, value_norm)
    assert advantages.shape == returns.shape == (t, n, 2)
    count = t * n * 2
    indices = minibatch_indices(count, 1, 2, generator=torch.Generator().manual_seed(3), device=DEV)
    optimizer = MappoOptimizer(policy)
    result = mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm, grads=True)
    stats = cpu(result.stats)
    assert stats[0][STAT("ratio")] == 1.0 and stats[0][STAT("clipfrac")] == 0.0
    assert stats[1][STAT("ratio")] != 1.0
    assert optimizer.step == 2
    grads = cpu(result.grads)
    cfg = twin.Config(huber_delta=10.0)
    batch = twin.Batch(cpu(ring)[:t].reshape(count, *cpu(ring).shape[3:]), cpu(record.actions).reshape(-1), cpu(record.logprobs).reshape(-1),
                       cpu(record.values)[:t].reshape(-1), cpu(returns).reshape(-1), cpu(advantages).reshape(-1))
    params, m, v, state = start.astype(np.float64), np.zeros(start.size), np.zeros(start.size), np.zeros(3)
    for k, inds in enumerate(cpu(indices)):
        out = twin.row(params, key, batch, inds, cfg, state)
        if k == 0:
            # the conditions of the inputs hold for this rollout seed (asserted: properties of the twin, not of the device's answer)
            single = twin.row(params, key, batch, inds, cfg, state, torch.float32)
            closest, worst = twin.relu_margin({"twin": out, "f32": single})
            assert out["kink"] > twin.KINK and closest > twin.FACTOR * worst, (out["kink"], closest, worst)
            d_grad = twin.distance(single["grad"], out["grad"])
            print("real ring, row 0: gradient measured / d:", twin.distance(grads[0], out["grad"]) / d_grad, "d = %.2e" % d_grad)
            assert twin.distance(grads[0], out["grad"]) <= twin.FACTOR * d_grad
        state = out["state"]
        _, _, params, m, v = twin.step_both(key, params, m, v, out["grad"], k, cfg)
    after = CnnRecord(1, n, 2, DEV)
    env.act(policy, record=after, seed=31, step=t)
    torch.cuda.synchronize()
    rows = cnn_twin.rows_of(cpu(ring)[t])
    exact = cnn_twin.act(params, rows, np.zeros(len(rows)))
    d_value, d_logp = cases.layout_margins(key, "trained")
    got_values, got_actions, got_logp = cpu(after.values)[0].reshape(-1), cpu(after.actions)[0].reshape(-1), cpu(after.logprobs)[0].reshape(-1)
    print("values off by", np.abs(got_values - exact["values"]).max(), "d", d_value, "; log-probs off by",
          np.abs(got_logp - exact["logp"][np.arange(len(rows)), got_actions]).max(), "d", d_logp)
    assert not np.array_equal(cpu(policy.params), start)
    assert np.abs(got_values - exact["values"]).max() <= twin.FACTOR * d_value
    assert np.abs(got_logp - exact["logp"][np.arange(len(rows)), got_actions]).max() <= twin.FACTOR * d_logp
    env.close()


def load_tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "overcooked_train_device.py")
    spec = importlib.util.spec_from_file_location("overcooked_train_device", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_training_tool_runs_on_simplecooked(hip_lib):
    tool = load_tool()
    runs = []
    for _ in range(2):
        evaluation = {}
        history = tool.train("simple", 33, 8, 2, 1, game="simplecooked", horizon=8, evaluation=evaluation)
        runs.append((history, evaluation))
    history, evaluation = runs[0]
    assert len(history) == 2 and [entry["optimizer_step"] for entry in history] == [15, 30]
    for entry in history:
        assert entry["episodes"] > 0 and entry["mean_return"] is not None and entry["global_step"] == (entry["update"] + 1) * 8 * 33
        for name in _lib.MAPPO_STATS[:7]:
            assert np.isfinite(entry[name]), name
        assert 0.5 < entry["ratio"] < 1.5 and entry["dist_entropy"] > 0 and entry["critic_grad_norm"] > 0
    assert history[0]["value_loss"] != history[1]["value_loss"]  # the parameters moved between the updates
    # the greedy episode: every world has one score
    assert sum(evaluation["scores"].values()) == 33 and all(score >= 0 for score in evaluation["scores"])
    # two runs agree bit for bit: every stat's mean, the episode totals and the greedy scores
    assert runs[1][0] == history and runs[1][1] == evaluation


def test_parameters_move_and_two_loops_agree_bit_for_bit(hip_lib):
    """the loop of the training tool, by hand, so that the parameter tensor can be compared: one-player random1 too"""
    for key, n in (("simple", 33), ("random1/1p", 33)):
        finals = []
        for _ in range(2):
            torch.manual_seed(4)
            w, h, p, f = cases.shape(key)
            from madrona_rl_envs_playground_amd.simulators import CnnActorCritic
            policy = CnnPolicy.from_module(CnnActorCritic(w, h, f), device=DEV)
            start = cpu(policy.params)
            optimizer, value_norm = MappoOptimizer(policy, lr=1e-2, critic_lr=1e-2), ValueNorm(DEV)
            env = make_env(key, n, 8)
            shuffles = torch.Generator(device=DEV).manual_seed(4)
            record = ring = None
            for update in range(2):
                record, ring = env.rollout(policy, 8, seed=4, first_step=8 * update, record=record, ring=ring)
                advantages, returns = mappo_advantages(record, value_norm)
                indices = minibatch_indices(8 * n * p, 1, 2, generator=shuffles, device=DEV)
                result = mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm, entropy_coef=0.0)
            torch.cuda.synchronize()
            finals.append((cpu(policy.params), cpu(result.stats), cpu(value_norm.state), cpu(record.actions)))
            assert np.isfinite(finals[-1][0]).all() and np.isfinite(finals[-1][1]).all()
            assert not np.array_equal(finals[-1][0], start)
            env.close()
        for a, b, what in zip(finals[0], finals[1], ("parameters", "stats", "ValueNorm state", "actions")):
            same_bits(a, b, f"{key}: {what} of a second loop")
