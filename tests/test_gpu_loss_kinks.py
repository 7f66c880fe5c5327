"""GPU: the loss heads of the four device learners exactly ON their kinks and floors (tests/kink_cases.py).

The exact cases ask for bits: critics of integer value with old values, returns, the clip width and huber's delta small
integers, so that every per-sample dL/dv is a multiple of 1 / (2 B) and the device's gradient, in whatever order it sums, is the
float64 twin's rounded to float32 -- or the wrong branch was taken.  One row holds every category, further rows one category
alone, so that no error cancels against another.  The tolerance cases (actors at ratio 1 with the clip closed to a point, an
advantage of 0, a constant advantage under normalisation, ValueNorm under its variance floor, the wide head's mask edges) keep
the project's margin: d is the distance of the float32 CPU computation from the twin on the same inputs, the device must be
within 8 d, and each test prints measured / d.  Expected values never come from the device; device-against-device equalities
are extra.  The conditions of every case are asserted on the CPU by tests/test_loss_kinks_api.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_twin  # noqa: E402
import kink_cases as cases  # noqa: E402
import mappo_twin  # noqa: E402
import mlpbase_twin  # noqa: E402
import ppo_twin  # noqa: E402
import test_gpu_agent_update as wide_gpu  # noqa: E402
import test_gpu_balance_mappo as mlp_gpu  # noqa: E402
import test_gpu_mappo_update as cnn_gpu  # noqa: E402
import test_gpu_ppo_update as ppo_gpu  # noqa: E402
import wide_twin  # noqa: E402
import wide_update_twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs import OvercookedMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AgentRecord, CartpoleSimulator, CnnPolicy, ExecMode, MappoOptimizer,  # noqa: E402
                                                         MlpPolicy, WideOptimizer, WidePolicy, agent_act, agent_credit, agent_update,
                                                         mappo_update)

DEV = torch.device("cuda", 0)
FACTOR = mappo_twin.FACTOR
MAPPO = _lib.MAPPO_STATS.index
PPO = ppo_twin.STATS.index
WIDE = wide_gpu.COL
F32 = np.float32


def cuda(array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def same_scalar(got, want, what):
    """a float32 stat of the device against the twin's float64 one, rounded once"""
    same_bits(np.float32(got), np.float32(want), what)


def within(what, got, exact, single, floor=0.0):
    """measured / d of one vector or scalar, printed and bounded by the project's factor; d = |float32 - twin|, at least ``floor``"""
    d = max(mappo_twin.distance(single, exact), floor)
    off = mappo_twin.distance(got, exact)
    ratio = off / d if d > 0 else (0.0 if off == 0 else float("inf"))
    print(what, "measured / d: %.2f, d = %.2e" % (ratio, d))
    assert ratio <= FACTOR, (what, ratio)
    return ratio


# ---------------------------------------------------------------- A: critics exactly on their kinks

def cnn_rows():
    return [("mixed", flags) for flags in sorted(cases.MAPPO_FLAGS)] + [(k, "default") for k in range(len(cases.MAPPO_TABLE))]


@pytest.mark.parametrize("which, flags", cnn_rows(), ids=lambda x: str(x))
def test_cnn_critic_on_its_kinks(hip_lib, which, flags):
    """A1: mrl_mappo_update's critic, B = 64 over two tiles with every category and B = 32 with one alone; the whole critic
    gradient and value_loss are the twin's bit for bit, under all four combinations of huber and value clipping"""
    row = cases.cnn_row(which, flags)
    na = mappo_twin.actor_size(row["layout"])
    stats, grads = cnn_gpu.device_of(row).update(row["indices"])
    same_bits(grads[0][na:], row["twin"]["grad"][na:].astype(F32), f"the critic's gradient, row {which}, {flags}")
    same_scalar(stats[0][MAPPO("value_loss")], row["twin"]["stats"]["value_loss"], f"value_loss, row {which}, {flags}")
    if which == "mixed":
        # the critic's planting leaves the actor's columns alone: they are the plain integer case's at the same clip width
        # (device against device)
        plain = mappo_twin.integer_case(row["layout"])
        device = cnn_gpu.Device(row["layout"], mappo_twin.N, plain["params"], plain["batch"], plain["cfg"]._replace(clip_param=row["cfg"].clip_param))
        plain_stats, plain_grads = device.update(plain["indices"])
        same_bits(grads[0][:na], plain_grads[0][:na], "the actor's gradient")
        for name in ("policy_loss", "dist_entropy", "actor_grad_norm", "ratio", "clipfrac"):
            same_bits(stats[0][MAPPO(name)], plain_stats[0][MAPPO(name)], name)
        same_scalar(stats[0][MAPPO("clipfrac")], row["twin"]["stats"]["clipfrac"], "clipfrac")


@pytest.mark.parametrize("which", ["mixed"] + list(range(len(cases.MAPPO_TABLE))), ids=str)
def test_mlp_critic_on_its_kinks(hip_lib, which):
    """A2: the same ``mappo_critic_sample`` through mrl_mappo_mlp_update, v a constant integer: the head's bias gradient and
    value_loss bit for bit, the body's gradient exactly 0; the head's weight gradient, sum(dL/dv x the body's float output),
    within 8 d"""
    row = cases.mlp_row(which)
    na, head = mlpbase_twin.actor_size(1), mlpbase_twin.HIDDEN + 1
    stats, grads = mlp_gpu.Device(row).update(row["indices"])
    exact, single = row["twin"]["grad"], row["f32"]["grad"]
    same_bits(grads[0][-1:], exact[-1:].astype(F32), f"db_head, row {which}")
    same_scalar(stats[0][MAPPO("value_loss")], row["twin"]["stats"]["value_loss"], f"value_loss, row {which}")
    assert not grads[0][na:-head].any(), "the critic's body has a gradient though the head's weights are 0"
    within(f"mlp row {which}: dW_head", grads[0][-head:-1], exact[-head:-1], single[-head:-1])


def squared_rows():
    return ["mixed"] + list(range(len(cases.SQUARED_TABLE)))


@pytest.mark.parametrize("which", squared_rows(), ids=str)
def test_ppo_critic_on_its_kinks(hip_lib, which):
    """A3: mrl_ppo_update's ``critic_head`` over two tiles of the gradient kernel: dW2, db2 and v_loss bit for bit"""
    row = cases.ppo_row(ppo_gpu.tile(), which)
    stats, grads = ppo_gpu.Device(row["params"], row["batch"], row["cfg"]).update(row["indices"])
    for name, at in zip(("dW2", "db2"), row["slices"]):
        same_bits(grads[0][at], row["twin"]["grad"][at].astype(F32), f"{name} of the critic, row {which}")
    same_scalar(stats[0][PPO("v_loss")], row["twin"]["stats"]["v_loss"], f"v_loss, row {which}")


@pytest.mark.parametrize("which", squared_rows(), ids=str)
def test_wide_critic_on_its_kinks(hip_lib, which):
    """A3: mrl_update_head's value half over two 32-row tiles of the backward kernels: the whole critic and v_loss bit for bit"""
    row = cases.wide_row(which)
    size = len(row["critic"])
    stats, grads = wide_gpu.Device(row["params"], row["rec"], row["cfg"]).update()
    assert stats[0][WIDE["samples"]] == cases.WIDE_SIZE and stats[0][WIDE["status"]] == 0
    same_bits(grads[0][:size], row["twin"]["grad"][:size].astype(F32), f"the critic's gradient, row {which}")
    same_scalar(stats[0][WIDE["v_loss"]], row["twin"]["stats"]["v_loss"], f"v_loss, row {which}")


# ---------------------------------------------------------------- B: the actors at ratio exactly 1 and with nothing to push

class CnnRig:
    """A device rollout of ACTOR_T x 33 worlds (the one of ``test_recomputed_values_and_log_probs_are_the_records_bit_for_bit``)
    and ``run``: one update of one row over all its samples from the rollout's parameters, the old log-probs the record's own
    less ``shift``: (stats row as a dict, gradient)."""
    name = "cramped_room"

    def __init__(self):
        layout, n, t = cases.CNN_LAYOUT, cases.ACTOR_N, cases.ACTOR_T
        self.policy = CnnPolicy.from_module(cnn_twin.make_module(layout, "trained"), device=DEV)
        self.env = OvercookedMadrona(layout, n, 0, horizon=cnn_twin.HORIZON)
        self.record, self.ring = self.env.rollout(self.policy, t, seed=5, first_step=0)
        self.shape, self.count = (t, n, 2), t * n * 2
        self.finish()

    def finish(self):
        torch.cuda.synchronize()
        self.params, self.logprobs = self.policy.params.clone(), self.record.logprobs.clone()
        self.indices = torch.arange(self.count, dtype=torch.int32, device=DEV).view(1, self.count)

    def observations(self):
        return cpu(self.ring)[:self.shape[0]].reshape(self.count, *self.ring.shape[3:])

    def batch(self, advantages):
        t = self.shape[0]
        values = cpu(self.record.values)[:t].reshape(-1)
        return mappo_twin.Batch(self.observations(), cpu(self.record.actions).reshape(-1), cpu(self.logprobs).reshape(-1), values, values,
                                np.asarray(advantages, F32))

    def run(self, clip, advantages, shift=None):
        cfg = cases.LEARNERS[self.name].cfg(clip)
        self.policy.params.copy_(self.params)
        self.record.logprobs.copy_(self.logprobs if shift is None else self.logprobs - cuda(np.asarray(shift, F32)).view(self.shape))
        returns = self.record.values[:self.shape[0]].clone()
        result = mappo_update(self.policy, MappoOptimizer(self.policy), self.record, getattr(self, "ring", None), cuda(np.asarray(advantages, F32)).view(self.shape),
                              returns, self.indices, value_norm=None, clip_param=cfg.clip_param, entropy_coef=cfg.entropy_coef,
                              value_loss_coef=cfg.value_loss_coef, max_grad_norm=cfg.max_grad_norm, huber_delta=cfg.huber_delta,
                              use_huber_loss=cfg.huber, use_clipped_value_loss=cfg.clipped_value, use_max_grad_norm=cfg.clip_grads,
                              stats=True, grads=True)
        stats = cpu(result.stats)[0]
        return {name: stats[MAPPO(name)] for name in _lib.MAPPO_STATS}, cpu(result.grads)[0]

    def at_one(self, stats):
        return stats["ratio"] == 1.0 and stats["clipfrac"] == 0.0

    def close(self):
        self.env.close()


class MlpRig(CnnRig):
    name = "beam"

    def __init__(self):
        n, t = cases.ACTOR_N, cases.ACTOR_T
        self.policy = mlp_gpu.make_policy(1, "trained")
        self.env = BalanceMadronaTorch(n, 0)
        self.record = self.env.rollout(self.policy, t, seed=5, first_step=0)
        self.shape, self.count = (t, n, 2), t * n * 2
        self.finish()

    def observations(self):
        return cpu(self.record.obs)[:self.shape[0]].reshape(self.count, 7)

    def batch(self, advantages):
        made = CnnRig.batch(self, advantages)
        return mlpbase_twin.Batch(*made)


class PpoRig:
    """Cartpole: a device rollout of 33 worlds.  The rollout's head takes logf of the soft-max sum and the update's the double
    logarithm rounded once, so a recorded log-prob is the update's own only to an ulp.  The update's own
    are read off the device first: rows of one sample (twice) at a learning rate of 0 report -logratio in old_approx_kl, and
    record + logratio is the recomputed log-prob exactly (the two lie within an ulp of each other)."""
    name = "cartpole"

    def __init__(self):
        n, t = cases.ACTOR_N, cases.ACTOR_T
        sim = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
        self.params = ppo_twin.initial_params(4, 2, 1.0)
        policy = MlpPolicy(4, 2, device="cuda:0")
        policy.params.copy_(cuda(self.params))
        rollout = sim.rollout_policy(policy, t, seed=9)
        self.count = t * n
        zeros = np.zeros(self.count, F32)
        self.recorded = ppo_twin.Batch(cpu(rollout.obs).reshape(-1, 4), cpu(rollout.actions).reshape(-1), cpu(rollout.logprobs).reshape(-1),
                                       zeros, cpu(rollout.values).reshape(-1), cpu(rollout.values).reshape(-1))
        sim.close()
        still = ppo_twin.Config(lr=0.0, norm_adv=False, clip_vloss=False, max_grad_norm=0.0)
        device = ppo_gpu.Device(self.params, self.recorded, still)
        stats, _ = device.update(np.repeat(np.arange(self.count, dtype=np.int32)[:, None], 2, axis=1), grads=False)
        same_bits(device.state()[0], self.params, "the parameters after updates at a learning rate of 0")
        logratio = -stats[:, PPO("old_approx_kl")]
        assert np.abs(logratio).max() < 1e-6
        print("cartpole: %d of %d recorded log-probs are the update's own" % ((logratio == 0).sum(), self.count))
        self.own = self.recorded._replace(logprobs=(self.recorded.logprobs + logratio).astype(F32))
        self.indices = np.arange(self.count, dtype=np.int32)[None, :]

    def batch(self, advantages):
        return self.own._replace(advantages=np.asarray(advantages, F32))

    def run(self, clip, advantages, shift=None):
        batch = self.batch(advantages)
        if shift is not None:
            batch = batch._replace(logprobs=batch.logprobs - np.asarray(shift, F32))
        stats, grads = ppo_gpu.Device(self.params, batch, cases.LEARNERS[self.name].cfg(clip)).update(self.indices)
        return {name: stats[0][PPO(name)] for name in ppo_twin.STATS}, grads[0]

    def at_one(self, stats):
        return stats["old_approx_kl"] == 0.0 and stats["approx_kl"] == 0.0 and stats["clipfrac"] == 0.0

    def close(self):
        pass


class WideRig:
    """hanabi_very_small: the record ``test_recompute_is_the_acts`` fills with real ``agent_act`` calls"""
    name = "hanabi_very_small"

    def __init__(self):
        n, steps, game = cases.ACTOR_N, 4, self.name
        d, s, a = wide_twin.dims(game)
        sim = wide_gpu.make_sim(game, n)
        self.policy = WidePolicy.from_module(wide_twin.make_agent(game, "peaked", seed=21), device=DEV)
        other = WidePolicy.from_module(wide_twin.make_agent(game, "orthogonal", seed=22), device=DEV)
        self.record = AgentRecord(steps, n, d, s, a, sim.observation_tensor().to_torch().dtype, sim.agent_state_tensor().to_torch().dtype, DEV)
        for t in range(steps):
            agent_act(sim, 0, self.policy, self.record, row=t, seed=9, step=t)
            agent_act(sim, 1, other, None, seed=9, step=t, workspace=self.record.workspace)
            sim.step()
            agent_credit(self.record, sim.reward_tensor().to_torch()[0], sim.done_tensor().to_torch())
        torch.cuda.synchronize()
        self.shape = (steps, n)
        self.cells = np.flatnonzero(cpu(self.record.active).reshape(-1))
        self.count = len(self.cells)
        assert 2 <= self.count < steps * n
        self.params, self.logprobs = self.policy.params.clone(), self.record.logprobs.clone()
        self.sim = sim

    def spread(self, per_sample, fill=0.0):
        """(T, N) float32 holding ``per_sample`` at the active cells"""
        out = np.full(self.shape[0] * self.shape[1], fill, F32)
        out[self.cells] = per_sample
        return out.reshape(self.shape)

    def batch(self, advantages):
        flat = lambda t: cpu(t).reshape((self.shape[0] * self.shape[1],) + tuple(t.shape[2:]))[self.cells]  # noqa: E731
        r = self.record
        return {"obs": flat(r.obs), "state": flat(r.states), "mask": flat(r.action_masks), "actions": flat(r.actions),
                "logprobs": cpu(self.logprobs).reshape(-1)[self.cells], "values": flat(r.values), "advantages": np.asarray(advantages, F32),
                "returns": flat(r.values)}

    def run(self, clip, advantages, shift=None):
        cfg = cases.LEARNERS[self.name].cfg(clip)
        self.policy.params.copy_(self.params)
        self.record.logprobs.copy_(self.logprobs if shift is None else self.logprobs - cuda(self.spread(shift)))
        result = agent_update(self.policy, WideOptimizer(self.policy), self.record, cuda(self.spread(advantages)), self.record.values.clone(),
                              epochs=1, clip_coef=cfg.clip_coef, ent_coef=cfg.ent_coef, vf_coef=cfg.vf_coef, max_grad_norm=cfg.max_grad_norm,
                              norm_adv=cfg.norm_adv, clip_vloss=cfg.clip_vloss, stats=True, grads=True)
        stats = cpu(result.stats)[0]
        assert stats[WIDE["samples"]] == self.count and stats[WIDE["status"]] == 0
        return {name: stats[WIDE[name]] for name in wide_update_twin.STATS}, cpu(result.grads)[0]

    at_one = PpoRig.at_one

    def close(self):
        self.sim.close()


RIGS = {"cramped_room": CnnRig, "beam": MlpRig, "cartpole": PpoRig, "hanabi_very_small": WideRig}


@pytest.mark.parametrize("name", sorted(RIGS))
def test_actor_at_ratio_one_and_at_advantage_zero(hip_lib, name):
    """B1: clip 0 on a record whose old log-probs are the device's own: ratio == 1 == lo == hi, a tie of the two surrogates on
    both ends of the clamp, through which torch passes the full gradient -- within 8 d of the twin (each precision with its own
    log-probs as the old ones) and bit for bit the device's gradient at clip 0.2.  B2: advantage exactly 0 with the old
    log-probs 1 below and 1 above: the surrogates tie at +-0 far outside the clip and the gradient is the entropy term alone --
    within 8 d of the twin, finite, and bit for bit the same row with old log-probs = current."""
    rig, learner = RIGS[name](), cases.LEARNERS[name]
    rng = np.random.default_rng(7)
    advantages, zero = rng.normal(size=rig.count).astype(F32), np.zeros(rig.count, F32)
    assert (advantages > 0).sum() > rig.count // 4 and (advantages < 0).sum() > rig.count // 4
    params, indices = cpu(rig.params) if torch.is_tensor(rig.params) else rig.params, np.arange(rig.count, dtype=np.int32)
    try:
        closed_stats, closed = rig.run(0.0, advantages)
        open_stats, opened = rig.run(0.2, advantages)
        still_stats, still = rig.run(0.2, zero)
        pushed_stats, pushed = rig.run(0.2, zero, shift=cases.signs(rig.count))
        batch = rig.batch(advantages)
    finally:
        rig.close()
    assert rig.at_one(closed_stats) and rig.at_one(open_stats), (closed_stats, open_stats)
    same_bits(learner.actor(closed), learner.actor(opened), f"{name}: the actor's gradient at clip 0 and at clip 0.2")
    rows = cases.actor_rows(learner, params, batch, indices, 0.0)
    d = mappo_twin.distance(learner.actor(rows["twin"]["grad"]), learner.actor(rows["f32"]["grad"]))
    nothing = cases.actor_rows(learner, params, batch, indices, 0.2, shift=cases.signs(rig.count), advantages=zero)
    dropped = mappo_twin.distance(learner.actor(rows["twin"]["grad"]), learner.actor(nothing["twin"]["grad"]))
    print(f"{name}: a dropped surrogate gradient would be {dropped / d:.0f} d away, a halved one {dropped / d / 2:.0f} d")
    assert dropped / 2 > 10 * FACTOR * d  # (a condition of the inputs, in the twin)
    within(f"{name}: actor gradient at clip 0", learner.actor(closed), learner.actor(rows["twin"]["grad"]), learner.actor(rows["f32"]["grad"]))
    # B2
    assert pushed_stats["clipfrac"] == 1.0 and np.isfinite(pushed).all()
    same_bits(learner.actor(pushed), learner.actor(still), f"{name}: the entropy term with the ratio far outside the clip and at 1")
    within(f"{name}: actor gradient at advantage 0", learner.actor(pushed), learner.actor(nothing["twin"]["grad"]),
           learner.actor(nothing["f32"]["grad"]))
    assert np.abs(learner.actor(pushed)).max() > 0


def test_ppo_constant_advantages_normalise_to_zero(hip_lib):
    """B3, mrl_ppo_mean_std: 0.75 everywhere, B = 64: mean exact, standard deviation exactly 0, (A - mean) / (0 + 1e-8) = 0"""
    case = cases.constant_advantage_case("cartpole")
    stats, grads = ppo_gpu.Device(case["params"], case["batch"], case["cfg"]).update(case["indices"])
    plain_stats, plain = ppo_gpu.Device(case["params"], case["zero"], case["plain_cfg"]).update(case["indices"])
    assert stats[0][PPO("pg_loss")] == 0 and np.isfinite(grads).all()
    same_bits(grads[0], plain[0], "the gradient under NORM_ADV with constant advantages and the one of advantages 0 without")
    within("cartpole, constant advantages: gradient", grads[0], case["twin"]["grad"], case["f32"]["grad"])


def test_wide_constant_advantages_normalise_to_zero(hip_lib):
    """B3, mrl_update_moments"""
    name = "hanabi_very_small"
    case = cases.constant_advantage_case(name)
    steps, n = wide_update_twin.record_shape(cases.CONSTANT_SIZE)
    outcome = []
    for batch, cfg in ((case["batch"], case["cfg"]), (case["zero"], case["plain_cfg"])):
        rec = wide_update_twin.make_record(batch, steps, n, case["seed"])
        outcome.append(wide_gpu.Device(case["params"], rec, cfg).update())
    (stats, grads), (_, plain) = outcome
    assert stats[0][WIDE["samples"]] == cases.CONSTANT_SIZE and stats[0][WIDE["status"]] == 0
    assert stats[0][WIDE["pg_loss"]] == 0 and np.isfinite(grads).all()
    same_bits(grads[0], plain[0], "the gradient under NORM_ADV with constant advantages and the one of advantages 0 without")
    within("hanabi_very_small, constant advantages: gradient", grads[0], case["twin"]["grad"], case["f32"]["grad"])


# ---------------------------------------------------------------- C: ValueNorm on its floors

def test_value_norm_on_its_floors_exactly(hip_lib):
    """C1, mrl_mappo_row_sums and mrl_mappo_value_norm on the first minibatch of a sparse-reward run: a fresh state, returns all 0.
    The debiasing term meets its epsilon floor, the variance its floor of 1e-2, the targets are exactly 0 and dL/dv = v / B: the
    critic's gradient and value_loss against int64 numpy bit for bit, the state after one row and after three the float32
    recurrence's"""
    row = cases.floor_case()
    na = mappo_twin.actor_size(row["layout"])
    zero = (0.0, 0.0, 0.0)
    device = cnn_gpu.device_of(row, state=zero)
    stats, grads = device.update(row["indices"][:1])
    same_bits(grads[0][na:], (row["critic"].astype(np.float64) / row["unit"]).astype(F32), "the critic's gradient")
    same_scalar(stats[0][MAPPO("value_loss")], row["value_loss"], "value_loss")
    same_bits(device.state()["value_norm"], row["states"][0], "the ValueNorm state after one row")
    device = cnn_gpu.device_of(row, state=zero)
    device.update(row["indices"], grads=False)
    same_bits(device.state()["value_norm"], row["states"][-1], f"the ValueNorm state after {cases.FLOOR_ROWS} rows")


def test_value_norm_under_its_variance_floor(hip_lib):
    """C2: a run in progress whose debiased variance is a quarter of the floor: the targets are normalised by sqrt(1e-2) = 0.1,
    not by 0.05 -- a wrong floor is a factor 2 in every target"""
    row = cases.under_floor_case()
    device = cnn_gpu.device_of(row, state=cases.UNDER_FLOOR_STATE)
    stats, grads = device.update(row["indices"])
    cnn_gpu.check_row("under the variance floor", stats[0], grads[0], row, mappo_twin.stat_margins(cases.UNDER_FLOOR_CASE[2]))
    exact, single = row["twin"]["state"], row["f32"]["state"]
    d = np.maximum(np.abs(single - exact), np.abs(exact) * 2.0 ** -24)
    got = device.state()["value_norm"]
    print("ValueNorm state measured / d:", np.abs(got - exact) / d)
    assert (np.abs(got - exact) <= FACTOR * d).all()


# ---------------------------------------------------------------- D: the wide head's mask edges

def test_wide_head_with_an_illegal_logit_above_every_legal_one(hip_lib):
    """D1: the soft-max's maximum is taken over the legal actions only"""
    case = cases.illegal_top_case()
    batch = case["batch"]
    size, a = batch["mask"].shape
    steps, n = wide_update_twin.record_shape(size)
    rec = wide_update_twin.make_record(batch, steps, n, case["seed"])
    stats, grads = wide_gpu.Device(case["params"], rec, case["cfg"]).update()
    assert np.isfinite(stats).all() and np.isfinite(grads).all()
    wide_gpu.check_row("an illegal logit of 1e4", stats[0], grads[0], case["twin"], case["f32"], size, wide_update_twin.stat_margins(cases.MASK_WEIGHTS))
    weights, bias = cases.wide_actor_head(case["params"], a)
    assert grads[0][bias][case["column"]] == 0 and not grads[0][weights].reshape(a, -1)[case["column"]].any()


def test_wide_head_with_a_single_legal_action(hip_lib):
    """D2: rows with exactly one legal action, alone in an update: log-prob 0, entropy 0, no gradient for the actor"""
    case = cases.single_legal_case()
    batch = case["batch"]
    size = len(batch["actions"])
    steps, n = wide_update_twin.record_shape(size)
    rec = wide_update_twin.make_record(batch, steps, n, case["seed"])
    # (make_record fills the inactive cells with other rows' masks rolled by one: they stay inactive)
    stats, grads = wide_gpu.Device(case["params"], rec, case["cfg"]).update()
    critic = cases.wide_critic_size(batch["state"].shape[1])
    assert stats[0][WIDE["samples"]] == size and stats[0][WIDE["status"]] == 0
    assert not grads[0][critic:].any(), "the actor has a gradient"
    assert stats[0][WIDE["entropy"]] == 0 and stats[0][WIDE["clipfrac"]] == 1.0
    exact, single = case["twin"], case["f32"]
    for name in ("old_approx_kl", "approx_kl", "pg_loss", "v_loss"):  # ratio = exp(-old)
        within(f"single legal action: {name}", stats[0][WIDE[name]], exact["stats"][name], single["stats"][name],
               floor=abs(exact["stats"][name]) * 2.0 ** -24)
    within("single legal action: gradient", grads[0], exact["grad"], single["grad"])


# ---------------------------------------------------------------- E: a row with nothing to learn

def untouched(before, after, part, what):
    for name in ("params", "exp_avg", "exp_avg_sq"):
        same_bits(after[name][part], before[name][part], f"{what}: the critic's {name}")
    assert not after["exp_avg"][part].any() and not after["exp_avg_sq"][part].any()


def test_cnn_row_with_nothing_to_learn(hip_lib):
    """E: R == v == v_old with clipping by norm on: critic_grad_norm 0, scale = min(max / (0 + 1e-6), 1) = 1, Adam's 0 / (0 +
    eps) = 0 -- the critic's parameters and both halves of its moments keep every bit"""
    row = cases.nothing_cnn()
    na = mappo_twin.actor_size(row["layout"])
    device = cnn_gpu.device_of(row)
    before = device.state()
    stats, grads = device.update(row["indices"])
    assert stats[0][MAPPO("critic_grad_norm")] == 0.0 and stats[0][MAPPO("value_loss")] == 0.0 and not grads[0][na:].any()
    untouched(before, device.state(), slice(na, None), "cnn")
    assert device.optimizer.step == 1


def test_mlp_row_with_nothing_to_learn(hip_lib):
    row = cases.nothing_mlp()
    na = mlpbase_twin.actor_size(1)
    device = mlp_gpu.Device(row)
    before = device.state()
    stats, grads = device.update(row["indices"])
    assert stats[0][MAPPO("critic_grad_norm")] == 0.0 and stats[0][MAPPO("value_loss")] == 0.0 and not grads[0][na:].any()
    untouched(before, device.state(), slice(na, None), "mlp")
    assert not np.array_equal(before["params"][:na], device.state()["params"][:na])  # (the actor did take its step)


def test_ppo_row_with_nothing_to_learn(hip_lib):
    """(one optimizer and one norm for both nets: the actor's gradient is not 0 and the clip scales it; the critic's 0 stays 0)"""
    row = cases.nothing_ppo(ppo_gpu.tile())
    device = ppo_gpu.Device(row["params"], row["batch"], row["cfg"])
    names = ("params", "exp_avg", "exp_avg_sq")
    before = dict(zip(names, device.state()))
    stats, grads = device.update(row["indices"])
    size = row["critic_size"]
    assert stats[0][PPO("v_loss")] == 0.0 and stats[0][PPO("total_norm")] > 0 and not grads[0][:size].any() and grads[0][size:].any()
    untouched(before, dict(zip(names, device.state())), slice(0, size), "ppo")


def test_wide_row_with_nothing_to_learn(hip_lib):
    row = cases.nothing_wide()
    device = wide_gpu.Device(row["params"], row["rec"], row["cfg"])
    names = ("params", "exp_avg", "exp_avg_sq")
    before = dict(zip(names, device.state()))
    stats, grads = device.update()
    size = cases.wide_critic_size(row["rec"]["states"].shape[2])
    assert stats[0][WIDE["status"]] == 0 and stats[0][WIDE["v_loss"]] == 0.0 and not grads[0][:size].any()
    untouched(before, dict(zip(names, device.state())), slice(0, size), "wide")
