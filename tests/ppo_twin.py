"""The float64 twin of ``mrl_ppo_update``: torch autograd in float64 over the loss that include/mrl_envs.h states (the one
of the reference trainer's update, scripts/cartpole_train_torch.py:275-310) plus a float64 clip_grad_norm_ and Adam in numpy,
the same function in torch float32 on the CPU -- whose distance from the twin is d, the unit of every margin of the update's tests --, the synthetic batches the
tests run and the cases of tests/test_gpu_ppo_update.py.  Nothing here touches a GPU.

Hyper-parameters cross the C ABI as float32, so the twin takes them rounded to float32 (``Config``): the device and the twin
then compute with the same numbers, and d measures arithmetic only."""
import collections
import functools

import numpy as np
import torch

import policy_twin
import update_twin
from madrona_rl_envs_playground_amd.simulators import MlpAgent
# (the tests reach these through this module)
from update_twin import distance, f32, make_indices, moments, tile_size  # noqa: F401

STATS = ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "total_norm", "loss")
KINK = 1e-5       # no sample of a fixed case may lie this close to a kink of the loss (in the twin)
FACTOR = 8.0      # the device must be within FACTOR x d (tests/test_gpu_policy_rollout.py grants the same)
BATCH = 4099      # S of every GPU case: gathers are real
SHAPES = [(4, 2), (4, 3), (6, 3)]
SCALES = [1.0, 100.0]
FIXED_SIZES = [2, 63, 65, 257, 2049]
CHAIN_SIZES = [63, 257]
CHAIN_ROWS = 6
CHAIN_MAX_SKIPPED = 1
# the Adam parity cases: unnormalised advantages of std 3 give a gradient norm above the trainer's max_grad_norm of 0.5
ADAM_CASES = [(d, a, 1.0, 63, "no_norm_adv") for d, a in SHAPES]
# a case is (D, A, scale, B, variant) -> seed of its batch and its index row; a seed that fails the branch conditions of
# tests/test_ppo_update_api.py is replaced here, not excused there
SEEDS = {
    (4, 2, 1.0, 2049, "default"): 218544,   # a sample within 1e-5 of a kink under the derived seed
    (4, 2, 1.0, 197, "default"): 105580,    # the same
    (4, 3, 100.0, 2049, "default"): 218743,  # the same
    (6, 3, 100.0, 2049, "default"): 120743,  # the same
    # the sizes beyond the workgroup cap use all 4 099 samples several times over: the derived seeds all have such a sample
    (4, 2, 1.0, 16389, "default"): 318924,
    (4, 2, 1.0, 32837, "default"): 234060,
    (4, 3, 1.0, 16389, "default"): 119024,
    (4, 3, 1.0, 32837, "default"): 334160,
    (6, 3, 1.0, 16389, "default"): 421024,
    (6, 3, 1.0, 32837, "default"): 236160,
}


class Config(collections.namedtuple("Config", "clip_coef ent_coef vf_coef max_grad_norm lr beta1 beta2 eps norm_adv clip_vloss")):
    """What ``ppo_update`` and ``PpoOptimizer`` are given, every float rounded to float32."""

    def __new__(cls, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-5,
                norm_adv=True, clip_vloss=True):
        return super().__new__(cls, f32(clip_coef), f32(ent_coef), f32(vf_coef), f32(max_grad_norm), f32(lr), f32(beta1), f32(beta2),
                               f32(eps), bool(norm_adv), bool(clip_vloss))


VARIANTS = {"default": Config(), "no_norm_adv": Config(norm_adv=False), "no_clip_vloss": Config(clip_vloss=False),
            "no_grad_clip": Config(max_grad_norm=0.0), "no_entropy": Config(ent_coef=0.0)}


def flat(agent):
    return torch.cat([p.detach().reshape(-1) for net in (agent.critic, agent.actor) for p in net.parameters()])


def flat_grad(agent):
    return torch.cat([p.grad.reshape(-1) for net in (agent.critic, agent.actor) for p in net.parameters()])


def agent_from(params, obs_dim, num_actions, dtype):
    """An ``MlpAgent`` of ``dtype`` holding the flat parameter vector ``params``."""
    agent = MlpAgent(obs_dim, num_actions, policy_twin.H).to(dtype)
    source = torch.as_tensor(np.asarray(params, np.float64)).to(dtype)
    at = 0
    with torch.no_grad():
        for net in (agent.critic, agent.actor):
            for p in net.parameters():
                p.copy_(source[at:at + p.numel()].view_as(p))
                at += p.numel()
    assert at == source.numel()
    return agent


Batch = collections.namedtuple("Batch", "obs actions logprobs advantages returns values")  # float32 / int32 numpy, S samples


def clipped_surrogate(advantage, ratio, clip):
    """per sample: the larger of -A ratio and -A clamp(ratio, 1 - clip, 1 + clip)"""
    return torch.maximum(-advantage * ratio, -advantage * ratio.clamp(1 - clip, 1 + clip))


def value_error(value, old_value, target, clip, clipped):
    """per sample: (v - R)^2, or with ``clipped`` the larger of it and (v_old + clamp(v - v_old, -clip, clip) - R)^2; also
    the clamped value itself, for the kink census"""
    near = old_value + (value - old_value).clamp(-clip, clip)
    plain = (value - target).square()
    return (torch.maximum(plain, (near - target).square()) if clipped else plain), near


def ppo_loss(agent, mb, cfg):
    """The PPO loss of include/mrl_envs.h (mrl_ppo_update) for the gathered minibatch ``mb`` (a ``Batch`` of tensors of the
    agent's dtype): {"loss": the tensor to differentiate, "stats": the logged numbers as Python floats, "ratio" / "value" /
    "near": per-sample arrays for the kink census}."""
    logp = torch.log_softmax(agent.actor(mb.obs), dim=1)
    entropy = -(logp.exp() * logp).sum(dim=1).mean()
    log_ratio = logp.gather(1, mb.actions.long().unsqueeze(1)).squeeze(1) - mb.logprobs
    ratio = log_ratio.exp()
    advantage = mb.advantages
    if cfg.norm_adv:
        advantage = (advantage - advantage.mean()) / (advantage.std() + 1e-8)
    policy_term = clipped_surrogate(advantage, ratio, cfg.clip_coef).mean()
    value = agent.critic(mb.obs).squeeze(1)
    squared, near = value_error(value, mb.values, mb.returns, cfg.clip_coef, cfg.clip_vloss)
    value_term = 0.5 * squared.mean()
    loss = policy_term - cfg.ent_coef * entropy + cfg.vf_coef * value_term
    with torch.no_grad():
        stats = {"pg_loss": policy_term.item(), "v_loss": value_term.item(), "entropy": entropy.item(),
                 "old_approx_kl": (-log_ratio).mean().item(), "approx_kl": (ratio - 1 - log_ratio).mean().item(),
                 "clipfrac": ((ratio - 1).abs() > cfg.clip_coef).float().mean().item(), "loss": loss.item()}
    as_array = lambda t: t.detach().double().numpy()  # noqa: E731
    return {"loss": loss, "stats": stats, "ratio": as_array(ratio), "value": as_array(value), "near": as_array(near)}


def row(params, batch, mb_inds, cfg, dtype=torch.float64):
    """One minibatch in ``dtype`` on the CPU: {"grad": (P,) float64, "stats": dict (with total_norm), "kink": the smallest
    distance of a sample from a kink, "branches": the fractions clipped high, clipped low and value-clipped}."""
    agent = agent_from(params, batch.obs.shape[1], int(_num_actions(params, batch.obs.shape[1])), dtype)
    inds = np.asarray(mb_inds).astype(np.int64)
    gathered = [torch.from_numpy(np.ascontiguousarray(np.asarray(a)[inds])) for a in batch]
    out = ppo_loss(agent, Batch(*[t.to(dtype) if t.dtype.is_floating_point else t for t in gathered]), cfg)
    out["loss"].backward()
    grad = flat_grad(agent).double().numpy()
    stats = out["stats"]
    stats["total_norm"] = float(torch.linalg.vector_norm(flat_grad(agent)).item())
    c = cfg.clip_coef
    ratio, v, vc = out["ratio"], out["value"], out["near"]
    old, ret = (np.asarray(a, np.float64)[inds] for a in (batch.values, batch.returns))
    kinks = [np.abs(ratio - (1 - c)), np.abs(ratio - (1 + c))]
    if cfg.clip_vloss:
        moved = np.abs(v - old)
        kinks.append(np.abs(moved - c))
        # where the value is clipped, the larger of the two squared errors changes hands at |v - R| = |v_clipped - R|
        kinks.append(np.where(moved > c, np.abs(np.abs(v - ret) - np.abs(vc - ret)), np.inf))
    branches = {"clipped_high": float((ratio > 1 + c).mean()), "clipped_low": float((ratio < 1 - c).mean()),
                "value_clipped": float((np.abs(v - old) > c).mean())}
    return {"grad": grad, "stats": stats, "kink": float(np.min(kinks)), "branches": branches}


def _num_actions(params, obs_dim):
    h = policy_twin.H
    critic = obs_dim * h + h + h * h + h + h + 1
    rest = np.asarray(params).size - critic - (obs_dim * h + h + h * h + h)
    assert rest % (h + 1) == 0
    return rest // (h + 1)


def clip_adam(params, exp_avg, exp_avg_sq, grad, step, cfg):
    """``update_twin.clip_adam`` (lines 314 and 315) as the trainer's flags put it: no clipping at ``max_grad_norm`` <= 0"""
    return update_twin.clip_adam(params, exp_avg, exp_avg_sq, grad, step, cfg.max_grad_norm if cfg.max_grad_norm > 0 else None, cfg.lr, cfg)


def clip_adam_torch(params, exp_avg, exp_avg_sq, grad, step, cfg, dtype):
    return update_twin.clip_adam_torch(params, exp_avg, exp_avg_sq, grad, step, cfg.max_grad_norm if cfg.max_grad_norm > 0 else None,
                                       cfg.lr, cfg, dtype)


def make_batch(params, obs_dim, num_actions, size, seed):
    """S samples whose "old" data put a good share of them on every branch of the loss under ``params``: observations
    N(0, 1), uniform actions, old_logprob = current + U(-0.4, 0.4), old_value = current + U(-0.5, 0.5), returns = old_value +
    N(0, 1), advantages = N(0, 3)."""
    rng = np.random.default_rng(seed)
    obs = rng.normal(size=(size, obs_dim)).astype(np.float32)
    actions = rng.integers(0, num_actions, size=size).astype(np.int32)
    now = policy_twin.act(params, obs, np.zeros(size), num_actions)
    logprobs = (now["logp"][np.arange(size), actions] + rng.uniform(-0.4, 0.4, size=size)).astype(np.float32)
    values = (now["values"] + rng.uniform(-0.5, 0.5, size=size)).astype(np.float32)
    returns = (values + rng.normal(size=size)).astype(np.float32)
    advantages = rng.normal(scale=3.0, size=size).astype(np.float32)
    return Batch(obs, actions, logprobs, advantages, returns, values)


@functools.lru_cache(maxsize=None)
def initial_params(obs_dim, num_actions, scale):
    agent = policy_twin.make_agent(obs_dim, num_actions, policy_twin.AGENT_SEED, actor_scale=scale)
    return flat(agent).numpy().astype(np.float32)


def seed_of(case):
    """``case`` = (D, A, scale, B, variant)"""
    d, a, scale, width, variant = case
    return SEEDS.get(case, 1000 * d + 100 * a + int(scale) + 7 * width + 13 * sorted(VARIANTS).index(variant))


@functools.lru_cache(maxsize=None)
def fixed_case(case, rows=1, draw=0):
    """Parameters, batch and index rows of a fixed-agent case, and for row 0 the twin and torch's float32 computation.
    ``draw`` > 0 gives further batches of the same case (``stat_margins``)."""
    d, a, scale, width, variant = case
    params = initial_params(d, a, scale)
    seed = seed_of(case) + 1000003 * draw
    batch = make_batch(params, d, a, BATCH, seed)
    indices = make_indices(rows, width, BATCH, seed)
    cfg = VARIANTS[variant]
    return {"params": params, "batch": batch, "indices": indices, "cfg": cfg, "twin": row(params, batch, indices[0], cfg),
            "f32": row(params, batch, indices[0], cfg, torch.float32)}


def row_margins(twin_row, f32_row):
    """d per kind of number of one row: {"grad": .., stat name: ..}"""
    d = {"grad": distance(twin_row["grad"], f32_row["grad"])}
    for name in STATS:
        d[name] = abs(twin_row["stats"][name] - f32_row["stats"][name])
    return d


STAT_DRAWS = 3  # batches per shape that a scalar stat's d is the largest over


@functools.lru_cache(maxsize=None)
def stat_margins(case):
    """d of every scalar stat of ``case``: the largest distance of torch's float32 computation from the twin over the three
    shapes and three batches each, at the case's own weight set, minibatch size and flags.  One row's own distance is a
    single draw of a float32 rounding error -- anywhere between nothing and an ulp of the stat, 0.01 ulp in some of these
    cases --, so it bounds no other float32 computation; the largest of nine draws is the ulp-sized d that the vector kinds
    get from the largest of their 9 155 elements.  The weight sets are not pooled: the scaled actor's stats are larger.  A
    batch with a sample within 1e-5 of a kink is passed over: there the two computations may take different branches."""
    _, _, scale, width, variant = case
    d = {name: 0.0 for name in STATS}
    for shape in SHAPES:
        used, draw = 0, 0
        while used < STAT_DRAWS:
            fixed = fixed_case((shape[0], shape[1], scale, width, variant), 1, draw)
            draw += 1
            assert draw < 64
            if fixed["twin"]["kink"] <= KINK:
                continue
            used += 1
            own = row_margins(fixed["twin"], fixed["f32"])
            for name in STATS:
                d[name] = max(d[name], own[name])
    return d


def saturation(workspace_bytes):
    """The cap on partial vectors times the tile: the largest B at which every workgroup still takes a single tile."""
    return update_twin.saturation(workspace_bytes)[1]


def large_sizes(tile_size, saturation_size):
    """Sizes at which a workgroup of the gradient kernel takes several tiles: one tile past the cap (two tiles per workgroup,
    so fewer workgroups than the cap, and a last one of a single ragged tile), and a tile and five samples past twice the cap
    (three tiles per workgroup, the last one again a single ragged tile)."""
    return [saturation_size + 5, 2 * saturation_size + tile_size + 5]


def large_cases(tile_size, saturation_size):
    return [(d, a, 1.0, width, "default") for d, a in SHAPES for width in large_sizes(tile_size, saturation_size)]


def gpu_cases(tile_size):
    """Every (D, A, scale, B, variant) tests/test_gpu_ppo_update.py runs for parity; ``tile_size`` is the gradient kernel's
    tile, from which the size with three workgroups and a ragged tail follows."""
    cases = []
    for d, a in SHAPES:
        for scale in SCALES:
            for width in FIXED_SIZES + [3 * tile_size + 5]:
                cases.append((d, a, scale, width, "default"))
    for d, a in SHAPES:
        for variant in sorted(VARIANTS):
            if variant != "default":
                cases.append((d, a, 1.0, 257, variant))
    return cases


# ---------------------------------------------------------------- the exact construction (critic only)

def integer_case(count, d3=None, seed=3):
    """The construction of ``test_matrix_core_operand_maps_with_exact_integers`` (tests/test_gpu_ppo_update.py) with the upstream
    gradient as an argument: a first layer that saturates tanh (h1 in {-1, 0, 1}), a second layer of zeros (h2 = 0, v = 0 exactly,
    d2[j] = W3[j] d3), W3[j] = j - 20, an actor of zeros.  ``d3`` (count,) int64: dL/dv per sample in whatever integer unit the
    caller holds it; by default -r for drawn integers r, which returns of 2 count r give with vf_coef 0.5 and no value clipping.
    Returns {"params", "batch" (old values 0), "dW2" (64, 64) and "db2" (64,) int64 in d3's unit, "bound": the largest sum of
    absolute terms, "slices": where dW2 and db2 lie in the flat gradient}; with a ``d3`` the returns and old values are the
    caller's to replace (tests/kink_cases.py)."""
    d, a, h = 4, 2, policy_twin.H
    rng = np.random.default_rng(seed)
    patterns = np.array([[(i + 1) // 3 ** k % 3 - 1 for k in range(d)] for i in range(h)], np.int64)  # 64 different rows of -1 / 0 / 1
    obs = rng.choice([-1, 1], size=(count, d)).astype(np.int64)
    r = rng.integers(-3, 4, size=count).astype(np.int64)
    d3 = -r if d3 is None else np.asarray(d3, np.int64).reshape(count)
    w3 = np.arange(h, dtype=np.int64) - 20
    critic = np.concatenate([(64.0 * patterns).reshape(-1), np.zeros(h), np.zeros(h * h), np.zeros(h), w3.astype(np.float64), np.zeros(1)])
    params = np.concatenate([critic, np.zeros(initial_params(d, a, 1.0).size - critic.size)]).astype(np.float32)
    batch = Batch(obs.astype(np.float32), np.zeros(count, np.int32), np.full(count, np.log(0.5), np.float32), np.zeros(count, np.float32),
                  (2.0 * count * r).astype(np.float32), np.zeros(count, np.float32))
    h1 = np.sign(patterns @ obs.T)          # (unit of layer 1, sample)
    d2 = w3[:, None] * d3[None, :]          # (unit of layer 2, sample)
    at = d * h + h
    return {"params": params, "batch": batch, "dW2": d2 @ h1.T, "db2": d2.sum(axis=1),
            "bound": int(max((np.abs(d2) @ np.abs(h1).T).max(), np.abs(d2).sum(axis=1).max())),
            "slices": (slice(at, at + h * h), slice(at + h * h, at + h * h + h))}
