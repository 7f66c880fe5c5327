"""Float64 twin of ``mrl_agent_update`` (include/mrl_envs.h): one epoch of the reference's ``CleanPPOAgent`` update
(pantheonrl_extension/vectoragent.py:283-318) written once with torch autograd on ``WideAgent.get_action_and_value`` and run in
float64 (the twin) and in float32 on the CPU, whose distance from the twin is the d of the GPU tests; clip and Adam are
``update_twin.clip_adam``.  Also the synthetic batches and records of tests/test_gpu_agent_update.py, built on the host by
filtering SAMPLES so that a float32 gradient can be compared with the twin at all (tests/test_agent_update_api.py asserts the
conditions).  Nothing here touches a GPU."""
import functools
import types

import numpy as np
import torch

import update_twin
import wide_twin
from madrona_rl_envs_playground_amd import _lib

FACTOR = 8.0
STATS = _lib.AGENT_UPDATE_STATS
LOSS_STATS = ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "loss")
KINK = 1e-5  # no sample closer than this to a kink of the loss
distance = update_twin.distance


def config(**changes):
    cfg = types.SimpleNamespace(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, lr=2.5e-4, beta1=0.9, beta2=0.999,
                                eps=1e-5, norm_adv=True, clip_vloss=True)
    cfg.__dict__.update(changes)
    for name, value in cfg.__dict__.items():  # the float32 values mrl_ppo_config carries, as the other twins hold them
        if isinstance(value, float):
            setattr(cfg, name, update_twin.f32(value))
    return cfg


def agent_from(params, d, s, a, dtype=torch.float64):
    """a ``WideAgent`` of ``dtype`` holding the flat ``params``"""
    agent = wide_twin.WideAgent(d, s, a).to(dtype)
    torch.nn.utils.vector_to_parameters(torch.from_numpy(np.asarray(params, np.float64)).to(dtype), agent.parameters())
    return agent


def pre_activations(agent, obs, state):
    """the pre-activations of the six hidden layers (critic's three, then the actor's) in the agent's dtype: (B, 6, 512) float64"""
    dtype = agent.critic[0].weight.dtype
    out = []
    with torch.no_grad():
        for net, x in ((agent.critic, state), (agent.actor, obs)):
            x = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
            for i in (0, 2, 4):
                z = net[i](x)
                out.append(z.double().numpy())
                x = torch.relu(z)
    return np.stack(out, axis=1)


def epoch(params, batch, cfg, dtype=torch.float64):
    """One epoch's losses and unclipped gradient on the B samples of ``batch`` in ``dtype``: the reference's lines :283-318
    (without the permutation, which only reorders a mean).  {"stats": {name: float}, "grad": (P) float64, "ratio", "value",
    "adv": per sample, float64}."""
    d, s, a = batch["obs"].shape[1], batch["state"].shape[1], batch["mask"].shape[1]
    agent = agent_from(params, d, s, a, dtype)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dtype)  # noqa: E731
    b_logprobs, b_values, b_advantages, b_returns = (t(batch[k]) for k in ("logprobs", "values", "advantages", "returns"))
    mask = torch.from_numpy(np.asarray(batch["mask"]) != 0)
    _, newlogprob, entropy, newvalue = agent.get_action_and_value(t(batch["obs"]), t(batch["state"]), mask,
                                                                  torch.from_numpy(np.asarray(batch["actions"])).long())
    logratio = newlogprob - b_logprobs
    ratio = logratio.exp()
    with torch.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > cfg.clip_coef).to(dtype).mean()
    mb_advantages = b_advantages
    if cfg.norm_adv:
        mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    newvalue = newvalue.view(-1)
    if cfg.clip_vloss:
        v_loss_unclipped = (newvalue - b_returns) ** 2
        v_clipped = b_values + torch.clamp(newvalue - b_values, -cfg.clip_coef, cfg.clip_coef)
        v_loss_clipped = (v_clipped - b_returns) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - b_returns) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - cfg.ent_coef * entropy_loss + v_loss * cfg.vf_coef
    loss.backward()
    grad = torch.cat([p.grad.reshape(-1) for p in agent.parameters()]).double().numpy()
    stats = {"pg_loss": pg_loss, "v_loss": v_loss, "entropy": entropy_loss, "old_approx_kl": old_approx_kl, "approx_kl": approx_kl,
             "clipfrac": clipfrac, "loss": loss}
    return {"stats": {k: float(v.detach().double()) for k, v in stats.items()}, "grad": grad,
            "ratio": ratio.detach().double().numpy(), "value": newvalue.detach().double().numpy(),
            "adv": mb_advantages.detach().double().numpy()}


def step(params, exp_avg, exp_avg_sq, grad, steps_before, cfg):
    """``update_twin.clip_adam`` with the update's configuration: (total_norm, params, exp_avg, exp_avg_sq)"""
    return update_twin.clip_adam(params, exp_avg, exp_avg_sq, grad, steps_before, cfg.max_grad_norm if cfg.max_grad_norm > 0 else None,
                                 cfg.lr, cfg)


# ---------------------------------------------------------------- batches

def hidden3(layers, x):
    """the third hidden activation of one net of ``wide_twin.split``, float64"""
    x = np.asarray(x, np.float64)
    for w, b in layers[:3]:
        x = np.maximum(x @ w.T + b, 0.0)
    return x


def masked_logp(logits, legal):
    masked = np.where(legal, logits, -np.inf)
    top = masked.max(axis=1, keepdims=True)
    return (masked - top) - np.log(np.where(legal, np.exp(masked - top), 0.0).sum(axis=1, keepdims=True))


def perturbed(params, inputs, actions, clip_coef, seed):
    """The "old" parameters the batch's log-probs and values come from: both output layers moved along a drawn direction, by
    an amount calibrated on the case's own candidate pool so that about half of it lands beyond either clip -- the critic's
    |v - v_old| and the actor's |ratio - 1| have their pool median at ``clip_coef``."""
    d, s, a = inputs["obs"].shape[1], inputs["state"].shape[1], inputs["mask"].shape[1]
    rng = np.random.default_rng(seed)
    nets = wide_twin.split(params, d, s, a)  # (views of ``split``'s own float64 copy)
    # critic: v_old = v + k (m - median m)
    w, b = nets["critic"][3]
    direction = rng.normal(size=w.shape)
    m = hidden3(nets["critic"], inputs["state"]) @ direction[0]
    spread = np.sort(np.abs(m - np.median(m)))
    k = clip_coef / (0.5 * (spread[len(m) // 2 - 1] + spread[len(m) // 2]) + 1e-300)
    w += k * direction
    b -= k * np.median(m)
    # actor: old logits = logits + k delta, k by bisection on the median of |ratio - 1|
    w, b = nets["actor"][3]
    direction = rng.normal(size=w.shape)
    h3 = hidden3(nets["actor"], inputs["obs"])
    logits, delta = h3 @ w.T + b, h3 @ direction.T
    legal, rows = np.asarray(inputs["mask"]) != 0, np.arange(len(h3))
    new = masked_logp(logits, legal)[rows, actions]

    def median_off(k):
        return np.median(np.abs(np.exp(new - masked_logp(logits + k * delta, legal)[rows, actions]) - 1.0))
    low, high = 0.0, 1e-3
    while median_off(high) < clip_coef and high < 1e3:
        high *= 2
    for _ in range(40):
        mid = 0.5 * (low + high)
        low, high = (mid, high) if median_off(mid) < clip_coef else (low, mid)
    w += 0.5 * (low + high) * direction
    return np.concatenate([x.reshape(-1) for name in ("critic", "actor") for w, b in nets[name] for x in (w, b)])


def sample_checks(params, cand, cfg):
    """Per candidate sample, float64 unless said: "relu_gap" the smallest |pre-activation| that is not exactly 0 in both float32
    and float64, "pre_d" the largest float32-vs-twin pre-activation distance, "ratio", "moved" = v - v_old, "loss_gap" the
    distance from the nearest kink of the loss that depends on the sample alone (|ratio - 1| = clip, |v - v_old| = clip, the
    value loss's two branches equal off the clip range)."""
    d, s, a = cand["obs"].shape[1], cand["state"].shape[1], cand["mask"].shape[1]
    z64 = pre_activations(agent_from(params, d, s, a, torch.float64), cand["obs"], cand["state"])
    z32 = pre_activations(agent_from(params, d, s, a, torch.float32), cand["obs"], cand["state"])
    both_zero = (z64 == 0) & (z32 == 0)
    gap = np.where(both_zero, np.inf, np.minimum(np.abs(z64), np.abs(z32))).reshape(len(z64), -1).min(axis=1)
    pre_d = np.abs(z64 - z32).reshape(len(z64), -1).max(axis=1)
    out = wide_twin.act(params, cand["obs"], cand["state"], cand["mask"], np.zeros(len(z64)))
    rows = np.arange(len(z64))
    ratio = np.exp(out["logp"][rows, cand["actions"]] - cand["logprobs"].astype(np.float64))
    moved = out["values"] - cand["values"].astype(np.float64)
    c = cfg.clip_coef
    ret = cand["returns"].astype(np.float64)
    clipped = cand["values"].astype(np.float64) + np.clip(moved, -c, c)
    branches = np.where(np.abs(moved) > c, np.abs((out["values"] - ret) ** 2 - (clipped - ret) ** 2), np.inf)
    loss_gap = np.minimum(np.minimum(np.abs(np.abs(ratio - 1) - c), np.abs(np.abs(moved) - c)), branches)
    return {"relu_gap": gap, "pre_d": pre_d, "ratio": ratio, "moved": moved, "loss_gap": loss_gap}


def candidates(game, weights, count, seed, cfg):
    """``count`` candidate samples: inputs from ``wide_twin.case_inputs``, legal actions drawn from the policy, old log-probs and
    values from the twin's forward on the perturbed parameters, returns drawn around the old values."""
    d, s, a = wide_twin.dims(game)
    params = wide_twin.flat(wide_twin.make_agent(game, weights)).astype(np.float64)
    inputs = wide_twin.case_inputs(game, count, seed)
    rng = np.random.default_rng(seed + 17)
    actions = wide_twin.act(params, inputs["obs"], inputs["state"], inputs["mask"], rng.uniform(size=count))["actions"]
    old = wide_twin.act(perturbed(params, inputs, actions, cfg.clip_coef, seed + 5), inputs["obs"], inputs["state"], inputs["mask"],
                        np.zeros(count))
    rows = np.arange(count)
    values = old["values"].astype(np.float32)
    return {"obs": inputs["obs"], "state": inputs["state"], "mask": inputs["mask"].astype(np.uint8), "actions": actions.astype(np.int32),
            "logprobs": old["logp"][rows, actions].astype(np.float32), "values": values,
            "returns": (values + rng.normal(scale=0.5, size=count)).astype(np.float32)}


SEARCHED_BELOW, POOL = 31, 64  # below 31 samples the seed is searched; the perturbation is calibrated on POOL candidates at least


def select(checks, size, cfg):
    """The first ``size`` candidates, in order, that meet the per-sample conditions, such that a quarter at least of them is
    ratio-clipped and a quarter value-clipped: a candidate that is not clipped is passed over once the kept ones could no longer
    reach a quota.  None if the pool does not yield them."""
    ok = (checks["relu_gap"] >= FACTOR * checks["pre_d"].max()) & (checks["loss_gap"] >= KINK)
    clipped = np.stack([np.abs(checks["ratio"] - 1) > cfg.clip_coef, np.abs(checks["moved"]) > cfg.clip_coef], axis=1)
    need = np.array([(size + 3) // 4] * 2)
    kept = []
    for i in np.flatnonzero(ok):
        left = size - len(kept) - 1
        if np.any(np.maximum(need - clipped[i], 0) > left):
            continue
        kept.append(i)
        need = need - clipped[i]
        if len(kept) == size:
            return np.array(kept)
    return None


@functools.lru_cache(maxsize=None)
def make_batch(game, weights, size):
    """B = ``size`` samples that meet the input conditions, kept in candidate order from a pool that is doubled until it yields
    enough -- below ``SEARCHED_BELOW`` samples, where one dropped candidate is already a large share, the seed is advanced
    instead until the first B candidates of a pool are kept --; then the advantages, drawn for the kept samples (their
    normalisation depends on the whole batch) and moved where |A| |ratio - clamp(ratio)| would fall below 10 ``KINK``.  The dict
    also carries "params" (the policy's, float32), "dropped" (the share of the candidates up to the last kept one that were
    passed over) and "pre_d"."""
    seed = wide_twin.case_seed(game, size, weights)
    cfg = config()
    params = wide_twin.flat(wide_twin.make_agent(game, weights))
    pool = max(POOL, size + size // 4 + 16)
    for attempt in range(400):
        cand = candidates(game, weights, pool, seed, cfg)
        checks = sample_checks(params, cand, cfg)
        kept = select(checks, size, cfg)
        if kept is not None and (size >= SEARCHED_BELOW or kept[-1] == size - 1):
            break
        if size >= SEARCHED_BELOW:
            pool *= 2
        else:
            seed += 1000003
    else:
        raise AssertionError("no batch found")
    batch = {k: np.ascontiguousarray(v[kept]) for k, v in cand.items()}
    rng = np.random.default_rng(seed + 23)
    adv = rng.normal(size=size).astype(np.float32)
    ratio = checks["ratio"][kept]
    off = np.abs(ratio - np.clip(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef))
    for _ in range(100):
        a64 = adv.astype(np.float64)
        normed = (a64 - a64.mean()) / (a64.std(ddof=1) + 1e-8)
        bad = (off > 0) & ((np.abs(normed) * off < 10 * KINK) | (np.abs(a64) * off < 10 * KINK))
        if not bad.any():
            break
        adv[bad] += np.float32(0.5)
    else:
        raise AssertionError("advantages stay on a kink")
    batch["advantages"] = adv
    batch["params"] = params
    batch["dropped"] = float(kept[-1] + 1 - size) / float(kept[-1] + 1)
    batch["pre_d"] = float(checks["pre_d"][kept].max())
    batch["seed"] = seed
    return batch


def cells_of(size, steps, num_worlds, seed):
    """the ``size`` active cells of a (steps, num_worlds) record, ascending"""
    return np.sort(np.random.default_rng(seed + 31).permutation(steps * num_worlds)[:size])


def make_record(batch, steps, num_worlds, seed, cells=None):
    """The batch's samples at ``cells`` of a (steps, num_worlds) record in ascending order, numpy arrays by the names of
    ``simulators.AgentRecord`` plus "advantages" and "returns"; the other cells are inactive and hold other rows' data, so a
    gather that reads a wrong cell computes something else."""
    size = len(batch["actions"])
    cells = cells_of(size, steps, num_worlds, seed) if cells is None else np.asarray(cells)
    total = steps * num_worlds
    rng = np.random.default_rng(seed + 37)
    filler = rng.integers(0, size, size=total)
    rec = {}
    for name, key in (("obs", "obs"), ("states", "state"), ("action_masks", "mask"), ("actions", "actions"), ("logprobs", "logprobs"),
                      ("values", "values"), ("advantages", "advantages"), ("returns", "returns")):
        flat = np.roll(batch[key][filler], 1, axis=-1) if batch[key].ndim > 1 else batch[key][filler] + batch[key].dtype.type(1)
        flat = np.ascontiguousarray(flat)
        flat[cells] = batch[key]
        rec[name] = flat.reshape((steps, num_worlds) + batch[key].shape[1:])
    rec["actions"] = rec["actions"] % batch["mask"].shape[1]
    rec["actions"].reshape(-1)[cells] = batch["actions"]
    active = np.zeros(total, np.uint8)
    active[cells] = 1
    rec["active"] = active.reshape(steps, num_worlds)
    rec["cells"] = cells
    return rec


def record_shape(size):
    """(T, N) of the record a batch of ``size`` samples sits in: T = 4 or 5 and about a third of the cells inactive"""
    steps = 4 if size % 2 else 5
    return steps, (3 * size // 2) // steps + 2


# the parity cases of tests/test_gpu_agent_update.py: (game, samples), each with both weight sets
SIZES = (2, 31, 33, 65, 257)
CASES = [(game, n) for game in ("balance", "hanabi_very_small") for n in SIZES] + [("hanabi_full", 65)]
FLAG_CASES = [("hanabi_very_small", 65, {"norm_adv": False}), ("hanabi_very_small", 65, {"clip_vloss": False})]


@functools.lru_cache(maxsize=None)
def parity(game, weights, size, flags=()):
    """the twin's and float32's epoch on the case's batch: (batch, twin, float32)"""
    cfg = config(**dict(flags))
    batch = make_batch(game, weights, size)
    return batch, epoch(batch["params"], batch, cfg, torch.float64), epoch(batch["params"], batch, cfg, torch.float32)


@functools.lru_cache(maxsize=None)
def stat_margins(weights, flags=()):
    """d of the scalar stats: one case's distance is a single draw of a rounding error and bounds nothing,
    so it is the largest float32-vs-twin distance over ``CASES`` at the same weight set and flags."""
    d = {name: 0.0 for name in LOSS_STATS}
    for game, size in CASES:
        _, exact, single = parity(game, weights, size, flags)
        for name in LOSS_STATS:
            d[name] = max(d[name], abs(single["stats"][name] - exact["stats"][name]))
    return d


# ---------------------------------------------------------------- exact integers, critic only

def integer_case(size, seed=wide_twin.INTEGER_SEED, d3=None):
    """``wide_twin.integer_layers`` weights on hanabi_very_small inputs, integer returns, ``size`` samples all active in a (1, size)
    record: with NORM_ADV and CLIP_VLOSS off and vf_coef = 1 the critic's gradient is d_value = (v - R) / B times integers.  B is
    a power of two, so every product and partial sum is an integer over B that float32 holds exactly while the sums of absolute
    terms stay below 2^24.  Returns (params float32, record, expected critic gradient float64, the bound).

    ``d3`` (size,) int64: another B dL/dv per sample, in whatever integer unit the caller holds it -- the expected gradient and
    the bound come back in that unit, and the record's returns and old values (the samples' own v), which state the default
    one, are the caller's to replace (tests/kink_cases.py)."""
    game = "hanabi_very_small"
    d, s, a = wide_twin.dims(game)
    layers = wide_twin.integer_layers(d, s, a)
    # the construction's hidden activations reach a few thousand; scaled-down output and third layers keep the backward sums small
    w4, b4 = layers["critic"][3]
    layers["critic"][3] = (np.sign(w4) * (np.arange(w4.shape[1])[None, :] % 5 == 0), b4)
    inputs = wide_twin.case_inputs(game, size, seed)
    values, logits, bound = wide_twin.integer_forward(layers, inputs["obs"], inputs["state"])
    rng = np.random.default_rng(seed + 1)
    returns = values + rng.integers(-3, 4, size=size)
    # backward in int64: d_value * B = v - R
    x = [np.asarray(inputs["state"], np.int64)]
    for k, (w, b) in enumerate(layers["critic"][:3]):
        x.append(np.maximum(x[-1] @ w.T + b, 0))
    dy = ((values - returns) if d3 is None else np.asarray(d3, np.int64).reshape(size))[:, None]
    grads = [None] * 4
    for k in (3, 2, 1, 0):
        w, _ = layers["critic"][k]
        grads[k] = (dy.T @ x[k], dy.sum(axis=0))
        bound = max(bound, int((np.abs(dy).T @ np.abs(x[k])).max()), int(np.abs(dy).sum(axis=0).max()))
        if k:
            bound = max(bound, int((np.abs(dy) @ np.abs(w)).max()))
            dy = (dy @ w) * (x[k] > 0)
    expected = np.concatenate([g.reshape(-1) for pair in grads for g in pair]).astype(np.float64) / size
    rows = np.arange(size)
    rec = {"obs": inputs["obs"][None], "states": inputs["state"][None], "action_masks": inputs["mask"].astype(np.uint8)[None],
           "actions": inputs["mask"].argmax(axis=1).astype(np.int32)[None], "logprobs": np.zeros((1, size), np.float32),
           "values": values.astype(np.float32)[None], "advantages": np.zeros((1, size), np.float32),
           "returns": returns.astype(np.float32)[None], "active": np.ones((1, size), np.uint8), "cells": rows}
    return wide_twin.integer_params(layers), rec, expected, bound
