"""The float64 twin of MAPPO's MLPBase actor-critic for the balance beam (``mrl_mlpbase_act``, ``mrl_mappo_mlp_update``): the
network of include/mrl_envs.h in torch float64 -- LayerNorm(7), Linear, ReLU, LayerNorm, ``layer_N`` more of those, head --, the
act's head (log-soft-max, the draw from a given u, the first arg-max) and one minibatch of the update: ``mappo_twin``'s losses and
ValueNorm and ``update_twin.clip_adam`` on this network.  Every function takes ``dtype``: the same computation in float32 on the
CPU is torch's own, and its distance from the twin is d, the unit of every margin of the device's tests (the device must be within
``FACTOR`` x d, the project's rule, tests/ppo_twin.py).  Nothing here touches a GPU."""
import collections

import numpy as np
import torch

import mappo_twin
from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic
from mappo_twin import FACTOR, KINK, STATE0, STATS, Config, VARIANTS, huber_loss, mse_loss, value_norm_update  # noqa: F401
from update_twin import clip_adam, clip_adam_torch, distance, f32, make_indices  # noqa: F401

D, A, HIDDEN = 7, 4, 64
FC_H = 4288  # floats of the unused fc_h block per net


def module_from(params, layer_N, dtype=torch.float64):
    """An ``MlpBaseActorCritic`` of ``dtype`` holding the flat parameter vector ``params`` (actor, then critic)."""
    module = MlpBaseActorCritic(layer_N=layer_N).to(dtype)
    source = torch.as_tensor(np.asarray(params, np.float64)).to(dtype)
    at = 0
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(source[at:at + p.numel()].view_as(p))
            at += p.numel()
    assert at == source.numel()
    return module


def flat(module):
    return torch.nn.utils.parameters_to_vector(module.parameters()).detach().double().numpy()


def actor_size(layer_N):
    return 654 + FC_H * (1 + layer_N) + A * HIDDEN + A


def fc_h_slices(layer_N):
    """where the two nets' fc_h blocks lie in the flat tensor"""
    na = actor_size(layer_N)
    return slice(654, 654 + FC_H), slice(na + 654, na + 654 + FC_H)


def used(layer_N):
    """boolean mask over the flat tensor: everything but the two fc_h blocks"""
    mask = np.ones(actor_size(layer_N) + actor_size(layer_N) - (A - 1) * (HIDDEN + 1), bool)
    for s in fc_h_slices(layer_N):
        mask[s] = False
    return mask


def net_forward(net, x, head):
    """(head output, [every hidden layer's Linear output]) of one net's base and ``head`` on x (n, 7), written out layer by layer"""
    base = net.base
    y = torch.nn.functional.layer_norm(x, (D,), base.feature_norm.weight, base.feature_norm.bias, 1e-5)
    pre = []
    for seq in [base.mlp.fc1] + list(base.mlp.fc2):
        z = seq[0](y)
        pre.append(z)
        y = seq[2](torch.relu(z))
    return head(y), pre


def forward(module, rows):
    """(values (n,), logits (n, 4), pre-activations of both nets' hidden layers) as tensors of the module's dtype"""
    x = torch.from_numpy(np.array(rows)).to(next(module.parameters()).dtype)
    logits, pre_a = net_forward(module.actor, x, module.actor.act.action_out.linear)
    values, pre_c = net_forward(module.critic, x, module.critic.v_out)
    return values[:, 0], logits, pre_a + pre_c


def act(params, rows, u, layer_N, dtype=torch.float64):
    """The head of include/mrl_envs.h: ``values``; ``logits``; ``logp`` (n, 4); ``cdf`` (n, 3) the boundaries p_0 + ... + p_a;
    ``actions`` drawn from ``u``; ``greedy`` the first arg-max.  float64 numpy arrays, computed in ``dtype``."""
    with torch.no_grad():
        values, logits, _ = forward(module_from(params, layer_N, dtype), rows)
        logp = torch.log_softmax(logits, dim=1)
    values, logits, logp = (t.double().numpy() for t in (values, logits, logp))
    cdf = np.cumsum(np.exp(logp), axis=1)[:, :-1]
    actions = (np.asarray(u, np.float64)[:, None] >= cdf).sum(axis=1).astype(np.int32)
    return {"values": values, "logits": logits, "logp": logp, "cdf": cdf, "actions": actions, "greedy": logits.argmax(axis=1).astype(np.int32)}


def near_boundary(cdf, u, tol=1e-5):
    """rows whose draw lies within ``tol`` of a boundary: the only ones whose action a float32 evaluation may decide otherwise"""
    return (np.abs(np.asarray(u, np.float64)[:, None] - cdf) <= tol).any(axis=1)


def act_margins(params, rows, layer_N):
    """(d of the values, d of the log-probabilities, d of the logits) on these rows: float32 on the CPU against the twin"""
    exact, single = act(params, rows, np.zeros(len(rows)), layer_N), act(params, rows, np.zeros(len(rows)), layer_N, torch.float32)
    return tuple(float(np.abs(single[k] - exact[k]).max()) for k in ("values", "logp", "logits"))


Batch = collections.namedtuple("Batch", "obs actions logprobs values returns advantages")  # obs (S, 7) int32; the rest (S,)


def row(params, layer_N, batch, mb_inds, cfg, state=(0.0, 0.0, 0.0), dtype=torch.float64):
    """One minibatch in ``dtype`` on the CPU, ``mappo_twin.row`` on this network: {"grad": (P,) float64, actor then critic, zero over
    fc_h (autograd leaves its grad None); "stats"; "state"; "norm"; "kink"; "branches"; "pre"}."""
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    module = module_from(params, layer_N, dtype)
    inds = np.asarray(mb_inds).astype(np.int64)
    rows = np.asarray(batch.obs)[inds]
    actions, old_logp, old_v, returns, adv = (torch.from_numpy(np.ascontiguousarray(np.asarray(a)[inds])) for a in
                                              (batch.actions, batch.logprobs, batch.values, batch.returns, batch.advantages))
    old_logp, old_v, adv = old_logp.to(dtype), old_v.to(dtype), adv.to(dtype)
    c = cfg.clip_param
    v, logits, pre = forward(module, rows)
    logp = torch.log_softmax(logits, dim=1)
    entropy = -(logp.exp() * logp).sum(dim=1).mean()
    ratio = (logp.gather(1, actions.long().unsqueeze(1)).squeeze(1) - old_logp).exp()
    surr1, surr2 = ratio * adv, ratio.clamp(1.0 - c, 1.0 + c) * adv
    policy_loss = -torch.min(surr1, surr2).mean()
    (policy_loss - entropy * cfg.entropy_coef).backward()

    new_state, norm = np.asarray(state, np_dtype), (np_dtype(0), np_dtype(1))
    target = returns.to(dtype)
    if cfg.valuenorm:
        new_state, mean, std = value_norm_update(state, returns.numpy(), cfg, np_dtype)
        norm = (mean, std)
        target = (target - float(mean)) / float(std) if dtype == torch.float64 else (target - torch.tensor(mean)) / torch.tensor(std)
    v_c = old_v + (v - old_v).clamp(-c, c)
    e, e_c = target - v, target - v_c
    term = (lambda err: huber_loss(err, cfg.huber_delta)) if cfg.huber else mse_loss
    plain, clipped = term(e), term(e_c)
    value_loss = (torch.max(plain, clipped) if cfg.clipped_value else plain).mean()
    (value_loss * cfg.value_loss_coef).backward()

    grad = torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in module.parameters()]).double().numpy()
    na = actor_size(layer_N)
    stats = {"value_loss": value_loss.item(), "policy_loss": policy_loss.item(), "dist_entropy": entropy.item(),
             "ratio": ratio.mean().item(), "clipfrac": ((ratio - 1).abs() > c).to(dtype).mean().item(),
             "actor_grad_norm": float(np.sqrt(np.sum(grad[:na] ** 2))), "critic_grad_norm": float(np.sqrt(np.sum(grad[na:] ** 2)))}
    arr = lambda t: t.detach().double().numpy()  # noqa: E731
    ratio_, v_, old_, e_, ec_ = arr(ratio), arr(v), arr(old_v), arr(e), arr(e_c)
    kinks = [np.abs(ratio_ - (1 - c)), np.abs(ratio_ - (1 + c))]
    if cfg.clipped_value:
        kinks.append(np.abs(np.abs(v_ - old_) - c))
        dead = (e_ < -cfg.huber_delta) & (ec_ < -cfg.huber_delta) if cfg.huber else np.zeros_like(e_, bool)
        kinks.append(np.where((np.abs(v_ - old_) > c) & ~dead, np.abs(arr(plain) - arr(clipped)), np.inf))
    if cfg.huber:
        kinks.append(np.abs(np.abs(e_) - cfg.huber_delta))
        if cfg.clipped_value:
            kinks.append(np.abs(np.abs(ec_) - cfg.huber_delta))
    branches = {"ratio_clipped": float(((ratio_ > 1 + c) | (ratio_ < 1 - c)).mean()), "value_clipped": float((np.abs(v_ - old_) > c).mean()),
                "huber_above": float((e_ > cfg.huber_delta).mean()), "huber_below": float((e_ < -cfg.huber_delta).mean())}
    return {"grad": grad, "stats": stats, "state": np.asarray(new_state, np.float64), "norm": (float(norm[0]), float(norm[1])),
            "kink": float(np.min(kinks)), "branches": branches, "pre": [arr(z) for z in pre]}


def step_both(layer_N, params, exp_avg, exp_avg_sq, grad, step, cfg):
    """both nets' clip and Adam on the flat arrays, as the reference's optimizers see them -- WITHOUT fc_h, whose grad is None:
    (actor_norm, critic_norm, params, exp_avg, exp_avg_sq); the fc_h entries come back as they went in"""
    na = actor_size(layer_N)
    keep = used(layer_N)
    limit = cfg.max_grad_norm if cfg.clip_grads else None
    out = [np.array(a, np.float64) for a in (params, exp_avg, exp_avg_sq)]
    norms = []
    for sl, lr in ((slice(0, na), cfg.lr), (slice(na, None), cfg.critic_lr)):
        k = keep[sl]
        res = clip_adam(out[0][sl][k], out[1][sl][k], out[2][sl][k], np.asarray(grad, np.float64)[sl][k], step, limit, lr, cfg)
        norms.append(res[0])
        for dst, new in zip(out, res[1:]):
            part = dst[sl]
            part[k] = new
    return (norms[0], norms[1]) + tuple(out)


relu_margin = mappo_twin.relu_margin
conditions_hold = mappo_twin.conditions_hold
row_margins = mappo_twin.row_margins
