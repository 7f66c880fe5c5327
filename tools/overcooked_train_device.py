#!/usr/bin/env python3
"""The reference's MAPPO loop for Overcooked (train/MAPPO/main_player.py with the CNN actor-critic, hidden_size 64, ValueNorm)
with every phase on the device: per update one ``env.rollout`` (collect), one ``mappo_advantages`` (returns and normalised
advantages) and one ``mappo_update`` (ppo_epoch x num_mini_batch actor and critic Adam steps), then ONE host wait, in which the
episode totals and the update's stats come back.  The flat parameter tensor is the only copy of the weights.

    python tools/overcooked_train_device.py --layout cramped_room --num-envs 1024 --num-steps 128 --updates 20

Importable: ``train(layout, num_envs, num_steps, updates, seed) -> list of per-update dicts``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def train(layout, num_envs, num_steps, updates, seed, lr=5e-4, critic_lr=5e-4, lr_decay=False, gamma=0.99, gae_lambda=0.95, ppo_epoch=15,
          num_mini_batch=1, clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, horizon=400,
          log=None):
    """``updates`` iterations of collect, advantages, update with the reference's defaults (train/config.py).  One dict per
    update: the learning rates, the mean of every stat over the update's rows (``train_info``), the episodes finished during the
    update with their mean return, and ``optimizer_step``."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    from madrona_rl_envs_playground_amd.simulators import (CnnActorCritic, CnnPolicy, MappoOptimizer, ValueNorm, mappo_advantages,
                                                             mappo_update, minibatch_indices)
    env = OvercookedMadrona(layout, num_envs, 0, horizon=horizon, record_episode_statistics=True)
    device = torch.device("cuda", 0)
    _, players, height, width, channels = env.static_world_major_observations.shape
    torch.manual_seed(seed)
    policy = CnnPolicy.from_module(CnnActorCritic(width, height, channels), device=device)
    optimizer = MappoOptimizer(policy, lr=lr, critic_lr=critic_lr)
    value_norm = ValueNorm(device)
    shuffles = torch.Generator(device=device).manual_seed(seed)
    rows = ppo_epoch * num_mini_batch
    host_stats = torch.empty((rows, len(_lib.MAPPO_STATS)), dtype=torch.float32).pin_memory()
    record, ring, history = None, None, []
    for update in range(updates):
        if lr_decay:  # utils/util.py:38-43
            optimizer.lr, optimizer.critic_lr = lr - lr * (update / updates), critic_lr - critic_lr * (update / updates)
        env.clear_episode_totals()
        record, ring = env.rollout(policy, num_steps, seed=seed, first_step=update * num_steps, record=record, ring=ring)
        advantages, returns = mappo_advantages(record, value_norm, gamma, gae_lambda)
        indices = minibatch_indices(num_steps * num_envs * players, num_mini_batch, ppo_epoch, generator=shuffles, device=device)
        result = mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm, clip_param=clip_param,
                              entropy_coef=entropy_coef, value_loss_coef=value_loss_coef, max_grad_norm=max_grad_norm,
                              huber_delta=huber_delta)
        host_stats.copy_(result.stats, non_blocking=True)
        totals = env.episode_totals()  # the update's one host wait; the copy above lies in front of it on the same stream
        episodes = totals["episodes"]
        entry = {"update": update, "lr": optimizer.lr, "critic_lr": optimizer.critic_lr, "optimizer_step": optimizer.step,
                 "episodes": episodes, "mean_return": totals["returns"][0] / episodes if episodes else None,
                 "global_step": (update + 1) * num_steps * num_envs}
        for column, name in enumerate(_lib.MAPPO_STATS[:7]):
            entry[name] = float(host_stats[:, column].mean())
        history.append(entry)
        if log:
            log(entry)
    env.close()
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="cramped_room")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--num-steps", type=int, default=128)
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--ppo-epoch", type=int, default=15)
    ap.add_argument("--num-mini-batch", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    train(args.layout, args.num_envs, args.num_steps, args.updates, args.seed, ppo_epoch=args.ppo_epoch, num_mini_batch=args.num_mini_batch,
          log=lambda entry: print(json.dumps(entry), flush=True))


if __name__ == "__main__":
    main()
