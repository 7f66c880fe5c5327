#!/usr/bin/env python3
"""The reference's PPO trainer (scripts/cartpole_train_torch.py) with every phase on the device: per update one
``env.rollout`` (collect), one ``gae`` (advantages) and one ``ppo_update`` (E x M Adam steps), then ONE host wait, in which the
episode totals and the update's stats come back.  The flat parameter tensor is the only copy of the weights.

    python tools/cartpole_train_device.py --game cartpole --num-envs 1024 --updates 50

Importable: ``train(num_envs, num_steps, updates, seed) -> list of per-update dicts``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def make_agent(obs_dim, num_actions, seed):
    """The trainer's initialisation (:99-121): orthogonal weights of gain sqrt(2), 1 for the critic's last layer and 0.01
    for the actor's, zero biases."""
    import torch
    from madrona_rl_envs_playground_amd.simulators import MlpAgent
    torch.manual_seed(seed)
    agent = MlpAgent(obs_dim, num_actions)
    with torch.no_grad():
        for net, last in ((agent.critic, 1.0), (agent.actor, 0.01)):
            for index, gain in ((0, 2.0 ** 0.5), (2, 2.0 ** 0.5), (4, last)):
                torch.nn.init.orthogonal_(net[index].weight, gain)
                torch.nn.init.constant_(net[index].bias, 0.0)
    return agent


def train(num_envs, num_steps, updates, seed, game="cartpole", learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
          num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01, vf_coef=0.5,
          max_grad_norm=0.5, log=None):
    """``updates`` iterations of collect, advantages, update.  One dict per update: the learning rate, the mean of every stat
    over the update's E x M rows and the last row's, the episodes finished during the update with their mean return, and
    ``optimizer_step``, the Adam steps taken so far."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.envs.acrobot_env import AcrobotMadronaTorch
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    from madrona_rl_envs_playground_amd.simulators import MlpPolicy, PpoOptimizer, gae, minibatch_indices, ppo_update
    if game == "cartpole":
        env = CartpoleMadronaTorch(num_envs, 0, record_episode_statistics=True)
    elif game == "acrobot":
        env = AcrobotMadronaTorch(num_envs, 0, record_episode_statistics=True)
    else:
        raise ValueError(f"game must be 'cartpole' or 'acrobot', got {game!r}")
    device = torch.device("cuda", 0)
    policy = MlpPolicy.from_module(make_agent(4, env.single_action_space.n, seed), device=device)
    optimizer = PpoOptimizer(policy, lr=learning_rate)
    shuffles = torch.Generator(device=device).manual_seed(seed)
    rows = update_epochs * num_minibatches
    host_stats = torch.empty((rows, len(_lib.PPO_STATS)), dtype=torch.float32).pin_memory()
    rollout, history = None, []
    for update in range(updates):
        if anneal_lr:
            optimizer.lr = (1.0 - update / updates) * learning_rate
        env.clear_episode_totals()
        rollout = env.rollout(policy, num_steps, seed=seed, first_step=update * num_steps, out=rollout)
        advantages, returns = gae(rollout, gamma, gae_lambda)
        indices = minibatch_indices(num_steps * num_envs, num_minibatches, update_epochs, generator=shuffles, device=device)
        result = ppo_update(policy, optimizer, rollout, advantages, returns, indices, clip_coef=clip_coef, ent_coef=ent_coef,
                            vf_coef=vf_coef, max_grad_norm=max_grad_norm, norm_adv=norm_adv, clip_vloss=clip_vloss)
        host_stats.copy_(result.stats, non_blocking=True)
        totals = env.episode_totals()  # the update's one host wait; the copy above lies in front of it on the same stream
        episodes = totals["episodes"]
        entry = {"update": update, "lr": optimizer.lr, "optimizer_step": optimizer.step, "episodes": episodes,
                 "mean_return": totals["returns"][0] / episodes if episodes else None,
                 "global_step": (update + 1) * num_steps * num_envs}
        for column, name in enumerate(_lib.PPO_STATS):
            entry[name] = float(host_stats[:, column].mean())
            entry["last_" + name] = float(host_stats[-1, column])
        history.append(entry)
        if log:
            log(entry)
    env.close()
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=("cartpole", "acrobot"), default="cartpole")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--num-steps", type=int, default=128)
    ap.add_argument("--updates", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    train(args.num_envs, args.num_steps, args.updates, args.seed, game=args.game, log=lambda entry: print(json.dumps(entry), flush=True))


if __name__ == "__main__":
    main()
