#!/usr/bin/env python3
"""The reference's MAPPO loop for the two kitchens (train/MAPPO/main_player.py with the CNN actor-critic, hidden_size 64, ValueNorm)
with every phase on the device: per update one ``env.rollout`` (collect), one ``mappo_advantages`` (returns and normalised
advantages) and one ``mappo_update`` (ppo_epoch x num_mini_batch actor and critic Adam steps), then ONE host wait, in which the
episode totals and the update's stats come back.  The flat parameter tensor is the only copy of the weights.

    python tools/overcooked_train_device.py --layout cramped_room --num-envs 1024 --num-steps 128 --updates 20
    python tools/overcooked_train_device.py --game simplecooked --recipe colab --evaluate

``--game simplecooked`` is the world the reference's trainer binds (train/env_utils.py:3); ``--recipe colab`` sets what its
notebook overcooked_compiled_colab.ipynb trains (``RECIPES``), and ``--evaluate`` is that notebook's test cell: one greedy episode
in every world, then the histogram of the worlds' scores.

Importable: ``train(layout, num_envs, num_steps, updates, seed) -> list of per-update dicts``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

GAMES = ("overcooked", "simplecooked")
# overcooked_compiled_colab.ipynb: layout simple, 800 worlds, episode_length 200 (= the horizon), ppo_epoch 7, one minibatch,
# lr = critic_lr = 1e-2, entropy_coef 0, 8 M env steps = 8 000 000 / (200 * 800) = 50 updates
RECIPES = {"colab": {"game": "simplecooked", "layout": "simple", "num_envs": 800, "num_steps": 200, "horizon": 200, "updates": 50,
                     "ppo_epoch": 7, "num_mini_batch": 1, "lr": 1e-2, "critic_lr": 1e-2, "entropy_coef": 0.0}}
# what the command line sets when neither the option nor a recipe does: today's
DEFAULTS = {"game": "overcooked", "layout": "cramped_room", "num_envs": 1024, "num_steps": 128, "horizon": 400, "updates": 20,
            "ppo_epoch": 15, "num_mini_batch": 1, "lr": 5e-4, "critic_lr": 5e-4, "entropy_coef": 0.01}


def make_env(game, layout, num_envs, horizon):
    """the kitchen env of ``game`` with episode statistics"""
    if game not in GAMES:
        raise ValueError(f"game must be one of {GAMES}, got {game!r}")
    if game == "simplecooked":
        from madrona_rl_envs_playground_amd.envs.overcooked2_env import OvercookedMadrona
    else:
        from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    return OvercookedMadrona(layout, num_envs, 0, horizon=horizon, record_episode_statistics=True)


def evaluate(env, policy, horizon, seed=0):
    """The notebook's test cell: every world restarts, then plays ``horizon`` steps greedily (``env.act`` + ``env.n_step``, nothing
    waits inside the loop); a world's score is the sum of seat 0's rewards (every seat is paid the same).  Returns {score: number
    of worlds}, ascending."""
    import torch
    env.n_reset(worlds=torch.ones(env.num_envs, dtype=torch.bool, device=env.static_dones.device))
    score = torch.zeros(env.num_envs, dtype=torch.int64, device=env.static_rewards.device)
    for step in range(horizon):
        actions = env.act(policy, seed=seed, step=step, greedy=True)
        env.n_step(actions)  # int32, the simulator's own ACTION tensor: the copy onto itself is what n_step does with it
        score += env.static_rewards[0].view(-1)
    values, counts = torch.unique(score, return_counts=True)  # (the host waits here)
    return {int(v): int(c) for v, c in zip(values.tolist(), counts.tolist())}


def train(layout, num_envs, num_steps, updates, seed, lr=5e-4, critic_lr=5e-4, lr_decay=False, gamma=0.99, gae_lambda=0.95, ppo_epoch=15,
          num_mini_batch=1, clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, horizon=400,
          log=None, game="overcooked", evaluation=None):
    """``updates`` iterations of collect, advantages, update with the reference's defaults (train/config.py).  One dict per
    update: the learning rates, the mean of every stat over the update's rows (``train_info``), the episodes finished during the
    update with their mean return, and ``optimizer_step``.  ``game``: "overcooked" or "simplecooked" (``layout`` is then one of
    Simplecooked's names).  ``evaluation``: a dict that takes ``evaluate``'s histogram under "scores" after the last update."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import (CnnActorCritic, CnnPolicy, MappoOptimizer, ValueNorm, mappo_advantages,
                                                             mappo_update, minibatch_indices)
    env = make_env(game, layout, num_envs, horizon)
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
    if evaluation is not None:
        evaluation["scores"] = evaluate(env, policy, horizon, seed=seed)
    env.close()
    return history


def resolve(args):
    """The settings of a parsed command line: an option given wins, then the recipe's value, then ``DEFAULTS``."""
    recipe = RECIPES[args.recipe] if args.recipe else {}
    return {name: getattr(args, name) if getattr(args, name) is not None else recipe.get(name, default) for name, default in DEFAULTS.items()}


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=GAMES)
    ap.add_argument("--recipe", choices=sorted(RECIPES))
    ap.add_argument("--layout")
    ap.add_argument("--num-envs", type=int)
    ap.add_argument("--num-steps", type=int)
    ap.add_argument("--horizon", type=int)
    ap.add_argument("--updates", type=int)
    ap.add_argument("--ppo-epoch", type=int)
    ap.add_argument("--num-mini-batch", type=int)
    ap.add_argument("--lr", type=float)
    ap.add_argument("--critic-lr", type=float)
    ap.add_argument("--entropy-coef", type=float)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--evaluate", action="store_true", help="afterwards one greedy episode in every world; prints {score: worlds}")
    ap.add_argument("--json", help="also write the settings, the per-update entries and the histogram to this file")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    s = resolve(args)
    evaluation = {} if args.evaluate else None
    history = train(s["layout"], s["num_envs"], s["num_steps"], s["updates"], args.seed, lr=s["lr"], critic_lr=s["critic_lr"],
                    ppo_epoch=s["ppo_epoch"], num_mini_batch=s["num_mini_batch"], entropy_coef=s["entropy_coef"], horizon=s["horizon"],
                    game=s["game"], evaluation=evaluation, log=lambda entry: print(json.dumps(entry), flush=True))
    if evaluation is not None:
        print(json.dumps({"greedy_scores": {str(k): v for k, v in evaluation["scores"].items()}}), flush=True)
    if args.json:
        from madrona_rl_envs_playground_amd import _lib
        out = {"build_hash": _lib.build_hash(), "settings": dict(s, seed=args.seed, recipe=args.recipe), "updates": history,
               "mean_returns": [entry["mean_return"] for entry in history]}
        if evaluation is not None:
            out["greedy_scores"] = {str(k): v for k, v in evaluation["scores"].items()}
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
