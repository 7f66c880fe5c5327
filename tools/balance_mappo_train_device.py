#!/usr/bin/env python3
"""The reference's MAPPO loop for the balance beam (train/trainer.py with ``balance``; train/MAPPO/main_player.py, ``MainPlayer.run``,
with the MLP actor-critic, hidden_size 64, ValueNorm) with every phase on the device: per update one ``env.rollout`` (collect), one
``mappo_advantages`` (returns and normalised advantages) and one ``mappo_update`` (ppo_epoch x num_mini_batch actor and critic Adam
steps), then ONE host wait, in which the episode totals and the update's stats come back.  The flat parameter tensor is the only copy
of the weights.

    python tools/balance_mappo_train_device.py --num-envs 1024 --updates 20
    python tools/balance_mappo_train_device.py --evaluate --json run.json
    python tools/balance_mappo_train_device.py --recurrent --data-chunk-length 10

``--recurrent``: the reference's ``--use_recurrent_policy`` -- a GRU between the base and the head of both nets
(``MlpBaseGruPolicy``); the running states are carried from rollout to rollout, the update evaluates chunks of
``--data-chunk-length`` steps from the states the rollout recorded (``chunk_indices``: a permutation of the chunks per epoch, as
``recurrent_generator`` draws it) and back-propagates through them.

The defaults are train/config.py's: ``episode_length`` 200 steps per update, ``ppo_epoch`` 15, one minibatch, lr = critic_lr =
5e-4, ``layer_N`` 2.  ``--evaluate``: greedy episodes in every world, then the histogram of the worlds' returns (an episode is two
steps; +1 per step is the best it can score).

Importable: ``train(num_envs, num_steps, updates, seed) -> list of per-update dicts``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

EPISODE_STEPS = 2  # src/balance_beam_env/sim.cpp: TIME - 1 moves, fewer where a seat leaves the line
DEFAULTS = {"num_envs": 1024, "num_steps": 200, "updates": 20, "ppo_epoch": 15, "num_mini_batch": 1, "lr": 5e-4, "critic_lr": 5e-4,
            "entropy_coef": 0.01, "layer_N": 2}


def make_env(num_envs):
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    return BalanceMadronaTorch(num_envs, 0, record_episode_statistics=True)


def evaluate(env, policy, seed=0):
    """Every world restarts, then plays one episode greedily (``env.act`` + ``env.n_step``, nothing waits inside the loop): two steps,
    or one where a seat walks off the line -- such a world's second step belongs to its next episode and is not counted.  A world's
    return is the sum of seat 0's rewards (both seats are paid the same).  Returns {return: number of worlds}, ascending, the
    returns rounded to six places."""
    import torch
    env.n_reset(worlds=torch.ones(env.num_envs, dtype=torch.bool, device=env.static_dones.device))
    if getattr(policy, "running", None) is not None:
        policy.running.zero_()  # a recurrent policy starts its episodes from zero states
    score = torch.zeros(env.num_envs, dtype=torch.float64, device=env.static_rewards.device)
    playing = torch.ones(env.num_envs, dtype=torch.bool, device=env.static_rewards.device)
    for step in range(EPISODE_STEPS):
        actions = env.act(policy, seed=seed, step=step, greedy=True)
        env.n_step(actions)  # int32, the simulator's own ACTION tensor: the copy onto itself is what n_step does with it
        score += env.static_rewards[0].view(-1).double() * playing
        playing &= env.static_dones.view(-1) == 0
    values, counts = torch.unique(torch.round(score * 1e6) / 1e6, return_counts=True)  # (the host waits here)
    return {round(float(v), 6): int(c) for v, c in zip(values.tolist(), counts.tolist())}


def train(num_envs, num_steps, updates, seed, lr=5e-4, critic_lr=5e-4, lr_decay=False, gamma=0.99, gae_lambda=0.95, ppo_epoch=15,
          num_mini_batch=1, clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, layer_N=2,
          log=None, evaluation=None, final=None, policy=None, recurrent=False, data_chunk_length=10):
    """``updates`` iterations of collect, advantages, update with the reference's defaults (train/config.py).  One dict per
    update: the learning rates, the mean of every stat over the update's rows (``train_info``), the episodes finished during the
    update with their mean return, and ``optimizer_step``.  ``evaluation``: a dict that takes ``evaluate``'s histogram under
    "returns" after the last update.  ``final``: a dict that takes the final parameters (a CPU tensor) under "params".  ``policy``: an
    ``MlpBasePolicy`` of ``layer_N`` to train in place from the parameters it holds -- a member of an ``MlpBasePolicyBank``, say --
    instead of a fresh one initialised under ``seed``.  ``recurrent``: train an ``MlpBaseGruPolicy`` over chunks of
    ``data_chunk_length`` steps, which must divide ``num_steps``."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import (MappoOptimizer, MlpBaseActorCritic, MlpBaseGruActorCritic, MlpBaseGruPolicy,
                                                             MlpBaseGruRecord, MlpBasePolicy, ValueNorm, chunk_indices, mappo_advantages,
                                                             mappo_update, minibatch_indices)
    env = make_env(num_envs)
    device = torch.device("cuda", 0)
    players = env.n_players
    if policy is None:
        torch.manual_seed(seed)
        if recurrent:
            policy = MlpBaseGruPolicy.from_module(MlpBaseGruActorCritic(layer_N=layer_N), device=device)
        else:
            policy = MlpBasePolicy.from_module(MlpBaseActorCritic(layer_N=layer_N), device=device)
    elif policy.layer_N != layer_N or isinstance(policy, MlpBaseGruPolicy) != bool(recurrent):
        raise ValueError(f"the policy has layer_N {policy.layer_N}, asked for {layer_N}; recurrent {bool(recurrent)} needs an "
                         f"{'MlpBaseGruPolicy' if recurrent else 'MlpBasePolicy'}")
    optimizer = MappoOptimizer(policy, lr=lr, critic_lr=critic_lr)
    value_norm = ValueNorm(device)
    shuffles = torch.Generator(device=device).manual_seed(seed)
    rows = ppo_epoch * num_mini_batch
    host_stats = torch.empty((rows, len(_lib.MAPPO_STATS)), dtype=torch.float32).pin_memory()
    record, history = None, []
    if recurrent:
        policy.state(num_envs)
        record = MlpBaseGruRecord(num_steps, num_envs, players, device, chunk_length=data_chunk_length)
    for update in range(updates):
        if lr_decay:  # utils/util.py:38-43
            optimizer.lr, optimizer.critic_lr = lr - lr * (update / updates), critic_lr - critic_lr * (update / updates)
        env.clear_episode_totals()
        record = env.rollout(policy, num_steps, seed=seed, first_step=update * num_steps, record=record)
        advantages, returns = mappo_advantages(record, value_norm, gamma, gae_lambda)
        if recurrent:
            indices = chunk_indices(record, num_mini_batch, ppo_epoch, generator=shuffles, device=device)
        else:
            indices = minibatch_indices(num_steps * num_envs * players, num_mini_batch, ppo_epoch, generator=shuffles, device=device)
        result = mappo_update(policy, optimizer, record, None, advantages, returns, indices, value_norm=value_norm, clip_param=clip_param,
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
        evaluation["returns"] = evaluate(env, policy, seed=seed)
    if final is not None:
        final["params"] = policy.params.cpu()
    env.close()
    return history


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, default=DEFAULTS["num_envs"])
    ap.add_argument("--num-steps", type=int, default=DEFAULTS["num_steps"])
    ap.add_argument("--updates", type=int, default=DEFAULTS["updates"])
    ap.add_argument("--ppo-epoch", type=int, default=DEFAULTS["ppo_epoch"])
    ap.add_argument("--num-mini-batch", type=int, default=DEFAULTS["num_mini_batch"])
    ap.add_argument("--lr", type=float, default=DEFAULTS["lr"])
    ap.add_argument("--critic-lr", type=float, default=DEFAULTS["critic_lr"])
    ap.add_argument("--entropy-coef", type=float, default=DEFAULTS["entropy_coef"])
    ap.add_argument("--layer-N", type=int, default=DEFAULTS["layer_N"], choices=(1, 2))
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--recurrent", action="store_true", help="the recurrent actor-critic (the reference's --use_recurrent_policy)")
    ap.add_argument("--data-chunk-length", type=int, default=10, help="steps per chunk of the recurrent update (the reference's default)")
    ap.add_argument("--evaluate", action="store_true", help="afterwards one greedy episode in every world; prints {return: worlds}")
    ap.add_argument("--json", help="also write the settings, the per-update entries and the histogram to this file")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    evaluation = {} if args.evaluate else None
    history = train(args.num_envs, args.num_steps, args.updates, args.seed, lr=args.lr, critic_lr=args.critic_lr, ppo_epoch=args.ppo_epoch,
                    num_mini_batch=args.num_mini_batch, entropy_coef=args.entropy_coef, layer_N=args.layer_N, evaluation=evaluation,
                    recurrent=args.recurrent, data_chunk_length=args.data_chunk_length, log=lambda entry: print(json.dumps(entry), flush=True))
    if evaluation is not None:
        print(json.dumps({"greedy_returns": {str(k): v for k, v in evaluation["returns"].items()}}), flush=True)
    if args.json:
        from madrona_rl_envs_playground_amd import _lib
        settings = {name: getattr(args, name) for name in ("num_envs", "num_steps", "updates", "ppo_epoch", "num_mini_batch", "lr",
                                                           "critic_lr", "entropy_coef", "layer_N", "seed", "recurrent",
                                                           "data_chunk_length")}
        out = {"build_hash": _lib.build_hash(), "settings": settings, "updates": history,
               "mean_returns": [entry["mean_return"] for entry in history]}
        if evaluation is not None:
            out["greedy_returns"] = {str(k): v for k, v in evaluation["returns"].items()}
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
