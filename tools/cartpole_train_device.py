#!/usr/bin/env python3
"""The reference's PPO trainers for the small tanh actor-critic (scripts/cartpole_train_torch.py, and with ``--game balance``
scripts/balance_train_single.py) with every phase on the device: per update one ``env.rollout`` (collect), one ``gae``
(advantages) and one ``ppo_update`` (E x M Adam steps), then ONE host wait, in which the episode totals and the update's stats
come back.  The flat parameter tensor is the only copy of the weights.

    python tools/cartpole_train_device.py --game cartpole --num-envs 1024 --updates 50
    python tools/cartpole_train_device.py --game balance          (that script's defaults: 4 worlds, 1000 steps, 125 updates)

``--game balance`` trains seat 0 of the balance beam through ``BalanceGym`` against a uniformly random partner and prints
``avg_score``, the mean return of the episodes finished during the update, as that script does.

    python tools/cartpole_train_device.py --game acrobot --seeds 1 2 3 4      (four seeds of --num-envs worlds each on one batch)

``--seeds`` trains K seeds at once, for every ``--game``: ONE simulator of K x ``--num-envs`` worlds, member k on worlds
``[k W, (k + 1) W)``, the same loop on ``env.rollout_bank``, ``gae`` and ``ppo_update_bank`` -- the launches of one seed's update
whatever K is, and still one host wait per update.  Member k is initialised and shuffled from seed k.  It prints, per update and
member, the mean return of the episodes its worlds finished last.

Importable: ``train(num_envs, num_steps, updates, seed) -> list of per-update dicts``; ``train_bank(num_envs, num_steps, updates,
seeds)`` likewise with per-member lists."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

# per game: --num-envs, --num-steps, --updates of the reference's script (balance: total_timesteps 500000 // (4 * 1000))
DEFAULTS = {"cartpole": (1024, 128, 50), "acrobot": (1024, 128, 50), "balance": (4, 1000, 125)}


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


def make_env(game, num_envs):
    from madrona_rl_envs_playground_amd.envs.acrobot_env import AcrobotMadronaTorch
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceGym
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    if game == "cartpole":
        return CartpoleMadronaTorch(num_envs, 0, record_episode_statistics=True)
    if game == "acrobot":
        return AcrobotMadronaTorch(num_envs, 0, record_episode_statistics=True)
    if game == "balance":
        return BalanceGym(num_envs, 0, False, record_episode_statistics=True)
    raise ValueError(f"game must be 'cartpole', 'acrobot' or 'balance', got {game!r}")


def train_bank(num_envs, num_steps, updates, seeds, game="cartpole", learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
               num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01, vf_coef=0.5,
               max_grad_norm=0.5, log=None):
    """``train`` for K = ``len(seeds)`` seeds on one simulator of K x ``num_envs`` worlds.  One dict per update: the learning rate,
    ``optimizer_step``, and per member (lists of K, member k the seed ``seeds[k]``) the mean of every stat over the update's rows,
    ``mean_return`` -- the mean of the last finished episode's return over the member's worlds that have finished one, reduced on
    the device from a (K, W) view of the episode statistics -- and ``worlds_finished``, how many worlds that is."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import MlpPolicyBank, PpoBankOptimizer, gae, member_minibatch_indices, ppo_update_bank
    members, total = len(seeds), len(seeds) * num_envs
    env = make_env(game, total)
    device = torch.device("cuda", 0)
    obs_dim, observation = (7, "beam") if game == "balance" else (4, "state")
    bank = MlpPolicyBank.from_modules([make_agent(obs_dim, env.single_action_space.n, seed) for seed in seeds], observation=observation,
                                      device=device)
    optimizer = PpoBankOptimizer(bank, lr=learning_rate)
    shuffles = [torch.Generator(device=device).manual_seed(seed) for seed in seeds]
    rows, columns = update_epochs * num_minibatches, len(_lib.PPO_STATS)
    # the episode statistics as (K, W): the ego's return of the episode a world finished last, and that episode's length (0: none yet)
    last_return = env.episode_stats.last_return.reshape(-1)[:total].view(members, num_envs)
    last_steps = env.episode_stats.last_steps.reshape(-1)[:total].view(members, num_envs)
    host = torch.empty((members, columns + 2), dtype=torch.float32).pin_memory()  # the stats' means, mean_return, worlds_finished
    rollout, history = None, []
    for update in range(updates):
        if anneal_lr:
            optimizer.lr = (1.0 - update / updates) * learning_rate
        rollout = env.rollout_bank(bank, num_steps, seed=seeds[0], first_step=update * num_steps, out=rollout)
        advantages, returns = gae(rollout, gamma, gae_lambda)
        indices = member_minibatch_indices(num_steps, total, members, num_minibatches, update_epochs, generator=shuffles, device=device)
        result = ppo_update_bank(bank, optimizer, rollout, advantages, returns, indices, clip_coef=clip_coef, ent_coef=ent_coef,
                                 vf_coef=vf_coef, max_grad_norm=max_grad_norm, norm_adv=norm_adv, clip_vloss=clip_vloss)
        finished = last_steps > 0
        count = finished.sum(dim=1)
        mean_return = torch.where(finished, last_return, torch.zeros_like(last_return)).sum(dim=1) / count.clamp(min=1)
        host.copy_(torch.cat([result.stats.mean(dim=1), mean_return.view(members, 1), count.view(members, 1).float()], dim=1), non_blocking=True)
        torch.cuda.current_stream().synchronize()  # the update's one host wait
        entry = {"update": update, "lr": optimizer.lr, "optimizer_step": optimizer.step, "seeds": list(seeds),
                 "global_step": (update + 1) * num_steps * total,
                 "worlds_finished": [int(v) for v in host[:, columns + 1]],
                 "mean_return": [float(v) if n else None for v, n in zip(host[:, columns], host[:, columns + 1])]}
        for column, name in enumerate(_lib.PPO_STATS):
            entry[name] = [float(v) for v in host[:, column]]
        history.append(entry)
        if log:
            log(entry)
    env.close()
    return history


def train(num_envs, num_steps, updates, seed, game="cartpole", learning_rate=2.5e-4, anneal_lr=True, gamma=0.99, gae_lambda=0.95,
          num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01, vf_coef=0.5,
          max_grad_norm=0.5, log=None):
    """``updates`` iterations of collect, advantages, update.  One dict per update: the learning rate, the mean of every stat
    over the update's E x M rows and the last row's, the episodes finished during the update with their mean return (also as
    ``avg_score``, the name scripts/balance_train_single.py prints it under), and ``optimizer_step``, the Adam steps taken so
    far."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import MlpPolicy, PpoOptimizer, gae, minibatch_indices, ppo_update
    env = make_env(game, num_envs)
    device = torch.device("cuda", 0)
    obs_dim, observation = (7, "beam") if game == "balance" else (4, "state")
    policy = MlpPolicy.from_module(make_agent(obs_dim, env.single_action_space.n, seed), observation=observation, device=device)
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
        mean_return = totals["returns"][0] / episodes if episodes else None
        entry = {"update": update, "lr": optimizer.lr, "optimizer_step": optimizer.step, "episodes": episodes,
                 "mean_return": mean_return, "avg_score": mean_return, "global_step": (update + 1) * num_steps * num_envs}
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
    ap.add_argument("--game", choices=sorted(DEFAULTS), default="cartpole")
    ap.add_argument("--num-envs", type=int, default=None, help="default: 1024, for balance the script's 4")
    ap.add_argument("--num-steps", type=int, default=None, help="default: 128, for balance the script's 1000")
    ap.add_argument("--updates", type=int, default=None, help="default: 50, for balance the script's 500000 // (4 * 1000) = 125")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--seeds", type=int, nargs="+", default=None,
                    help="train these seeds at once as the members of one bank, --num-envs worlds each (in place of --seed)")
    ap.add_argument("--scores-out", default=None, help="write avg_score per update to this JSON file")
    args = ap.parse_args()
    num_envs, num_steps, updates = (given if given is not None else default
                                    for given, default in zip((args.num_envs, args.num_steps, args.updates), DEFAULTS[args.game]))
    if args.seeds:
        history = train_bank(num_envs, num_steps, updates, args.seeds, game=args.game, log=lambda entry: print(json.dumps(entry), flush=True))
        if args.scores_out:
            from madrona_rl_envs_playground_amd import _lib
            record = {"build_hash": _lib.build_hash(), "game": args.game, "num_envs": num_envs, "num_steps": num_steps, "updates": updates,
                      "seeds": args.seeds, "mean_return": [entry["mean_return"] for entry in history],
                      "worlds_finished": [entry["worlds_finished"] for entry in history]}
            os.makedirs(os.path.dirname(os.path.abspath(args.scores_out)), exist_ok=True)
            with open(args.scores_out, "w") as f:
                json.dump(record, f, indent=1, sort_keys=True)
                f.write("\n")
        return
    history = train(num_envs, num_steps, updates, args.seed, game=args.game, log=lambda entry: print(json.dumps(entry), flush=True))
    if args.scores_out:
        from madrona_rl_envs_playground_amd import _lib
        record = {"build_hash": _lib.build_hash(), "game": args.game, "num_envs": num_envs, "num_steps": num_steps, "updates": updates,
                  "seed": args.seed, "avg_score": [entry["avg_score"] for entry in history],
                  "episodes": [entry["episodes"] for entry in history]}
        os.makedirs(os.path.dirname(os.path.abspath(args.scores_out)), exist_ok=True)
        with open(args.scores_out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
