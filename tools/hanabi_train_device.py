#!/usr/bin/env python3
"""The loop of the reference's scripts/hanabi_train.py and scripts/balance_train.py -- two ``CleanPPOAgent``s, ego and partner,
around ``env.step`` -- on this engine's calls: every ``get_action`` is ``mrl_agent_act`` on the simulator's tensors, every
``update`` is ``mrl_agent_credit``, the advantages at an update boundary are ``mrl_gae_active``; the learning phase is torch's,
or with ``--device-update`` ``mrl_agent_update``.

    python tools/hanabi_train_device.py --game hanabi --config very_small --num-updates 20
    python tools/hanabi_train_device.py --game balance --device-update

Hyper-parameter defaults are the two scripts' own (Hanabi: 1000 worlds, T = 128, lr 6.25e-5, gamma 0.999, clip 0.05; balance
beam: 120 worlds, T = 60, lr 2.5e-4, gamma 0.99, clip 0.2; one minibatch, four epochs).  Prints one line per update: episodes
finished, their mean / min / max return (read once per update from the device totals), losses and steps per second."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEFAULTS = {"hanabi": dict(num_envs=1000, num_steps=128, lr=6.25e-5, gamma=0.999, clip_coef=0.05),
            "balance": dict(num_envs=120, num_steps=60, lr=2.5e-4, gamma=0.99, clip_coef=0.2)}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--game", choices=("hanabi", "balance"), default="hanabi")
    parser.add_argument("--config", choices=("very_small", "small", "full"), default="full", help="Hanabi variant")
    parser.add_argument("--num-updates", type=int, default=1000)
    parser.add_argument("--num-envs", type=int)
    parser.add_argument("--num-steps", type=int)
    parser.add_argument("--learning-rate", type=float)
    parser.add_argument("--seed", type=int, default=1)
    parser.add_argument("--device-update", action="store_true", help="run the epochs on the device (mrl_agent_update), not in torch")
    parser.add_argument("--tensorboard", action="store_true", help="log to runs/ (if tensorboard is importable)")
    args = parser.parse_args()

    import torch

    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona, config_choice
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent

    hp = dict(DEFAULTS[args.game])
    for key, value in (("num_envs", args.num_envs), ("num_steps", args.num_steps), ("lr", args.learning_rate)):
        if value is not None:
            hp[key] = value
    num_envs = hp.pop("num_envs")
    torch.manual_seed(args.seed)
    env = HanabiMadrona(num_envs, 0, False, config_choice[args.config]) if args.game == "hanabi" else BalanceMadronaTorch(num_envs, 0)
    device = torch.device("cuda", 0)
    name = f"{args.game}_{args.config if args.game == 'hanabi' else 'beam'}_{args.seed}"
    common = dict(device=device, num_updates=args.num_updates, verbose=args.tensorboard, anneal_lr=True, gae_lambda=0.95,
                  num_minibatches=1, update_epochs=4, **hp)
    ego = CleanPPOAgent(envs=env, name=name + "_ego", seed=2 * args.seed, **common)
    partner = CleanPPOAgent(envs=env.getDummyEnv(1), name=name + "_partner", seed=2 * args.seed + 1, **common)
    ego.device_update = partner.device_update = args.device_update
    env.add_partner_agent(partner)

    obs = env.reset()
    start, seen = time.time(), 1
    for _ in range(args.num_updates * hp["num_steps"] + 1):
        action = ego.get_action(obs)
        if ego.updates != seen:  # an update ran inside get_action
            seen = ego.updates
            stats, losses = ego.episode_stats, ego.last_losses
            print(f"update {seen - 1}: episodes {stats['episodes']} return mean {stats['mean']:.3f} min {stats['min']:.3f} max "
                  f"{stats['max']:.3f} | v_loss {losses['value_loss']:.4f} pg_loss {losses['policy_loss']:.4f} entropy "
                  f"{losses['entropy']:.3f} kl {losses['approx_kl']:.5f} | {int(ego.global_step * num_envs / (time.time() - start))} "
                  "world-steps/s", flush=True)
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    env.close()


if __name__ == "__main__":
    main()
