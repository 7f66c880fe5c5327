#!/usr/bin/env python3
"""Cross-play between the conventions PPO lands on for Hanabi, on the device: one member of a ``WidePolicyBank`` per seed, each
trained in self-play -- a ``CleanPPOAgent`` that learns the member through its view of the bank (``use_policy(bank.policy(k))``)
against a ``WidePolicyAgent`` that plays the same row, so both seats follow the parameters as they move -- with
``tools/hanabi_train_device.py``'s hyper-parameters, then the K x K matrix of ``simulators.cross_play``: seat 0 under the row's
member, seat 1 under the column's, every pair on its own worlds of ONE simulator, every game finished within ``--steps`` counted.

    python tools/hanabi_cross_play_device.py --config very_small --seeds 0 1 2
    python tools/hanabi_cross_play_device.py --config full --seeds 0 1 2 --updates 200 --steps 400 --json cross.json

The diagonal is self-play; off-diagonal entries fall where two members' conventions disagree.

Importable: ``run(config, seeds, updates, ...) -> {"config", "seeds", "mean_return", "episodes", "self_play_training_return"}``
(the last: each member's mean game return over its final training update, None while no game had finished)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

HP = dict(num_steps=128, lr=6.25e-5, gamma=0.999, clip_coef=0.05)  # scripts/hanabi_train.py's


def train_member(bank, k, seed, config, num_envs, updates, device_update=True, log=None):
    """``updates`` PPO updates of row ``k`` of ``bank`` in self-play; returns the mean return of the games of the last update"""
    import torch
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona, config_choice
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent, WidePolicyAgent
    torch.manual_seed(seed)
    env = HanabiMadrona(num_envs, 0, False, config_choice[config])
    ego = CleanPPOAgent(envs=env, name=f"hanabi_{config}_{seed}", device=torch.device("cuda", 0), num_updates=max(updates, 1), verbose=False,
                        anneal_lr=True, gae_lambda=0.95, num_minibatches=1, update_epochs=4, seed=2 * seed, **HP)
    with torch.no_grad():
        bank.policy(k).params.copy_(ego.policy.params)  # the reference's initialisation under this seed
    ego.device_update = device_update
    ego.use_policy(bank.policy(k))
    env.add_partner_agent(WidePolicyAgent(env, bank.policy(k), seed=2 * seed + 1))
    obs = env.reset()
    seen, last = 1, None
    for _ in range(updates * HP["num_steps"] + (1 if updates else 0)):
        action = ego.get_action(obs)
        if ego.updates != seen:  # an update ran inside get_action
            seen = ego.updates
            if ego.episode_stats["episodes"]:
                last = ego.episode_stats["mean"]
            if log:
                log({"seed": seed, "update": seen - 1, **ego.episode_stats})
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    env.close()
    return last


def run(config, seeds, updates, num_envs=1000, play_worlds=None, steps=200, greedy=True, device_update=True, log=None):
    """Train one member per seed, then cross-play them.  ``play_worlds``: the worlds of the cross-play batch (default 64 per pair);
    ``steps`` and ``greedy`` are ``cross_play``'s."""
    import torch
    from madrona_rl_envs_playground_amd import hanabi_spec
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona, config_choice
    from madrona_rl_envs_playground_amd.simulators import WidePolicyBank, cross_play
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("at least one seed")
    c = config_choice[config]
    bank = WidePolicyBank(hanabi_spec.observation_size(c), hanabi_spec.state_size(c), hanabi_spec.num_moves(c), len(seeds),
                          device=torch.device("cuda", 0))
    self_play = [train_member(bank, k, seed, config, num_envs, updates, device_update, log) for k, seed in enumerate(seeds)]
    env = HanabiMadrona(len(seeds) ** 2 * 64 if play_worlds is None else int(play_worlds), 0, False, c)
    result = cross_play(env, bank, greedy=greedy, steps=steps)
    out = {"config": config, "seeds": seeds, "mean_return": result.mean_return.cpu().tolist(), "episodes": result.episodes.cpu().tolist(),
           "self_play_training_return": self_play}
    env.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", choices=("very_small", "small", "full"), default="very_small", help="Hanabi variant")
    ap.add_argument("--seeds", type=int, nargs="+", required=True, help="one trained member per seed")
    ap.add_argument("--updates", type=int, default=20, help="PPO updates of every member")
    ap.add_argument("--num-envs", type=int, default=1000, help="worlds of a member's training")
    ap.add_argument("--play-worlds", type=int, default=None, help="worlds of the cross-play batch (default 64 per pair)")
    ap.add_argument("--steps", type=int, default=200, help="steps of the cross-play")
    ap.add_argument("--sampled", action="store_true", help="members draw their actions instead of taking the arg-max")
    ap.add_argument("--torch-update", action="store_true", help="run the epochs in torch autograd, not mrl_agent_update")
    ap.add_argument("--verbose", action="store_true", help="print every update of every member")
    ap.add_argument("--json", help="also write the result to this file")
    args = ap.parse_args(argv)
    out = run(args.config, args.seeds, args.updates, args.num_envs, args.play_worlds, args.steps, not args.sampled, not args.torch_update,
              log=(lambda entry: print(json.dumps(entry), flush=True)) if args.verbose else None)
    width = max(8, max(len(str(s)) for s in args.seeds) + 5)
    print("mean return; seat 0: row, seat 1: column")
    print(" " * width + "".join(f"{'seed ' + str(s):>{width}}" for s in args.seeds))
    for seed, row in zip(args.seeds, out["mean_return"]):
        print(f"{'seed ' + str(seed):>{width}}" + "".join(f"{value:>{width}.3f}" for value in row))
    print(json.dumps(out), flush=True)
    if args.json:
        from madrona_rl_envs_playground_amd import _lib
        with open(args.json, "w") as f:
            json.dump(dict(out, build_hash=_lib.build_hash(), updates=args.updates), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
