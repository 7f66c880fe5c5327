#!/usr/bin/env python3
"""Cross-play between the conventions MAPPO lands on for the balance beam, on the device: one member of an ``MlpBasePolicyBank`` per
seed, each trained in self-play through its view of the bank (``tools/balance_mappo_train_device.py``'s loop: ``env.rollout``,
``mappo_advantages``, ``mappo_update``), then the K x K matrix of ``simulators.cross_play`` -- seat 0 under the row's member, seat 1
under the column's, every pair on its own worlds of ONE simulator, every episode finished within ``--steps`` counted.  What the
reference measures with ``--seed_skip`` and ``--pop_size`` and K x K simulators.

    python tools/balance_cross_play_device.py --seeds 0 1 2 3
    python tools/balance_cross_play_device.py --seeds 0 1 2 3 --updates 20 --json cross.json

The diagonal is self-play.  A seed's run ends on one of the beam's conventions (profiles/balance_mappo_run.json has a run's
histogram), so off-diagonal entries fall where two members' conventions disagree.

Importable: ``run(seeds, updates, ...) -> {"seeds", "mean_return", "episodes", "self_play_training_return"}`` (the last:
each member's mean episode return over its final training update)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import balance_mappo_train_device as trainer  # noqa: E402


def run(seeds, updates, num_envs=1024, num_steps=200, layer_N=2, play_worlds=None, steps=None, greedy=True, log=None):
    """Train one member per seed, then cross-play them.  ``play_worlds``: the worlds of the cross-play batch (default 64 per pair);
    ``steps`` and ``greedy`` are ``cross_play``'s."""
    import torch
    from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic, MlpBasePolicyBank, cross_play
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError("at least one seed")
    device = torch.device("cuda", 0)
    bank = MlpBasePolicyBank(len(seeds), layer_N, device=device)
    self_play = []
    for k, seed in enumerate(seeds):
        torch.manual_seed(seed)
        with torch.no_grad():
            bank.policy(k).params.copy_(torch.nn.utils.parameters_to_vector(MlpBaseActorCritic(layer_N=layer_N).parameters()))
        history = trainer.train(num_envs, num_steps, updates, seed, layer_N=layer_N, policy=bank.policy(k),
                                log=(lambda entry, seed=seed: log(dict(entry, seed=seed))) if log else None)
        self_play.append(history[-1]["mean_return"] if history else None)
    pairs = len(seeds) ** 2
    env = trainer.make_env(pairs * 64 if play_worlds is None else int(play_worlds))
    result = cross_play(env, bank, greedy=greedy, steps=steps)
    out = {"seeds": seeds, "mean_return": result.mean_return.cpu().tolist(), "episodes": result.episodes.cpu().tolist(),
           "self_play_training_return": self_play}
    env.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, nargs="+", required=True, help="one trained member per seed")
    ap.add_argument("--updates", type=int, default=trainer.DEFAULTS["updates"])
    ap.add_argument("--num-envs", type=int, default=trainer.DEFAULTS["num_envs"])
    ap.add_argument("--num-steps", type=int, default=trainer.DEFAULTS["num_steps"])
    ap.add_argument("--layer-N", type=int, default=trainer.DEFAULTS["layer_N"], choices=(1, 2))
    ap.add_argument("--play-worlds", type=int, default=None, help="worlds of the cross-play batch (default 64 per pair)")
    ap.add_argument("--steps", type=int, default=None, help="steps of the cross-play (default cross_play's)")
    ap.add_argument("--sampled", action="store_true", help="members draw their actions instead of taking the arg-max")
    ap.add_argument("--verbose", action="store_true", help="print every update of every member")
    ap.add_argument("--json", help="also write the result to this file")
    args = ap.parse_args(argv)
    out = run(args.seeds, args.updates, args.num_envs, args.num_steps, args.layer_N, args.play_worlds, args.steps, not args.sampled,
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
