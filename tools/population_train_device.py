#!/usr/bin/env python3
"""Train a population in self-play on ONE batch of worlds, on the device: K members of a ``CnnPolicyBank`` (the kitchens) or an
``MlpBasePolicyBank`` (the balance beam), one per seed; both seats of world n are played by member n mod K for the whole run (no
resample).  Per update: ONE ``env.rollout_bank``, ONE ``mappo_advantages_bank`` and ONE ``mappo_update_bank`` over every epoch and
minibatch row -- 2 + 3 R launches for the whole population -- then one host wait for the update's numbers.  Afterwards the K x K
matrix of ``simulators.cross_play``.

    python tools/population_train_device.py --game balance --seeds 0 1 2 3 --num-envs 1024 --updates 20
    python tools/population_train_device.py --game overcooked --layout cramped_room --seeds 0 1 2 3 --updates 20 --json run.json
    python tools/population_train_device.py --game simplecooked --layout simple --seeds 0 1 --num-envs 800 --updates 50

A member's mean return of an update is the mean, over its worlds that have finished an episode, of the return of the world's most
recent finished episode (the episode statistics' last-return tensor, as seat 0 was paid), read with torch ops behind the update.
The numbers are printed and recorded, never asserted.

Importable: ``train(game, seeds, num_envs, num_steps, updates, ...) -> (bank, history)`` and ``run(...)``, which adds the matrix."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

GAMES = ("overcooked", "simplecooked", "balance")
DEFAULT_LAYOUT = {"overcooked": "cramped_room", "simplecooked": "simple"}


def make_env(game, num_envs, layout=None, horizon=400):
    """the env of ``game`` with episode statistics"""
    if game not in GAMES:
        raise ValueError(f"game must be one of {GAMES}, got {game!r}")
    if game == "balance":
        import balance_mappo_train_device
        return balance_mappo_train_device.make_env(num_envs)
    import overcooked_train_device
    return overcooked_train_device.make_env(game, layout or DEFAULT_LAYOUT[game], num_envs, horizon)


def make_bank(game, env, seeds, layer_N=2):
    """a bank of the env's shape: member k is the reference's initialisation under ``seeds[k]``"""
    import torch
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicyBank, MlpBaseActorCritic, MlpBasePolicyBank
    device = env.static_actions.device
    if game == "balance":
        bank, module = MlpBasePolicyBank(len(seeds), layer_N, device=device), lambda: MlpBaseActorCritic(layer_N=layer_N)
    else:
        _, _, height, width, channels = env.static_world_major_observations.shape
        bank, module = CnnPolicyBank(width, height, channels, len(seeds), device=device), lambda: CnnActorCritic(width, height, channels)
    with torch.no_grad():
        for k, seed in enumerate(seeds):
            torch.manual_seed(seed)
            bank.params[k].copy_(torch.nn.utils.parameters_to_vector(module().parameters()))
    return bank


def member_rows(cells, epochs, num_mini_batch, generator):
    """``minibatch_indices`` per member -> int32 (K, epochs * num_mini_batch, S // num_mini_batch): every epoch is one permutation of
    the member's own samples (``cells`` (K, S)) cut into rows; no host wait"""
    import torch
    members, samples = cells.shape
    width = samples // num_mini_batch
    order = torch.rand((members, epochs, samples), generator=generator, device=cells.device).argsort(dim=2)
    rows = cells.view(members, 1, samples).expand(members, epochs, samples).gather(2, order)[:, :, :width * num_mini_batch]
    return rows.reshape(members, epochs * num_mini_batch, width).contiguous()


def train(game, seeds, num_envs, num_steps, updates, layout=None, horizon=400, layer_N=2, lr=5e-4, critic_lr=5e-4, gamma=0.99, gae_lambda=0.95,
          ppo_epoch=15, num_mini_batch=1, clip_param=0.2, entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0,
          seed=0, log=None, bank=None):
    """``updates`` iterations of one bank rollout, one ``mappo_advantages_bank`` and one ``mappo_update_bank`` -> (bank, history).
    One dict per update: per member the mean return (None before its first finished episode), the worlds it was taken over and
    the mean of every stat over the update's rows.  ``bank``: train these members in place instead of fresh ones."""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import (MappoBankOptimizer, ValueNormBank, mappo_advantages_bank, mappo_update_bank,
                                                             member_samples)
    seeds = [int(s) for s in seeds]
    k = len(seeds)
    if k == 0 or num_envs % k:
        raise ValueError(f"{num_envs} worlds do not split evenly over {k} members")
    env = make_env(game, num_envs, layout, horizon)
    device = env.static_actions.device
    bank = make_bank(game, env, seeds, layer_N) if bank is None else bank
    players = 2 if game == "balance" else env.num_players
    world_owner = torch.arange(num_envs, device=device) % k
    owner = world_owner.view(num_envs, 1).expand(num_envs, players).to(torch.int32).contiguous()
    cells = member_samples(owner, range(k), num_steps)  # the one look at the owners on the host
    optimizer = MappoBankOptimizer(bank, lr=lr, critic_lr=critic_lr)
    value_norms = ValueNormBank(k, device)
    shuffles = torch.Generator(device=device).manual_seed(seed)
    own_worlds = (world_owner.view(1, num_envs) == torch.arange(k, device=device).view(k, 1)).to(torch.float64)  # (K, N)
    last_return = env.sim.last_episode_return_tensor().to_torch()
    last_steps = env.sim.last_episode_steps_tensor().to_torch()
    columns = len(_lib.MAPPO_STATS)
    record = ring = ids_record = None
    history = []
    for update in range(updates):
        if game == "balance":
            record, ids_record = env.rollout_bank(bank, owner, num_steps, seed=seed, first_step=update * num_steps, record=record,
                                                  ids_record=ids_record)
        else:
            record, ring, ids_record = env.rollout_bank(bank, owner, num_steps, seed=seed, first_step=update * num_steps, record=record,
                                                        ring=ring, ids_record=ids_record)
        advantages, returns = mappo_advantages_bank(record, cells, value_norms, gamma, gae_lambda)
        indices = member_rows(cells, ppo_epoch, num_mini_batch, shuffles)
        result = mappo_update_bank(bank, optimizer, record, ring, advantages, returns, indices, value_norms, clip_param=clip_param,
                                   entropy_coef=entropy_coef, value_loss_coef=value_loss_coef, max_grad_norm=max_grad_norm,
                                   huber_delta=huber_delta)
        finished = (last_steps.reshape(-1)[:num_envs] > 0).to(torch.float64) * own_worlds  # (K, N)
        sums = (finished * last_return.reshape(players, num_envs)[0].to(torch.float64)).sum(dim=1)
        packed = torch.cat([sums, finished.sum(dim=1), result.stats.to(torch.float64).mean(dim=1).reshape(-1)]).cpu()  # the update's one host wait
        sums, worlds, stats = packed[:k].tolist(), packed[k:2 * k].tolist(), packed[2 * k:].view(k, columns).tolist()
        entry = {"update": update, "optimizer_step": optimizer.step, "global_step": (update + 1) * num_steps * num_envs,
                 "mean_return": [s / w if w else None for s, w in zip(sums, worlds)], "worlds": [int(w) for w in worlds]}
        for column, name in enumerate(_lib.MAPPO_STATS[:7]):
            entry[name] = [row[column] for row in stats]
        history.append(entry)
        if log:
            log(entry)
    env.close()
    return bank, history


def run(game, seeds, num_envs, num_steps, updates, play_worlds=None, log=None, **options):
    """``train``, then the members' cross-play matrix (greedy) on a fresh env of ``play_worlds`` worlds (default 64 per pair)"""
    from madrona_rl_envs_playground_amd.simulators import cross_play
    bank, history = train(game, seeds, num_envs, num_steps, updates, log=log, **options)
    pairs = len(bank) ** 2
    env = make_env(game, pairs * 64 if play_worlds is None else int(play_worlds), options.get("layout"), options.get("horizon", 400))
    result = cross_play(env, bank, greedy=True)
    out = {"game": game, "seeds": [int(s) for s in seeds], "history": history, "mean_return": result.mean_return.cpu().tolist(),
           "episodes": result.episodes.cpu().tolist()}
    env.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=GAMES, required=True)
    ap.add_argument("--layout", default=None, help="the kitchen's layout (default cramped_room / simple)")
    ap.add_argument("--seeds", type=int, nargs="+", required=True, help="one member per seed")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--num-steps", type=int, default=None, help="steps per rollout (default 200 on the beam, 128 in a kitchen)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=400, help="a kitchen's episode length")
    ap.add_argument("--layer-N", type=int, default=2, choices=(1, 2), help="the beam's MLP")
    ap.add_argument("--ppo-epoch", type=int, default=15)
    ap.add_argument("--num-mini-batch", type=int, default=1)
    ap.add_argument("--lr", type=float, default=5e-4)
    ap.add_argument("--critic-lr", type=float, default=5e-4)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
    ap.add_argument("--play-worlds", type=int, default=None, help="worlds of the cross-play batch (default 64 per pair)")
    ap.add_argument("--json", help="also write the result to this file")
    args = ap.parse_args(argv)
    steps = args.num_steps if args.num_steps is not None else (200 if args.game == "balance" else 128)

    def show(entry):
        returns = " ".join("   none" if r is None else f"{r:7.3f}" for r in entry["mean_return"])
        print(f"update {entry['update']:3d}  mean return per member: {returns}", flush=True)

    out = run(args.game, args.seeds, args.num_envs, steps, args.updates, play_worlds=args.play_worlds, log=show, layout=args.layout,
              horizon=args.horizon, layer_N=args.layer_N, lr=args.lr, critic_lr=args.critic_lr, ppo_epoch=args.ppo_epoch,
              num_mini_batch=args.num_mini_batch, entropy_coef=args.entropy_coef)
    width = max(8, max(len(str(s)) for s in args.seeds) + 5)
    print("cross-play, mean return; seat 0: row, seat 1: column")
    print(" " * width + "".join(f"{'seed ' + str(s):>{width}}" for s in args.seeds))
    for seed, row in zip(args.seeds, out["mean_return"]):
        print(f"{'seed ' + str(seed):>{width}}" + "".join(f"{value:>{width}.3f}" for value in row))
    print(json.dumps({key: out[key] for key in ("game", "seeds", "mean_return", "episodes")}), flush=True)
    if args.json:
        from madrona_rl_envs_playground_amd import _lib
        with open(args.json, "w") as f:
            json.dump(dict(out, build_hash=_lib.build_hash(), updates=args.updates), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
