#!/usr/bin/env python3
"""Cross-play on the device: K policies in one ``CnnPolicyBank``, the K x K matrix of their pairings from ONE batch of worlds
(``simulators.cross_play``: world n plays pair n mod K^2, one horizon of bank acts and steps, no host wait inside), and, on
request, an ego trained against the K of them as frozen partners.

    python tools/cross_play_device.py --layout cramped_room --seeds 0 1 2 3 --num-envs 1024
    python tools/cross_play_device.py --checkpoints a.pt b.pt c.pt --train-ego 20

``--seeds``: the reference's initialisation under each seed.  ``--checkpoints``: files ``torch.save`` wrote, each either a flat
parameter tensor of ``CnnPolicy.num_params`` floats or a dict with the reference's two state dicts under "actor" and "critic".
``--train-ego U``: row K of the bank starts as a copy of row 0 and takes U updates; in each, every world's seat 0 plays the ego and
its seat 1 a partner out of rows 0..K-1, drawn again at random whenever the world's episode ends (``env.rollout_bank`` with a
``CnnResample``), the advantages are normalised over the ego's column alone (``mappo_advantages(seats=[0])``) and ``mappo_update``
runs on the ego's samples only.  Afterwards the ego's row of the matrix (ego on seat 0 against every partner) is printed too.
The numbers are printed and recorded, never asserted.

Importable: ``build_bank``, ``matrix``, ``train_ego``."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def build_bank(env, seeds=None, checkpoints=None, spare=0):
    """A bank of the env's shape: one member per checkpoint or per seed, then ``spare`` rows of zeros"""
    import torch
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnPolicyBank
    device = env.static_actions.device
    _, _, height, width, channels = env.static_world_major_observations.shape
    members = []
    for path in checkpoints or []:
        blob = torch.load(path, map_location="cpu")
        if isinstance(blob, dict):
            module = CnnActorCritic(width, height, channels)
            module.actor.load_state_dict(blob["actor"])
            module.critic.load_state_dict(blob["critic"])
            members.append(CnnPolicy.from_module(module, device=device))
        else:
            policy = CnnPolicy(width, height, channels, device=device)
            policy.params.copy_(torch.as_tensor(blob, dtype=torch.float32).reshape(-1))
            members.append(policy)
    for seed in seeds or []:
        torch.manual_seed(seed)
        members.append(CnnPolicy.from_module(CnnActorCritic(width, height, channels), device=device))
    if not members:
        raise ValueError("give --seeds or --checkpoints")
    bank = CnnPolicyBank(width, height, channels, len(members) + spare, device=device)
    for k, member in enumerate(members):
        bank.params[k].copy_(member.params)
    return bank, len(members)


def matrix(env, bank, members_a=None, members_b=None, seed=0):
    """``cross_play`` as nested lists (the one host wait)"""
    from madrona_rl_envs_playground_amd.simulators import cross_play
    result = cross_play(env, bank, members_a, members_b, greedy=True, seed=seed)
    return {"mean_return": result.mean_return.cpu().tolist(), "worlds_per_pair": result.episodes.cpu().tolist()}


def train_ego(env, bank, partners, updates, num_steps=128, seed=1, lr=5e-4, ppo_epoch=15, num_mini_batch=1, log=None):
    """``updates`` updates of row ``partners`` (the ego, seat 0) against rows 0..partners-1 on seat 1; one dict per update"""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import CnnResample, MappoOptimizer, ValueNorm, mappo_advantages, mappo_update, minibatch_indices
    device = env.static_actions.device
    n = env.num_envs
    ego = bank.policy(partners)
    optimizer, value_norm = MappoOptimizer(ego, lr=lr, critic_lr=lr), ValueNorm(device)
    ids = torch.stack([torch.full((n,), partners), torch.arange(n) % partners], dim=1).to(torch.int32).to(device).contiguous()
    episodes = torch.zeros(n, dtype=torch.int32, device=device)
    resample = CnnResample("random", [partners, 0], [1, partners], 2, seed=seed)  # the ego stays, the partner is drawn again
    shuffles = torch.Generator(device=device).manual_seed(seed)
    ego_samples = torch.arange(num_steps * n, device=device, dtype=torch.int32) * 2  # (t N + n) P + 0
    record = ring = ids_record = None
    history = []
    for update in range(updates):
        env.clear_episode_totals()
        record, ring, ids_record = env.rollout_bank(bank, ids, num_steps, episodes=episodes, resample=resample, seed=seed,
                                                    first_step=update * num_steps, record=record, ring=ring, ids_record=ids_record)
        advantages, returns = mappo_advantages(record, value_norm, seats=[0])
        indices = ego_samples[minibatch_indices(num_steps * n, num_mini_batch, ppo_epoch, generator=shuffles, device=device).long()].contiguous()
        result = mappo_update(ego, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm)
        stats = result.stats.mean(dim=0).cpu()  # the update's one host wait
        totals = env.episode_totals()
        entry = {"update": update, "episodes": totals["episodes"],
                 "mean_return": totals["returns"][0] / totals["episodes"] if totals["episodes"] else None}
        entry.update({name: float(stats[column]) for column, name in enumerate(_lib.MAPPO_STATS[:7])})
        history.append(entry)
        if log:
            log(entry)
    return history


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layout", default="cramped_room")
    ap.add_argument("--num-envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=400)
    ap.add_argument("--seeds", type=int, nargs="*")
    ap.add_argument("--checkpoints", nargs="*")
    ap.add_argument("--train-ego", type=int, default=0, metavar="U")
    ap.add_argument("--num-steps", type=int, default=128)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", help="a JSON file for everything printed")
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    env = OvercookedMadrona(args.layout, args.num_envs, 0, horizon=args.horizon, record_episode_statistics=True)
    bank, k = build_bank(env, args.seeds, args.checkpoints, spare=1 if args.train_ego else 0)
    members = list(range(k))
    report = {"layout": args.layout, "worlds": args.num_envs, "horizon": args.horizon, "policies": k,
              "cross_play": matrix(env, bank, members, members, seed=args.seed)}
    print(json.dumps({"cross_play": report["cross_play"]}), flush=True)
    if args.train_ego:
        bank.params[k].copy_(bank.params[0])
        report["ego_updates"] = train_ego(env, bank, k, args.train_ego, num_steps=args.num_steps, seed=args.seed,
                                          log=lambda entry: print(json.dumps(entry), flush=True))
        report["ego_against_partners"] = matrix(env, bank, [k], members, seed=args.seed)
        print(json.dumps({"ego_against_partners": report["ego_against_partners"]}), flush=True)
    env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
