#!/usr/bin/env python3
"""What the recurrent CNN actor-critic of the kitchens costs -> profiles/cnn_gru_cost.json.

  iteration   a rollout of T = 200, the advantages and 7 epochs of one minibatch over all chunks at L = 10, on the device
              (``env.rollout``, ``mappo_advantages``, ``mappo_update``) against the torch loop of the same recurrent modules on the
              same simulator (one act per step through ``CnnGruActorCritic``, autograd through the chunks, two ``torch.optim.Adam``;
              no ValueNorm on the torch side): Simplecooked ``simple`` at 800 worlds and ``cramped_room`` at 1024.
  plain       a plain ``CnnPolicy``'s rollout of 200 steps and ``mappo_update`` of 7 epochs at 1024 worlds, this build against
              a built tree of the parent commit (``--parent-tree``), a window per process, processes alternating.

Medians of ``--windows`` alternating windows with min and max, and the build id.

    python tools/cnn_gru_probe.py --parent-tree build_parent"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MRL_PROBE_TREE") or REPO)  # (a plain window of another build runs that build's own tree)

T, L, EPOCHS = 200, 10, 7
SHAPES = (("simplecooked", "simple", 800), ("overcooked", "cramped_room", 1024))


def timed(fn):
    import torch
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e3


def summary(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "windows": list(samples)}


def device_iteration(env, policy, optimizer, value_norm, record, ring, seed):
    from madrona_rl_envs_playground_amd.simulators import chunk_indices, mappo_advantages, mappo_update, minibatch_indices
    out = {}
    out["rollout"] = timed(lambda: env.rollout(policy, T, seed=seed, record=record, ring=ring))

    def rest():
        advantages, returns = mappo_advantages(record, value_norm)
        if hasattr(record, "chunk_length"):
            indices = chunk_indices(record, 1, EPOCHS, device=ring.device)
        else:
            indices = minibatch_indices(T * record.num_worlds * record.num_players, 1, EPOCHS, device=ring.device)
        mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm)
    out["update"] = timed(rest)
    out["iteration"] = out["rollout"] + out["update"]
    return out


def torch_iteration(env, module, optimizers, state):
    """the reference's loop in torch on the same simulator: T acts and steps, GAE, EPOCHS passes over all chunks"""
    import torch
    n, p = env.num_envs, env.num_players
    cells = n * p
    x_of = lambda: env.static_world_major_observations.reshape((cells,) + tuple(env.static_world_major_observations.shape[2:])).transpose(1, 2).float()  # noqa: E731
    buf = {k: [] for k in ("obs", "act", "logp", "val", "rew", "done", "h0a", "h0c")}

    def rollout():
        with torch.no_grad():
            for t in range(T):
                done = env.static_dones.view(-1, 1).float().repeat(1, p).view(-1)
                if t % L == 0:
                    buf["h0a"].append(state[0].clone()), buf["h0c"].append(state[1].clone())
                x = x_of()
                logits, state[0] = module.actor(x, state[0], 1.0 - done)
                value, state[1] = module.critic(x, state[1], 1.0 - done)
                dist = torch.distributions.Categorical(logits=logits)
                action = dist.sample()
                env.static_actions.copy_(action.view(n, p).t().reshape(env.static_actions.shape).to(env.static_actions.dtype))
                env.n_step(env.static_actions)
                for k, v in (("obs", x), ("act", action), ("logp", dist.log_prob(action)), ("val", value[:, 0]), ("done", done),
                             ("rew", env.static_rewards.view(p, n).t().reshape(-1).float())):
                    buf[k].append(v)

    def update():
        obs, act, logp, val, rew, done = (torch.stack(buf[k]) for k in ("obs", "act", "logp", "val", "rew", "done"))
        adv, last = torch.zeros_like(val), torch.zeros(cells, device=val.device)
        for t in reversed(range(T)):
            nxt, keep = (val[t + 1], 1.0 - done[t + 1]) if t + 1 < T else (val[t], torch.ones_like(last))
            last = rew[t] + 0.99 * nxt * keep - val[t] + 0.99 * 0.95 * keep * last
            adv[t] = last
        ret = adv + val
        adv = (adv - adv.mean()) / (adv.std() + 1e-5)
        chunked = lambda a: a.view((T // L, L) + tuple(a.shape[1:])).transpose(0, 1).reshape((L, -1) + tuple(a.shape[2:]))  # noqa: E731
        obs, act, logp, val, ret, adv, masks = (chunked(a) for a in (obs, act, logp, val, ret, adv, 1.0 - done))
        h0a, h0c = torch.cat(buf["h0a"]), torch.cat(buf["h0c"])
        for _ in range(EPOCHS):
            logits, _ = module.actor.chunk(obs, h0a, masks)
            values, _ = module.critic.chunk(obs, h0c, masks)
            dist = torch.distributions.Categorical(logits=logits)
            ratio = (dist.log_prob(act) - logp).exp()
            policy_loss = -torch.min(ratio * adv, ratio.clamp(0.8, 1.2) * adv).mean() - 0.01 * dist.entropy().mean()
            v = values[..., 0]
            clipped = val + (v - val).clamp(-0.2, 0.2)
            huber = lambda e: torch.where(e.abs() <= 10.0, e * e / 2, 10.0 * (e.abs() - 5.0))  # noqa: E731
            value_loss = torch.max(huber(ret - v), huber(ret - clipped)).mean()
            for opt, loss, net in ((optimizers[0], policy_loss, module.actor), (optimizers[1], value_loss, module.critic)):
                opt.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(net.parameters(), 10.0)
                opt.step()

    out = {"rollout": timed(rollout), "update": timed(update)}
    out["iteration"] = out["rollout"] + out["update"]
    return out


def iteration_cost(game, layout, worlds, windows):
    import torch
    from madrona_rl_envs_playground_amd.simulators import CnnGruActorCritic, CnnGruPolicy, CnnGruRecord, MappoOptimizer, ValueNorm
    from tools.overcooked_train_device import make_env
    env = make_env(game, layout, worlds, T)
    device = env.static_actions.device
    _, players, height, width, channels = env.static_world_major_observations.shape
    torch.manual_seed(1)
    policy = CnnGruPolicy.from_module(CnnGruActorCritic(width, height, channels), device=device)
    policy.state(worlds, players)
    optimizer, value_norm = MappoOptimizer(policy), ValueNorm(device)
    record = CnnGruRecord(T, worlds, players, device, chunk_length=L)
    ring = torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=device)
    module = CnnGruActorCritic(width, height, channels).to(device)
    optimizers = [torch.optim.Adam(net.parameters(), lr=5e-4, eps=1e-5) for net in (module.actor, module.critic)]
    state = [torch.zeros(worlds * players, 64, device=device) for _ in range(2)]
    sides = {"device": lambda: device_iteration(env, policy, optimizer, value_norm, record, ring, 1),
             "torch": lambda: torch_iteration(env, module, optimizers, state)}
    for run in sides.values():
        run()  # warm
    samples = {side: {"rollout": [], "update": [], "iteration": []} for side in sides}
    for _ in range(windows):
        for side, run in sides.items():
            for part, ms in run().items():
                samples[side][part].append(ms)
    env.close()
    return {"game": game, "layout": layout, "worlds": worlds, "players": int(players), "chunks_per_epoch": T // L * worlds * int(players),
            **{side: {part: summary(v) for part, v in parts.items()} for side, parts in samples.items()}}


def plain_window():
    """one process, one window: a plain policy's rollout and update at 1024 worlds of cramped_room -> a JSON line"""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnRecord, MappoOptimizer, ValueNorm
    from tools.overcooked_train_device import make_env
    env = make_env("overcooked", "cramped_room", 1024, T)
    device = env.static_actions.device
    _, players, height, width, channels = env.static_world_major_observations.shape
    torch.manual_seed(1)
    policy = CnnPolicy.from_module(CnnActorCritic(width, height, channels), device=device)
    optimizer, value_norm = MappoOptimizer(policy), ValueNorm(device)
    record = CnnRecord(T, 1024, players, device)
    ring = torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=device)
    device_iteration(env, policy, optimizer, value_norm, record, ring, 1)  # warm
    runs = [device_iteration(env, policy, optimizer, value_norm, record, ring, 1) for _ in range(3)]
    env.close()
    print(json.dumps({"build_hash": _lib.build_hash(), "rollout": statistics.median(r["rollout"] for r in runs),
                      "update": statistics.median(r["update"] for r in runs)}))


def plain_cost(parent_tree, windows):
    builds = {"this": None, "parent": os.path.abspath(parent_tree)}
    got = {name: [] for name in builds}
    for _ in range(windows):
        for name, lib in builds.items():
            env = dict(os.environ)
            env.pop("MRL_PROBE_TREE", None)
            if lib:
                env["MRL_PROBE_TREE"] = lib
            proc = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-window"], env=env, capture_output=True, text=True, timeout=300)
            if proc.returncode != 0:
                raise RuntimeError(f"the {name} build's window failed:\n{proc.stderr[-2000:]}")
            got[name].append(json.loads(proc.stdout.strip().splitlines()[-1]))
    return {name: {"build_hash": rows[0]["build_hash"], "rollout": summary([r["rollout"] for r in rows]), "update": summary([r["update"] for r in rows])}
            for name, rows in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "cnn_gru_cost.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built; without it the plain paths are not compared")
    ap.add_argument("--plain-window", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.plain_window:
        return plain_window()
    from madrona_rl_envs_playground_amd import _lib
    out = {"build_hash": _lib.build_hash(), "T": T, "chunk_length": L, "epochs": EPOCHS, "iteration": []}
    for game, layout, worlds in SHAPES:
        out["iteration"].append(iteration_cost(game, layout, worlds, args.windows))
        print(json.dumps(out["iteration"][-1]), flush=True)
    if args.parent_tree:
        out["plain"] = plain_cost(args.parent_tree, args.windows)
        print(json.dumps(out["plain"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
