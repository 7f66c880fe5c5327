#!/usr/bin/env python3
"""What one iteration of the reference's own training recipe costs -- MAPPO's CNN actor-critic on Simplecooked at the shape of
its notebook overcooked_compiled_colab.ipynb: layout ``simple``, 800 worlds, T = 200 = the horizon, 7 epochs of one minibatch
over all 320 000 samples -- with every phase on the device against the torch loop of the same networks on the same simulator:
ms per iteration and per phase, written to profiles/simplecooked_mappo_cost.json under the library's build hash.

    python tools/simplecooked_mappo_probe.py            measure (needs the GPU)

Two loops on one env, in ALTERNATING windows, five windows each after one that warms both up, medians and extremes reported.  A
window is one iteration, timed as a whole (one wait at its end) and, in a second pass of the same window, phase by phase (a wait
after each phase):
  torch    rollout: per step and seat the int8 -> float cast, ``module.actor`` / ``module.critic`` (the ``CnnActorCritic`` whose
           parameters alias the flat tensor), ``Categorical.sample``, ``env.n_step(actions, out=slot)``, reward and done rows
           copied; advantages: the reference's ``compute_returns`` loop over the T rows in torch; update: ``torch_update`` of
           tools/cnn_update_probe.py (the loop of ``R_MAPPO.train``);
  device   ``env.rollout`` (mrl_rollout_cnn), ``mappo_advantages`` (mrl_gae + a handful of torch ops), ``minibatch_indices`` +
           ``mappo_update`` (mrl_mappo_update).
No ratio is asserted or required: the numbers are what was measured."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "profiles", "simplecooked_mappo_cost.json")
LAYOUT, WORLDS, T, EPOCHS, MINIBATCHES = "simple", 800, 200, 7, 1
LR, ENT, GAMMA, LAMBDA = 1e-2, 0.0, 0.99, 0.95
WINDOWS = 5
PHASES = ("rollout", "advantages", "update")


def torch_rollout(env, module, record, ring, num_steps):
    """the rollout loop of train/MAPPO/main_player.py:211-261 on the env's own tensors: both seats through both nets, a step into
    the next ring slot, the rows of the record filled as ``mrl_rollout_cnn`` fills them"""
    import torch
    p = env.num_players
    ring[0].copy_(env.static_world_major_observations)
    with torch.no_grad():
        for k in range(num_steps + 1):
            x = ring[k].transpose(2, 3).reshape((-1,) + (env.width, env.height, ring.shape[-1])).float()  # (N P, W, H, F)
            record.values[k].view(-1).copy_(module.critic(x).squeeze(1))
            if k:
                record.rewards[k - 1].copy_(env.static_rewards.view(p, -1).t())
            done = env.static_dones.view(-1, 1).expand(-1, p).float()
            if k == num_steps:
                record.next_done.copy_(done)
                break
            record.dones[k].copy_(done)
            dist = torch.distributions.Categorical(logits=module.actor(x))
            action = dist.sample()
            record.actions[k].view(-1).copy_(action)
            record.logprobs[k].view(-1).copy_(dist.log_prob(action))
            env.n_step(action.view(-1, p).t().reshape(p, -1, 1).contiguous(), out=ring[k + 1])


def torch_advantages(record, value_norm):
    """``SharedReplayBuffer.compute_returns`` with ``use_gae`` and ValueNorm (utils/shared_buffer.py:216-228), then ``R_MAPPO.train``'s
    normalisation (r_mappo.py:174-182): a loop over the T rows, as the reference runs it"""
    import torch
    t = record.num_steps
    values = value_norm.denormalize(record.values)
    masks = 1.0 - torch.cat([record.dones, record.next_done[None]])
    returns, gae = torch.zeros_like(record.rewards), 0
    for step in reversed(range(t)):
        delta = record.rewards[step] + GAMMA * values[step + 1] * masks[step + 1] - values[step]
        gae = delta + GAMMA * LAMBDA * masks[step + 1] * gae
        returns[step] = gae + values[step]
    advantages = returns - values[:-1]
    return (advantages - advantages.mean()) / (advantages.std() + 1e-5), returns


def measure(windows):
    import torch
    import cnn_update_probe as upd
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.overcooked2_env import OvercookedMadrona
    upd.EPOCHS, upd.MINIBATCHES, upd.ENT = EPOCHS, MINIBATCHES, ENT  # the notebook's epochs and entropy_coef in that file's loop
    dev = torch.device("cuda", 0)
    env = OvercookedMadrona(LAYOUT, WORLDS, 0, horizon=T)
    _, players, h, w, f = env.static_world_major_observations.shape
    count = T * WORLDS * players
    torch.manual_seed(1)
    start = S.CnnActorCritic(w, h, f)
    sides = {}
    for name in ("torch", "device"):
        policy = S.CnnPolicy.from_module(start, device=dev)
        sides[name] = {"policy": policy, "value_norm": S.ValueNorm(dev), "record": S.CnnRecord(T, WORLDS, players, dev),
                       "ring": torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=dev)}
    module = sides["torch"]["policy"].module()
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=LR, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=LR, eps=1e-5)
    optimizer = S.MappoOptimizer(sides["device"]["policy"], lr=LR, critic_lr=LR)
    shuffles = torch.Generator(device=dev).manual_seed(1)
    step = {"first": 0}

    def torch_phases():
        s = sides["torch"]
        yield lambda: torch_rollout(env, module, s["record"], s["ring"], T)
        yield lambda: s.update(zip(("advantages", "returns"), torch_advantages(s["record"], s["value_norm"])))
        yield lambda: upd.torch_update(module, actor_opt, critic_opt, s["value_norm"], s["record"], s["ring"], s["advantages"], s["returns"])

    def device_update(s):
        indices = S.minibatch_indices(count, MINIBATCHES, EPOCHS, generator=shuffles, device=dev)
        S.mappo_update(s["policy"], optimizer, s["record"], s["ring"], s["advantages"], s["returns"], indices, value_norm=s["value_norm"],
                       entropy_coef=ENT)

    def device_phases():
        s = sides["device"]

        def rollout():
            env.rollout(s["policy"], T, seed=1, first_step=step["first"], record=s["record"], ring=s["ring"])
            step["first"] += T
        yield rollout
        yield lambda: s.update(zip(("advantages", "returns"), S.mappo_advantages(s["record"], s["value_norm"], GAMMA, LAMBDA)))
        yield lambda: device_update(s)

    def window(phases, split):
        """ms of one iteration: as a whole, or the three phases each behind a wait of its own"""
        env.n_step(torch.zeros_like(env.static_actions))  # (the torch loop redirects the output: back to the simulator's own tensor)
        torch.cuda.synchronize()
        times, begin = [], time.perf_counter()
        for phase in phases():
            phase()
            if split:
                torch.cuda.synchronize()
                times.append((time.perf_counter() - begin) * 1e3)
                begin = time.perf_counter()
        torch.cuda.synchronize()
        return times if split else (time.perf_counter() - begin) * 1e3

    window(torch_phases, False), window(device_phases, False)  # warm-up
    names = [f"{side}_{what}" for side in ("torch", "device") for what in ("iteration",) + PHASES]
    times = {name: [] for name in names}
    for _ in range(windows):
        for side, phases in (("torch", torch_phases), ("device", device_phases)):
            times[f"{side}_iteration"].append(window(phases, False))
            for what, ms in zip(PHASES, window(phases, True)):
                times[f"{side}_{what}"].append(ms)
    finite = all(bool(torch.isfinite(s["policy"].params).all()) for s in sides.values())
    env.close()

    def summary(xs):
        return {"ms": [round(x, 2) for x in xs], "median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2),
                "max_ms": round(max(xs), 2)}

    out = {name: summary(xs) for name, xs in times.items()}
    out["parameters_finite"] = finite
    out["env_steps_per_s"] = {side: round(T * WORLDS / (out[f"{side}_iteration"]["median_ms"] * 1e-3)) for side in ("torch", "device")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    rows = measure(args.windows)
    record = {"build_hash": _lib.build_hash(), "game": "simplecooked", "layout": LAYOUT, "worlds": WORLDS, "num_steps": T, "horizon": T,
              "epochs": EPOCHS, "minibatches": MINIBATCHES, "samples": T * WORLDS * 2, "lr": LR, "entropy_coef": ENT, "windows": args.windows,
              "rows": rows,
              "what": "ms per iteration (rollout of T steps, advantages, E x M minibatch steps): host clock around one window behind a "
                      "device wait; *_iteration one wait at the end, the phases a wait each; windows of the two loops alternating in "
                      "one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rows), flush=True)
    print("->", args.out)


if __name__ == "__main__":
    main()
