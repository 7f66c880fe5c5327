#!/usr/bin/env python3
"""What one PPO update costs on the device (``ppo_update``: mrl_ppo_update, three launches per minibatch) against the loop a
user of ``MlpPolicy.module()`` runs in torch: us per update, written to profiles/ppo_update_cost.json under the library's
build hash.

    python tools/ppo_update_probe.py          measure (needs the GPU)

One update is E = 4 epochs of M = 4 minibatches over a Cartpole batch of T = 128 rows at N = 1024 and 65536 worlds.  Two
loops, in one process, in ALTERNATING windows on the same rollout, five windows each after one that warms both up, medians and
extremes reported:
  torch_loop   the update phase of the reference's trainer (scripts/cartpole_train_torch.py:267-315) written with torch on
               ``policy.module()`` and ``torch.optim.Adam`` -- shuffle, gather, both forward passes, the clipped losses,
               backward, clip_grad_norm_, step -- and the ``load_`` that hands the result back to the rollout kernel;
  ppo_update   ``minibatch_indices`` + ``ppo_update`` on the flat parameter tensor.
``device_below_torch`` says whether the device loop's median lies below the torch loop's by more than the two loops' own
spreads (max - min) added."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "ppo_update_cost.json")
T, EPOCHS, MINIBATCHES = 128, 4, 4
WORLDS = (1024, 65536)
CLIP, ENT, VF, MAX_NORM = 0.2, 0.01, 0.5, 0.5


def minibatch_loss(agent, obs, actions, old_logp, advantages, returns, old_values):
    """the PPO loss of include/mrl_envs.h (mrl_ppo_update) with the trainer's defaults, in torch"""
    import torch
    logp = torch.log_softmax(agent.actor(obs), dim=1)
    ratio = (logp.gather(1, actions.long().unsqueeze(1)).squeeze(1) - old_logp).exp()
    a = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
    policy_term = torch.maximum(-a * ratio, -a * ratio.clamp(1 - CLIP, 1 + CLIP)).mean()
    value = agent.critic(obs).squeeze(1)
    near = old_values + (value - old_values).clamp(-CLIP, CLIP)
    value_term = 0.5 * torch.maximum((value - returns).square(), (near - returns).square()).mean()
    entropy = -(logp.exp() * logp).sum(dim=1).mean()
    return policy_term - ENT * entropy + VF * value_term


def torch_update(agent, optimizer, policy, r, advantages, returns):
    """E shuffles cut into M minibatches; per minibatch a gather, the loss, backward, clip_grad_norm_ and an Adam step"""
    import torch
    flat = [r.obs.reshape(-1, r.obs.shape[-1]), r.actions.reshape(-1), r.logprobs.reshape(-1), advantages.reshape(-1),
            returns.reshape(-1), r.values.reshape(-1)]
    count = flat[1].numel()
    for _ in range(EPOCHS):
        for rows in torch.randperm(count, device=flat[0].device).chunk(MINIBATCHES):
            loss = minibatch_loss(agent, *[t[rows] for t in flat])
            optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(agent.parameters(), MAX_NORM)
            optimizer.step()
    policy.load_(agent)


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(times):
    t = sorted(times)
    return {"us": [round(v, 1) for v in times], "median": round(statistics.median(t), 1), "min": round(t[0], 1), "max": round(t[-1], 1)}


def measure(n, repeats):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    env = CartpoleMadronaTorch(n, 0)
    torch.manual_seed(1)
    policy = S.MlpPolicy.from_module(S.MlpAgent(4, 2).cuda())
    rollout = env.rollout(policy, T)
    advantages, returns = S.gae(rollout, 0.99, 0.95)
    device_policy = S.MlpPolicy.from_module(policy.module())
    device_optimizer = S.PpoOptimizer(device_policy)
    agent = policy.module()
    optimizer = torch.optim.Adam(agent.parameters(), lr=2.5e-4, eps=1e-5)
    shuffles = torch.Generator(device="cuda").manual_seed(1)

    def device_update():
        indices = S.minibatch_indices(T * n, MINIBATCHES, EPOCHS, generator=shuffles, device="cuda")
        S.ppo_update(device_policy, device_optimizer, rollout, advantages, returns, indices, clip_coef=CLIP, ent_coef=ENT, vf_coef=VF,
                     max_grad_norm=MAX_NORM)

    times = {"torch_loop": [], "ppo_update": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = timed(lambda: torch_update(agent, optimizer, policy, rollout, advantages, returns))
        d = timed(device_update)
        if rep:
            times["torch_loop"].append(a)
            times["ppo_update"].append(d)
    row = {name: summary(v) for name, v in times.items()}
    spread = (row["ppo_update"]["max"] - row["ppo_update"]["min"]) + (row["torch_loop"]["max"] - row["torch_loop"]["min"])
    row["spread_us"] = round(spread, 1)
    row["torch_minus_device_median_us"] = round(row["torch_loop"]["median"] - row["ppo_update"]["median"], 1)
    row["device_below_torch"] = row["torch_loop"]["median"] - row["ppo_update"]["median"] > spread
    row["minibatch_size"] = T * n // MINIBATCHES
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for n in WORLDS:
        rows[f"cartpole@{n}"] = measure(n, args.repeats)
        print(f"cartpole@{n}", json.dumps(rows[f"cartpole@{n}"]), flush=True)
    record = {"build_hash": _lib.build_hash(), "num_steps": T, "epochs": EPOCHS, "minibatches": MINIBATCHES, "repeats": args.repeats,
              "rows": rows, "what": "us per update of E x M minibatch steps: device events around one whole update, windows of the two "
                                    "loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
