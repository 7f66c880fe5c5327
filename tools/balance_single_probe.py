#!/usr/bin/env python3
"""What one iteration of single-agent PPO on the balance beam costs with every phase on the device, against the loop
scripts/balance_train_single.py runs in torch on the same simulator: us per iteration, written to
profiles/balance_single_cost.json under the library's build hash.

    python tools/balance_single_probe.py          measure (needs the GPU)

One iteration is a rollout of T steps, the advantages and E x M = 4 x 4 minibatch steps.  Shapes: the script's own (4 worlds,
T = 1000) and 1024 and 65536 worlds at T = 128.  Two loops, in one process, in ALTERNATING windows, five windows each after
one that warms both up, medians and extremes reported:
  torch_loop   the script's iteration (:204-313) on ``BalanceGym``: per step ``agent.get_action_and_value``, six buffer rows and
               ``envs.step`` -- whose partner is a ``RandomVectorAgent`` on torch's generator --, then T sequential torch
               iterations for the advantages and the update phase of tools/ppo_update_probe.py (``torch_update``);
  device       ``BalanceGym.rollout`` + ``gae`` + ``minibatch_indices`` + ``ppo_update`` on the flat parameter tensor.
``device_below_torch`` says whether the device loop's median lies below the torch loop's by more than the two loops' own
spreads (max - min) added.  The figures are written as they come, a size where torch wins included."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "profiles", "balance_single_cost.json")
SHAPES = ((4, 1000), (1024, 128), (65536, 128))  # (worlds, T)
GAMMA, LAMBDA = 0.99, 0.95


def torch_iteration(env, agent, optimizer, policy, buffers, steps):
    """scripts/balance_train_single.py:204-313 for one update, on preallocated buffers"""
    import torch
    import ppo_update_probe as update
    from madrona_rl_envs_playground_amd.simulators import Rollout
    obs, actions, logprobs, rewards, dones, values = buffers
    next_obs = env.reset()
    next_done = torch.zeros(env.num_envs, device=next_obs.device)
    for step in range(steps):
        obs[step] = next_obs
        dones[step] = next_done
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(next_obs)
            values[step] = value.flatten()
        actions[step] = action
        logprobs[step] = logprob
        next_obs, reward, next_done, _ = env.step(action)
        rewards[step] = reward.view(-1)
    with torch.no_grad():
        next_value = agent.get_value(next_obs).reshape(1, -1)
        advantages = torch.zeros_like(rewards)
        lastgaelam = 0
        for t in reversed(range(steps)):
            nextnonterminal = 1.0 - (next_done if t == steps - 1 else dones[t + 1])
            nextvalues = next_value if t == steps - 1 else values[t + 1]
            delta = rewards[t] + GAMMA * nextvalues * nextnonterminal - values[t]
            advantages[t] = lastgaelam = delta + GAMMA * LAMBDA * nextnonterminal * lastgaelam
        returns = advantages + values
    rollout = Rollout(obs, actions, logprobs, values, rewards, dones, None, None, None)
    update.torch_update(agent, optimizer, policy, rollout, advantages, returns)


def measure(n, steps, repeats):
    import torch
    import ppo_update_probe as update
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceGym
    env = BalanceGym(n, 0, False)
    torch.manual_seed(1)
    policy = S.MlpPolicy.from_module(S.MlpAgent(7, 4).cuda(), observation="beam")
    device_policy = S.MlpPolicy.from_module(policy.module(), observation="beam")
    device_optimizer = S.PpoOptimizer(device_policy)
    agent = policy.module()
    optimizer = torch.optim.Adam(agent.parameters(), lr=2.5e-4, eps=1e-5)
    shuffles = torch.Generator(device="cuda").manual_seed(1)
    dev = "cuda:0"
    buffers = [torch.zeros((steps, n, 7), device=dev)] + [torch.zeros((steps, n), device=dev) for _ in range(5)]
    kept = {"rollout": None, "first_step": 0}

    def device_iteration():
        kept["rollout"] = r = env.rollout(device_policy, steps, seed=1, first_step=kept["first_step"], out=kept["rollout"])
        kept["first_step"] += steps
        advantages, returns = S.gae(r, GAMMA, LAMBDA)
        indices = S.minibatch_indices(steps * n, update.MINIBATCHES, update.EPOCHS, generator=shuffles, device="cuda")
        S.ppo_update(device_policy, device_optimizer, r, advantages, returns, indices, clip_coef=update.CLIP, ent_coef=update.ENT,
                     vf_coef=update.VF, max_grad_norm=update.MAX_NORM)

    times = {"torch_loop": [], "device": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = update.timed(lambda: torch_iteration(env, agent, optimizer, policy, buffers, steps))
        d = update.timed(device_iteration)
        if rep:
            times["torch_loop"].append(a)
            times["device"].append(d)
    row = {name: update.summary(v) for name, v in times.items()}
    spread = (row["device"]["max"] - row["device"]["min"]) + (row["torch_loop"]["max"] - row["torch_loop"]["min"])
    row["spread_us"] = round(spread, 1)
    row["torch_over_device_median"] = round(row["torch_loop"]["median"] / row["device"]["median"], 2)
    row["device_below_torch"] = row["torch_loop"]["median"] - row["device"]["median"] > spread
    row["num_worlds"], row["num_steps"], row["minibatch_size"] = n, steps, steps * n // update.MINIBATCHES
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    import ppo_update_probe as update
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for n, steps in SHAPES:
        name = f"balance@{n}x{steps}"
        rows[name] = measure(n, steps, args.repeats)
        print(name, json.dumps(rows[name]), flush=True)
    record = {"build_hash": _lib.build_hash(), "epochs": update.EPOCHS, "minibatches": update.MINIBATCHES, "repeats": args.repeats,
              "rows": rows, "what": "us per iteration (rollout of T steps + advantages + E x M minibatch steps): device events around "
                                    "one whole iteration, windows of the two loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
