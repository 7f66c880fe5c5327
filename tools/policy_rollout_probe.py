#!/usr/bin/env python3
"""What collecting a PPO rollout costs with the policy on the device (mrl_rollout_policy, mrl_gae) against the loop a user
runs today: us per rollout step, written to profiles/policy_rollout_cost.json under the library's build hash.

    python tools/policy_rollout_probe.py                 measure (needs the GPU)
    python tools/policy_rollout_probe.py --trace DIR     one more run under `rocprofv3 --kernel-trace --stats` (no other
                                                         tracing) -> profiles/policy_rollout_kernel_stats.csv

T = 128 rows (the trainer's num_steps) at 1024, 65536 and 1 M worlds, Cartpole and Acrobot.  Two loops, in one process, in
ALTERNATING windows on the same simulator class, five windows each after one that warms both up, medians and extremes
reported:
  torch_loop      the collection loop of the reference's trainer (scripts/cartpole_train_torch.py:204-218) as this package
                  could run it before: the torch agent on the GPU, `env.step`, the six row writes;
  rollout_policy  `env.rollout(policy, T)`.
and the same for the advantages: `torch_gae`, the T sequential torch iterations of :245-256, against `gae`.
A window is `rollouts` whole rollouts between two device events (4, or 1 at 1 M worlds).  `device_below_torch` says
whether the device loop's median lies below the torch loop's by more than the two loops' own spreads (max - min) added."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "policy_rollout_cost.json")
STATS_OUT = os.path.join(REPO, "profiles", "policy_rollout_kernel_stats.csv")
T = 128
CONFIGS = [(game, n) for game in ("cartpole", "acrobot") for n in (1024, 65536, 1 << 20)]
GAMMA, GAE_LAMBDA = 0.99, 0.95


def make(game, n):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.acrobot_env import AcrobotMadronaTorch
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    env = CartpoleMadronaTorch(n, 0) if game == "cartpole" else AcrobotMadronaTorch(n, 0)
    torch.manual_seed(1)
    agent = S.MlpAgent(4, env.single_action_space.n).cuda()
    return env, agent, S.MlpPolicy.from_module(agent)


def torch_buffers(n):
    import torch
    z = lambda *shape: torch.zeros(shape, device="cuda")  # noqa: E731
    return {"obs": z(T, n, 4), "actions": z(T, n), "logprobs": z(T, n), "rewards": z(T, n), "dones": z(T, n), "values": z(T, n)}


def torch_loop(env, agent, b, next_obs, next_done):
    """one rollout: per step the agent's forward, the draw, the step and the six row writes"""
    import torch
    for step in range(T):
        b["obs"][step] = next_obs
        b["dones"][step] = next_done
        with torch.no_grad():
            action, logprob, _, value = agent.get_action_and_value(next_obs)
            b["values"][step] = value.flatten()
        b["actions"][step] = action
        b["logprobs"][step] = logprob
        next_obs, reward, next_done, _ = env.step(action)
        b["rewards"][step] = reward.view(-1)
    return next_obs, next_done


def torch_gae(agent, b, next_obs, next_done):
    import torch
    with torch.no_grad():
        next_value = agent.get_value(next_obs).reshape(1, -1)
        advantages = torch.zeros_like(b["rewards"])
        last = 0
        for t in reversed(range(T)):
            alive = 1.0 - (next_done if t == T - 1 else b["dones"][t + 1])
            ahead = next_value if t == T - 1 else b["values"][t + 1]
            delta = b["rewards"][t] + GAMMA * ahead * alive - b["values"][t]
            advantages[t] = last = delta + GAMMA * GAE_LAMBDA * alive * last
        return advantages, advantages + b["values"]


def timed(fn, count):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(count):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / count


def summary(times):
    t = sorted(times)
    return {"us": [round(v, 3) for v in times], "median": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def verdict(device, torch_row):
    spread = (device["max"] - device["min"]) + (torch_row["max"] - torch_row["min"])
    return {"spread_us": round(spread, 3), "torch_minus_device_median_us": round(torch_row["median"] - device["median"], 3),
            "device_below_torch": torch_row["median"] - device["median"] > spread}


def measure(game, n, repeats):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    env, agent, policy = make(game, n)
    b = torch_buffers(n)
    rollouts = 1 if n > 65536 else 4
    state = {"obs": env.reset(), "done": torch.zeros(n, device="cuda"), "out": None}

    def loop_a():
        state["obs"], state["done"] = torch_loop(env, agent, b, state["obs"], state["done"])

    def loop_b():
        state["out"] = env.rollout(policy, T, out=state["out"])

    times = {"torch_loop": [], "rollout_policy": [], "torch_gae": [], "gae": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = timed(loop_a, rollouts) / T
        d = timed(loop_b, rollouts) / T
        ga = timed(lambda: torch_gae(agent, b, state["obs"], state["done"]), rollouts)
        gd = timed(lambda: S.gae(state["out"], GAMMA, GAE_LAMBDA), 20 * rollouts)
        if rep:
            for name, value in (("torch_loop", a), ("rollout_policy", d), ("torch_gae", ga), ("gae", gd)):
                times[name].append(value)
    row = {name: summary(v) for name, v in times.items()}
    row["step_kernel"] = env.sim.kernel_name
    row["rollouts_per_window"] = rollouts
    row["collect"] = verdict(row["rollout_policy"], row["torch_loop"])
    row["advantages"] = verdict(row["gae"], row["torch_gae"])
    env.close()
    return row


def traced():
    """what runs under the profiler: one rollout of T rows per game at 1024 worlds, and one gae"""
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    for game in ("cartpole", "acrobot"):
        env, _, policy = make(game, 1024)
        S.gae(env.rollout(policy, T), GAMMA, GAE_LAMBDA)
        torch.cuda.synchronize()
        env.close()


def trace(out_dir):
    out_dir = os.path.abspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "kt", "--",
           sys.executable, os.path.abspath(__file__), "--traced"]
    proc = subprocess.run(cmd, capture_output=True, text=True)
    open(os.path.join(out_dir, "rocprofv3.log"), "w").write(proc.stdout + proc.stderr)
    if proc.returncode != 0:
        raise SystemExit(f"rocprofv3 failed ({proc.returncode}): see {out_dir}/rocprofv3.log")
    found = glob.glob(out_dir + "/**/*kernel_stats.csv", recursive=True)
    if not found:
        raise SystemExit(f"no kernel_stats.csv under {out_dir}")
    shutil.copy(found[0], STATS_OUT)
    calls = {row["Name"].split("(")[0].split("<")[0].split("::")[-1]: int(row["Calls"]) for row in csv.DictReader(open(STATS_OUT))}
    print("launches of the traced run (two rollouts of", T, "rows):", json.dumps(calls))
    print("->", STATS_OUT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", metavar="DIR", help="run once more under rocprofv3 --kernel-trace --stats, output under DIR")
    ap.add_argument("--traced", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.traced:
        traced()
        return
    if args.trace:
        trace(args.trace)
        return
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for game, n in CONFIGS:
        rows[f"{game}@{n}"] = measure(game, n, args.repeats)
        print(f"{game}@{n}", json.dumps(rows[f"{game}@{n}"]), flush=True)
    record = {"build_hash": _lib.build_hash(), "num_steps": T, "repeats": args.repeats, "rows": rows,
              "what": "us per rollout step (torch_loop, rollout_policy) and us per advantage pass (torch_gae, gae): device events around "
                      "whole rollouts, windows of the two loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
