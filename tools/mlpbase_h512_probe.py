#!/usr/bin/env python3
"""What a collection step of the balance beam costs under MAPPO's MLP actor-critic at hidden_size 512 (``MlpBasePolicyH512``,
layer_N 2): us per loop step -- both seats' act through both nets, then the simulator's step -- over a rollout of T = 128 steps,
on the device (``env.rollout``: mrl_rollout_mlpbase with MRL_MLPBASE_H512) against the torch loop of the same float32 module on
the same simulator (tools/balance_mappo_probe.py's ``torch_rollout``), at 1024 and at 32 768 worlds, written to
profiles/mlpbase_h512_cost.json under the library's build hash.

    python tools/mlpbase_h512_probe.py                 measure (needs the GPU)
    python tools/mlpbase_h512_probe.py --plain TREE    also the plain hidden-64 rollout at 1024 worlds, this build against the package
                                                       built in TREE (a checkout of the parent commit): a window per process, the
                                                       processes alternating; a window is 8 rollouts of T steps after one that warms up

Two loops on one env in ALTERNATING windows, five each after one that warms both up; a window is one rollout behind a device
wait, timed by the host clock.  Medians, minima and maxima are reported.  The arithmetic floor per cell is 2 nets x 3 layers x 512
x 512 x 2 flop = 3.1 MFLOP; the file states it at the chip's 155 TF f32 matrix peak beside each row.  No ratio is asserted."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MRL_PROBE_TREE") or REPO)  # a --plain child of the other tree imports that tree's package
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "profiles", "mlpbase_h512_cost.json")
WORLDS, T, WINDOWS, LAYER_N = (1024, 32768), 128, 5, 2
FLOP_PER_CELL, PEAK_FLOPS = 2 * 3 * 512 * 512 * 2, 155e12


def measure(worlds, windows):
    import torch
    from balance_mappo_probe import torch_rollout
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    dev = torch.device("cuda", 0)
    env = BalanceMadronaTorch(worlds, 0)
    torch.manual_seed(1)
    policy = S.MlpBasePolicyH512.from_module(S.MlpBaseActorCritic(hidden=512, layer_N=LAYER_N), device=dev)
    module = policy.module()
    records = {side: S.MlpBaseRecord(T, worlds, env.n_players, dev) for side in ("torch", "device")}
    first = {"step": 0}

    def device_loop():
        env.rollout(policy, T, seed=1, first_step=first["step"], record=records["device"])
        first["step"] += T

    loops = {"torch": lambda: torch_rollout(env, module, records["torch"], T), "device": device_loop}

    def window(loop):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        return (time.perf_counter() - begin) * 1e6 / T

    for loop in loops.values():
        window(loop)  # warm-up
    times = {side: [] for side in loops}
    for _ in range(windows):
        for side, loop in loops.items():
            times[side].append(window(loop))
    env.close()
    out = {side: {"us_per_step": [round(x, 1) for x in xs], "median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1),
                  "max_us": round(max(xs), 1)} for side, xs in times.items()}
    gap = abs(out["torch"]["median_us"] - out["device"]["median_us"])
    spreads = sum(out[side]["max_us"] - out[side]["min_us"] for side in loops)
    out["faster"] = min(loops, key=lambda side: out[side]["median_us"])
    out["difference_exceeds_both_spreads"] = bool(gap > spreads)
    out["floor_us_at_155_tf"] = round(worlds * env.n_players * FLOP_PER_CELL / PEAK_FLOPS * 1e6, 1)
    return out


def plain_window(worlds=1024, rollouts=8):
    """us per step of the hidden-64 rollout with the package this process imported"""
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    dev = torch.device("cuda", 0)
    env = BalanceMadronaTorch(worlds, 0)
    torch.manual_seed(1)
    policy = S.MlpBasePolicy.from_module(S.MlpBaseActorCritic(layer_N=LAYER_N), device=dev)
    record = env.rollout(policy, T, seed=1)
    torch.cuda.synchronize()
    begin = time.perf_counter()
    for k in range(rollouts):
        env.rollout(policy, T, seed=1, first_step=(k + 1) * T, record=record)
    torch.cuda.synchronize()
    us = (time.perf_counter() - begin) * 1e6 / (rollouts * T)
    env.close()
    return us


def plain_against(tree, windows):
    """the plain rollout of this build and of the package in ``tree``, a fresh process per window, alternating; after a child that
    fails nothing more is started"""
    times = {"parent_build": [], "this_build": []}
    sides = [("parent_build", os.path.abspath(tree)), ("this_build", "")]
    for w in range(windows):
        for side, where in sides[::-1 if w & 1 else 1]:  # which build goes first alternates too
            proc = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--plain-window"],
                                  capture_output=True, text=True, env=dict(os.environ, MRL_PROBE_TREE=where))
            if proc.returncode != 0:
                sys.exit(f"{side}: a plain window ended with status {proc.returncode}: nothing more is started\n{proc.stdout}{proc.stderr}")
            times[side].append(float(proc.stdout.split()[-1]))
    out = {side: {"us_per_step": [round(x, 2) for x in xs], "median_us": round(statistics.median(xs), 2), "min_us": round(min(xs), 2),
                  "max_us": round(max(xs), 2)} for side, xs in times.items()}
    out["median_inside_or_below_parents_spread"] = bool(out["this_build"]["median_us"] <= out["parent_build"]["max_us"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", metavar="TREE")
    ap.add_argument("--plain-window", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--worlds", type=int, nargs="+", default=list(WORLDS))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.plain_window:
        print(plain_window())
        return
    from madrona_rl_envs_playground_amd import _lib
    record = {"build_hash": _lib.build_hash(), "game": "balance", "hidden": 512, "layer_N": LAYER_N, "num_steps": T, "windows": args.windows,
              "rows": {}, "what": "us per loop step (both seats' act through both nets + the step) of a rollout of T steps, the closing "
                                  "value act included: host clock around one rollout behind a device wait, divided by T; windows of the two "
                                  "loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for worlds in args.worlds:
        record["rows"][str(worlds)] = measure(worlds, args.windows)
        print(worlds, json.dumps(record["rows"][str(worlds)]), flush=True)
        with open(args.out, "w") as f:  # (after every size: a later, larger one that runs out of time leaves the earlier ones)
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    if args.plain:
        record["plain_hidden_64_rollout_1024_worlds"] = plain_against(args.plain, args.windows)
        print(json.dumps(record["plain_hidden_64_rollout_1024_worlds"]), flush=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
