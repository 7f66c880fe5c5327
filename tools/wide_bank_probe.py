#!/usr/bin/env python3
"""What a policy per world costs under the wide policy: the bank act (``mrl_agent_act_bank``: the effective ids, the plan, the four
layers over its tiles, the head) against the plain act (``mrl_agent_act``) in the loop both seats act, then the step, on Hanabi
``full``; us per loop step, written to profiles/wide_bank_cost.json under the library's build hash.

    python tools/wide_bank_probe.py                          measure (needs the GPU)
    python tools/wide_bank_probe.py --parent-tree DIR        also the plain act of this build against the build in DIR

1000 and 65536 worlds.  Every comparison runs its two sides in ALTERNATING windows of T = 16 loop steps, five windows each after
one that warms both up; medians and extremes are reported as they come, nothing is asserted.
  a  ``k1``      a bank of one (ids all 0) against the plain act under the same policy: the price of the effective ids, the plan
                 and the indirection, everything else being equal.
  b  ``k4``      a bank of four with random ids and a random resample behind every step against four simulators of N / 4 worlds,
                 each under the plain act with one of the four policies, one after the other on the same stream -- the only way
                 without a bank.
  c  ``cross``   the 4 x 4 cross-play loop step on one simulator whose world n plays pair n mod 16 against sixteen simulators of
                 N / 16 worlds with two plain acts and a step each.
  d  ``plain_act``   with ``--parent-tree``: the plain loop step of this build against the same calls of the build in DIR, a checkout
                 of the parent commit with its library built, in ALTERNATING PROCESSES, a window each.  The layer kernel became a
                 template for the bank; the plain act must not have paid for it.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "wide_bank_cost.json")
SIZES = (1000, 65536)
WINDOWS, T, K = 5, 16, 4
CONFIG = "full"
CASE_TIMEOUT_S = 300


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e6 / T


def alternate(sides):
    """{name: window function} -> {name: summary}; a window is T loop steps"""
    for fn in sides.values():
        fn()  # warm-up
    times = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            times[name].append(timed(fn))
    return {name: summary(xs) for name, xs in times.items()}


def dims():
    from madrona_rl_envs_playground_amd import hanabi_spec
    from madrona_rl_envs_playground_amd.envs.hanabi_env import config_choice
    c = config_choice[CONFIG]
    return hanabi_spec.observation_size(c), hanabi_spec.state_size(c), hanabi_spec.num_moves(c)


def make_policies(count, device):
    import torch
    from madrona_rl_envs_playground_amd.simulators import WideAgent, WidePolicy
    policies = []
    for seed in range(count):
        torch.manual_seed(seed)
        policies.append(WidePolicy.from_module(WideAgent(*dims(), orthogonal=True), device=device))
    return policies


def make_sim(worlds):
    """a Hanabi ``full`` simulator and a workspace of the plain act for it"""
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.envs.hanabi_env import config_choice
    from madrona_rl_envs_playground_amd.simulators import ExecMode, HanabiSimulator
    c = config_choice[CONFIG]
    sim = HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=worlds, colors=c["colors"], ranks=c["ranks"], players=c["players"],
                          max_information_tokens=c["max_information_tokens"], max_life_tokens=c["max_life_tokens"])
    workspace = torch.empty(int(_lib.lib().mrl_agent_workspace_bytes(worlds)), dtype=torch.uint8, device=torch.device("cuda", 0))
    return sim, workspace


def plain_steps(sim, workspace, seats, at):
    """T loop steps: seat p acts under seats[p], then the step"""
    from madrona_rl_envs_playground_amd.simulators import agent_act
    for t in range(T):
        for p, policy in enumerate(seats):
            agent_act(sim, p, policy, seed=1, step=at + t, workspace=workspace)
        sim.step()


def measure(n):
    import torch
    from madrona_rl_envs_playground_amd.simulators import CnnResample, WidePolicyBank, agent_act_bank, wide_resample
    device = torch.device("cuda", 0)
    sim, workspace = make_sim(n)
    policies = make_policies(K, device)
    bank1, bank4 = WidePolicyBank.from_policies(policies[:1]), WidePolicyBank.from_policies(policies)
    step = {"at": 0}

    def numbered(fn):
        def window():
            fn(step["at"])
            step["at"] += T
        return window

    def bank_steps(bank, ids, at, resample=None, episodes=None):
        for t in range(T):
            agent_act_bank(sim, 0, bank, ids, seed=1, step=at + t)
            agent_act_bank(sim, 1, bank, ids, seed=1, step=at + t)
            sim.step()
            if resample is not None:
                wide_resample(sim, ids, episodes, resample)

    out = {"worlds": n, "steps_per_window": T, "policies": K, "config": CONFIG}

    # a: a bank of one against the plain act
    zeros = torch.zeros((n, 2), dtype=torch.int32, device=device)
    out["k1"] = alternate({
        "plain_step": numbered(lambda at: plain_steps(sim, workspace, [policies[0]] * 2, at)),
        "bank_step": numbered(lambda at: bank_steps(bank1, zeros, at)),
    })

    # b: four policies over the worlds at random, resampled at every game's end, against four simulators of N / 4
    ids = torch.randint(0, K, (n, 2), generator=torch.Generator().manual_seed(0), dtype=torch.int32).to(device)
    episodes = torch.zeros(n, dtype=torch.int32, device=device)
    resample = CnnResample("random", 0, K, 2, seed=2)
    quarters = [make_sim(n // K) for _ in range(K)]

    def four(at):
        for (s, w), policy in zip(quarters, policies):
            plain_steps(s, w, [policy] * 2, at)

    out["k4"] = alternate({
        "four_simulators_step": numbered(four),
        "bank_step": numbered(lambda at: bank_steps(bank4, ids, at, resample, episodes)),
    })
    for s, _ in quarters:
        s.close()
    del quarters

    # c: the 4 x 4 cross-play loop step against sixteen simulators
    pair = torch.arange(n, device=device) % (K * K)
    pair_ids = torch.stack([pair // K, pair % K], dim=1).to(torch.int32).contiguous()
    sixteenths = [make_sim(n // (K * K)) for _ in range(K * K)]

    def sixteen(at):
        for i, (s, w) in enumerate(sixteenths):
            plain_steps(s, w, [policies[i // K], policies[i % K]], at)

    out["cross"] = alternate({"sixteen_simulators_step": numbered(sixteen), "bank_step": numbered(lambda at: bank_steps(bank4, pair_ids, at))})
    for s, _ in sixteenths:
        s.close()
    sim.close()
    return out


def plain_window(n):
    """one window of the plain loop in this process, after one that warms up -> us per loop step"""
    import torch
    sim, workspace = make_sim(n)
    policy = make_policies(1, torch.device("cuda", 0))[0]
    plain_steps(sim, workspace, [policy] * 2, 0)
    us = timed(lambda: plain_steps(sim, workspace, [policy] * 2, T))
    sim.close()
    return us


def child(args, tree=REPO):
    """this file with ``args`` in a process of its own that imports the package of ``tree`` -> (status, the last JSON line)"""
    proc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--tree", tree] + args,
                          capture_output=True, text=True)
    if proc.returncode != 0:
        print(proc.stdout + proc.stderr, file=sys.stderr)
        return proc.returncode, None
    return 0, json.loads([x for x in proc.stdout.splitlines() if x.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: measure the plain act against it")
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)  # a child imports the package from here
    ap.add_argument("--case", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--plain-window", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    if args.case is not None:
        print(json.dumps(measure(args.case)), flush=True)
        return 0
    if args.plain_window is not None:
        from madrona_rl_envs_playground_amd import _lib
        print(json.dumps({"us": plain_window(args.plain_window), "build_hash": _lib.build_hash()}), flush=True)
        return 0
    from madrona_rl_envs_playground_amd import _lib
    results = []
    for n in SIZES:
        status, result = child(["--case", str(n)])
        if status:
            print(f"{n} worlds ended with status {status}: nothing more is started", file=sys.stderr)
            return status
        print(json.dumps(result), flush=True)
        results.append(result)
    report = {"build_hash": _lib.source_hash(), "unit": "us per loop step (both seats act, then the step)", "game": "hanabi " + CONFIG,
              "windows": WINDOWS, "steps_per_window": T, "cases": results}
    if args.parent_tree:
        plain = []
        for n in SIZES:
            times, hashes = {"this_build": [], "parent_build": []}, {}
            for _ in range(WINDOWS):
                for name, tree in (("parent_build", os.path.abspath(args.parent_tree)), ("this_build", REPO)):
                    status, result = child(["--plain-window", str(n)], tree)
                    if status:
                        print(f"the plain act of {name} at {n} worlds ended with status {status}: nothing more is started", file=sys.stderr)
                        return status
                    times[name].append(result["us"])
                    hashes[name] = result["build_hash"]
            entry = {"worlds": n, "build_hashes": hashes}
            entry.update({name: summary(xs) for name, xs in times.items()})
            entry["median_difference_us"] = round(entry["this_build"]["median_us"] - entry["parent_build"]["median_us"], 1)
            entry["parent_spread_us"] = round(entry["parent_build"]["max_us"] - entry["parent_build"]["min_us"], 1)
            print(json.dumps(entry), flush=True)
            plain.append(entry)
        report["plain_act"] = {"unit": "us per loop step (two plain acts and the step), one window of 16 steps per process, processes alternating",
                               "cases": plain}
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
