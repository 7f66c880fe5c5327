#!/usr/bin/env python3
"""What a policy per world costs on the balance beam: the bank act (``mrl_mlpbase_act_bank``: the plan and the act over its tiles)
against the plain act (``mrl_mlpbase_act``) in the rollout loop, us per loop step, written to profiles/mlpbase_bank_cost.json under
the library's build hash.

    python tools/mlpbase_bank_probe.py                          measure (needs the GPU)
    python tools/mlpbase_bank_probe.py --parent-tree DIR        also the plain act of this build against the build in DIR

1024 and 32768 worlds.  Every comparison runs its two sides in ALTERNATING windows of T = 128 loop steps, five windows each after
one that warms both up; medians and extremes are reported as they come, nothing is asserted.
  a  ``k1``      ``env.rollout_bank`` under a bank of one (ids all 0) against ``env.rollout`` under the same policy: the price of the
                 plan and of the indirection, everything else being equal.
  b  ``k4``      ``env.rollout_bank`` under a bank of four with random ids (and a random resample behind every step) against four
                 environments of N / 4 worlds, each under ``env.rollout`` with one of the four policies, one after the other on the
                 same stream -- the only way without a bank.
  c  ``cross``   the 4 x 4 cross-play loop step, ``mlpbase_act_bank`` + ``sim.step()`` on one environment whose world n plays pair n
                 mod 16, against sixteen environments of N / 16 worlds with two ``mlpbase_act`` (one per seat) and a step each.
  d  ``plain_act``   with ``--parent-tree``: ``env.rollout`` (the plain act and the step) of this build against the same call of the
                 build in DIR, a checkout of the parent commit with its library built, in ALTERNATING PROCESSES, a window each.  The
                 act body became a template for the bank; the plain act must not have paid for it.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "mlpbase_bank_cost.json")
SIZES = (1024, 32768)
WINDOWS, T, K = 5, 128, 4
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


def make_policies(count, device):
    import torch
    from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic, MlpBasePolicy
    policies = []
    for seed in range(count):
        torch.manual_seed(seed)
        policies.append(MlpBasePolicy.from_module(MlpBaseActorCritic(), device=device))
    return policies


def measure(n):
    import torch
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    from madrona_rl_envs_playground_amd.simulators import CnnResample, MlpBasePolicyBank, MlpBaseRecord, mlpbase_act, mlpbase_act_bank
    device = torch.device("cuda", 0)

    def make(worlds):
        return BalanceMadronaTorch(worlds, 0), MlpBaseRecord(T, worlds, 2, device)

    env, record = make(n)
    policies = make_policies(K, device)
    bank1, bank4 = MlpBasePolicyBank.from_policies(policies[:1]), MlpBasePolicyBank.from_policies(policies)
    ids_record = torch.empty((T + 1, n, 2), dtype=torch.int32, device=device)
    step = {"at": 0}

    def numbered(fn):
        def window():
            fn(step["at"])
            step["at"] += T
        return window

    out = {"worlds": n, "steps_per_window": T, "policies": K}

    # a: a bank of one against the plain rollout
    zeros = torch.zeros((n, 2), dtype=torch.int32, device=device)
    out["k1"] = alternate({
        "plain_step": numbered(lambda at: env.rollout(policies[0], T, seed=1, first_step=at, record=record)),
        "bank_step": numbered(lambda at: env.rollout_bank(bank1, zeros, T, seed=1, first_step=at, record=record, ids_record=ids_record)),
    })

    # b: four policies over the worlds at random, resampled at every episode's end, against four environments of N / 4
    ids = torch.randint(0, K, (n, 2), generator=torch.Generator().manual_seed(0), dtype=torch.int32).to(device)
    episodes = torch.zeros(n, dtype=torch.int32, device=device)
    resample = CnnResample("random", 0, K, 2, seed=2)
    quarters = [make(n // K) for _ in range(K)]

    def four(at):
        for (e, r), policy in zip(quarters, policies):
            e.rollout(policy, T, seed=1, first_step=at, record=r)

    out["k4"] = alternate({
        "four_simulators_step": numbered(four),
        "bank_step": numbered(lambda at: env.rollout_bank(bank4, ids, T, episodes=episodes, resample=resample, seed=1, first_step=at,
                                                          record=record, ids_record=ids_record)),
    })
    for e, _ in quarters:
        e.close()
    del quarters

    # c: the 4 x 4 cross-play loop step against sixteen environments
    pair = torch.arange(n, device=device) % (K * K)
    pair_ids = torch.stack([pair // K, pair % K], dim=1).to(torch.int32).contiguous()
    sixteenths = [BalanceMadronaTorch(n // (K * K), 0) for _ in range(K * K)]

    def sixteen(at):
        for t in range(T):
            for i, e in enumerate(sixteenths):
                mlpbase_act(e.sim, policies[i // K], 0b01, seed=1, step=at + t, greedy=True)
                mlpbase_act(e.sim, policies[i % K], 0b10, seed=1, step=at + t, greedy=True)
                e.sim.step()

    def banked(at):
        for t in range(T):
            mlpbase_act_bank(env.sim, bank4, pair_ids, seed=1, step=at + t, greedy=True)
            env.sim.step()

    out["cross"] = alternate({"sixteen_simulators_step": numbered(sixteen), "bank_step": numbered(banked)})
    for e in sixteenths:
        e.close()
    env.close()
    return out


def plain_window(n):
    """one window of the plain rollout in this process, after one that warms up -> us per loop step"""
    import torch
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    from madrona_rl_envs_playground_amd.simulators import MlpBaseRecord
    device = torch.device("cuda", 0)
    env, record = BalanceMadronaTorch(n, 0), MlpBaseRecord(T, n, 2, device)
    policy = make_policies(1, device)[0]
    env.rollout(policy, T, seed=1, first_step=0, record=record)
    us = timed(lambda: env.rollout(policy, T, seed=1, first_step=T, record=record))
    env.close()
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
    report = {"build_hash": _lib.source_hash(), "unit": "us per loop step (both seats act, then the step)", "windows": WINDOWS,
              "steps_per_window": T, "cases": results}
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
        report["plain_act"] = {"unit": "us per loop step of env.rollout, one window of 128 steps per process, processes alternating",
                               "cases": plain}
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
