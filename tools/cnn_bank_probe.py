#!/usr/bin/env python3
"""What a policy per world costs: the bank act (``mrl_cnn_act_bank``: the plan launch and the act over its tiles) against the
plain act (``mrl_cnn_act``) in the rollout loop, us per loop step, written to profiles/cnn_bank_cost.json under the library's
build hash.

    python tools/cnn_bank_probe.py           measure (needs the GPU)

cramped_room at 1024 and 32768 worlds.  Every comparison runs its two sides in ALTERNATING windows of T = 128 loop steps, five
windows each after one that warms both up; medians and extremes are reported as they come, nothing is asserted.
  a  ``k1``      ``env.rollout_bank`` under a bank of one (ids all 0) against ``env.rollout`` under the same policy: the price of the
                 plan launch and of the indirection, everything else being equal.
  b  ``k4``      ``env.rollout_bank`` under a bank of four with random ids (and a random resample behind every step) against four
                 environments of N / 4 worlds, each under ``env.rollout`` with one of the four policies, one after the other on the
                 same stream -- the only way without a bank.
  c  ``cross``   the 4 x 4 cross-play loop step, ``cnn_act_bank`` + ``sim.step()`` on one environment whose world n plays pair n mod
                 16, against sixteen environments of N / 16 worlds with two ``cnn_act`` (one per seat) and a step each.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "cnn_bank_cost.json")
LAYOUT, SIZES = "cramped_room", (1024, 32768)
WINDOWS, T, K = 5, 128, 4
CASE_TIMEOUT_S = 300


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def alternate(sides):
    """{name: window function} -> {name: summary}; a window is T loop steps"""
    import torch

    def timed(fn):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e6 / T

    for fn in sides.values():
        fn()  # warm-up
    times = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            times[name].append(timed(fn))
    return {name: summary(xs) for name, xs in times.items()}


def measure(n):
    import torch
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnPolicyBank, CnnRecord, CnnResample, cnn_act, cnn_act_bank
    device = torch.device("cuda", 0)

    def make(worlds):
        env = OvercookedMadrona(LAYOUT, worlds, 0)
        record = CnnRecord(T, worlds, env.num_players, device)
        ring = torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=device)
        return env, record, ring

    env, record, ring = make(n)
    w, h, f = env.width, env.height, 5 * env.num_players + 16
    policies = []
    for seed in range(K):
        torch.manual_seed(seed)
        policies.append(CnnPolicy.from_module(CnnActorCritic(w, h, f), device=device))
    bank1, bank4 = CnnPolicyBank.from_policies(policies[:1]), CnnPolicyBank.from_policies(policies)
    ids_record = torch.empty((T + 1, n, 2), dtype=torch.int32, device=device)
    step = {"at": 0}

    def numbered(fn):
        def window():
            fn(step["at"])
            step["at"] += T
        return window

    out = {"layout": LAYOUT, "worlds": n, "steps_per_window": T, "policies": K}

    # a: a bank of one against the plain rollout
    zeros = torch.zeros((n, 2), dtype=torch.int32, device=device)
    out["k1"] = alternate({
        "plain_step": numbered(lambda at: env.rollout(policies[0], T, seed=1, first_step=at, record=record, ring=ring)),
        "bank_step": numbered(lambda at: env.rollout_bank(bank1, zeros, T, seed=1, first_step=at, record=record, ring=ring, ids_record=ids_record)),
    })

    # b: four policies over the worlds at random, resampled at every episode's end, against four environments of N / 4
    ids = torch.randint(0, K, (n, 2), generator=torch.Generator().manual_seed(0), dtype=torch.int32).to(device)
    episodes = torch.zeros(n, dtype=torch.int32, device=device)
    resample = CnnResample("random", 0, K, 2, seed=2)
    quarters = [make(n // K) for _ in range(K)]

    def four(at):
        for (e, r, g), policy in zip(quarters, policies):
            e.rollout(policy, T, seed=1, first_step=at, record=r, ring=g)

    out["k4"] = alternate({
        "four_simulators_step": numbered(four),
        "bank_step": numbered(lambda at: env.rollout_bank(bank4, ids, T, episodes=episodes, resample=resample, seed=1, first_step=at, record=record,
                                                          ring=ring, ids_record=ids_record)),
    })
    for e, _, _ in quarters:
        e.close()
    del quarters

    # c: the 4 x 4 cross-play loop step against sixteen environments
    pair = torch.arange(n, device=device) % (K * K)
    pair_ids = torch.stack([pair // K, pair % K], dim=1).to(torch.int32).contiguous()
    sixteenths = [OvercookedMadrona(LAYOUT, n // (K * K), 0) for _ in range(K * K)]

    def sixteen(at):
        for t in range(T):
            for i, e in enumerate(sixteenths):
                cnn_act(e.sim, policies[i // K], 0b01, seed=1, step=at + t, greedy=True)
                cnn_act(e.sim, policies[i % K], 0b10, seed=1, step=at + t, greedy=True)
                e.sim.step()

    def banked(at):
        for t in range(T):
            cnn_act_bank(env.sim, bank4, pair_ids, seed=1, step=at + t, greedy=True)
            env.sim.step()

    out["cross"] = alternate({"sixteen_simulators_step": numbered(sixteen), "bank_step": numbered(banked)})
    for e in sixteenths:
        e.close()
    env.close()
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        print(json.dumps(measure(int(sys.argv[2]))), flush=True)
        return 0
    from madrona_rl_envs_playground_amd import _lib
    results = []
    for n in SIZES:
        proc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--case", str(n)],
                              capture_output=True, text=True)
        if proc.returncode != 0:
            print(proc.stdout + proc.stderr, file=sys.stderr)
            print(f"{LAYOUT} at {n} worlds ended with status {proc.returncode}: nothing more is started", file=sys.stderr)
            return proc.returncode
        line = [x for x in proc.stdout.splitlines() if x.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    report = {"build_hash": _lib.source_hash(), "unit": "us per loop step (both seats act, then the step)", "windows": WINDOWS,
              "steps_per_window": T, "cases": results}
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
