#!/usr/bin/env python3
"""What training K seeds of the small PPO agent on one batch costs: one ``MlpPolicyBank`` on a simulator of K W worlds
(``rollout_bank``, ``gae``, ``ppo_update_bank``: the launches of one seed's iteration whatever K is) against K simulators of W
worlds trained one after another through ``rollout``, ``gae`` and ``ppo_update`` -- all the parent commit can do --, ms per
iteration, written to profiles/ppo_bank_cost.json under the library's build hash.

    python tools/ppo_bank_probe.py                          measure (needs the GPU)
    python tools/ppo_bank_probe.py --parent-tree DIR        also the plain calls of this build against the build in DIR

Every comparison runs its sides in ALTERNATING windows, five windows each after one that warms all sides up; medians and extremes
are reported as they come, nothing is asserted.  One iteration is a rollout of T = 128 steps, ``gae`` and an update of 4 epochs x 4
minibatches = 16 rows, on Cartpole.
  a  ``iteration``  one bank on K W worlds against K simulators of W worlds one after another: W = 1024 with K = 4 and K = 16,
                    W = 65536 with K = 4.
  b  ``plain``      with ``--parent-tree``: ``rollout_policy`` + ``gae`` + ``ppo_update`` at 1024 worlds of this build against the same
                    calls of the build in DIR, a checkout of the parent commit with its library built, in ALTERNATING PROCESSES,
                    a window each.  ``inside_parent_spread`` says whether this build's median lies at or below the parent build's
                    maximum.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "ppo_bank_cost.json")
WINDOWS, STEPS, MINIBATCHES, EPOCHS = 5, 128, 4, 4
ITERATION_CASES = ((1024, 4), (1024, 16), (65536, 4))
CASE_TIMEOUT_S = 240


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(sides):
    """{name: window function} -> {name: summary}"""
    for fn in sides.values():
        fn()  # warm-up
    times = {name: [] for name in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            times[name].append(timed(fn))
    return {name: summary(xs) for name, xs in times.items()}


def agents(k):
    import torch
    from madrona_rl_envs_playground_amd.simulators import MlpAgent
    out = []
    for seed in range(k):
        torch.manual_seed(seed)
        out.append(MlpAgent(4, 2))
    return out


def measure_iteration(w, k):
    import torch
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    from madrona_rl_envs_playground_amd.simulators import (MlpPolicy, MlpPolicyBank, PpoBankOptimizer, PpoOptimizer, gae,
                                                             member_minibatch_indices, minibatch_indices, ppo_update, ppo_update_bank)
    device = torch.device("cuda", 0)
    shuffles = torch.Generator(device=device).manual_seed(1)
    at = {"bank": 0, "small": 0}
    # (small steps: the windows go on training the same weights)
    env = CartpoleMadronaTorch(k * w, 0)
    bank = MlpPolicyBank.from_modules(agents(k), device=device)
    optimizer = PpoBankOptimizer(bank, lr=1e-5)
    kept = {"rollout": None}

    def banked():
        rollout = kept["rollout"] = env.rollout_bank(bank, STEPS, seed=1, first_step=at["bank"], out=kept["rollout"])
        at["bank"] += STEPS
        advantages, returns = gae(rollout, 0.99, 0.95)
        indices = member_minibatch_indices(STEPS, k * w, k, MINIBATCHES, EPOCHS, generator=shuffles, device=device)
        ppo_update_bank(bank, optimizer, rollout, advantages, returns, indices)

    # the only way without the bank calls: a simulator of W worlds per seed, each trained through the plain calls
    members = []
    for agent in agents(k):
        policy = MlpPolicy.from_module(agent, device=device)
        members.append({"env": CartpoleMadronaTorch(w, 0), "policy": policy, "optimizer": PpoOptimizer(policy, lr=1e-5), "rollout": None})

    def one_by_one():
        for m in members:
            rollout = m["rollout"] = m["env"].rollout(m["policy"], STEPS, seed=1, first_step=at["small"], out=m["rollout"])
            advantages, returns = gae(rollout, 0.99, 0.95)
            indices = minibatch_indices(STEPS * w, MINIBATCHES, EPOCHS, generator=shuffles, device=device)
            ppo_update(m["policy"], m["optimizer"], rollout, advantages, returns, indices)
        at["small"] += STEPS

    out = {"game": "cartpole", "worlds_per_member": w, "members": k, "num_steps": STEPS, "rows": MINIBATCHES * EPOCHS,
           "minibatch_size": STEPS * w // MINIBATCHES}
    out.update(alternate({"simulators_one_by_one": one_by_one, "bank_on_one_batch": banked}))
    out["bank_over_one_by_one"] = round(out["bank_on_one_batch"]["median_ms"] / out["simulators_one_by_one"]["median_ms"], 3)
    out["parameters_finite"] = bool(torch.isfinite(bank.params).all())
    for m in members:
        m["env"].close()
    env.close()
    return out


def plain_window():
    """one window of the plain iteration in this process, after one that warms up -> ms; only calls the parent commit has"""
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    env = CartpoleMadronaTorch(1024, 0)
    policy = S.MlpPolicy.from_module(S.MlpAgent(4, 2).cuda())
    optimizer = S.PpoOptimizer(policy, lr=1e-5)
    shuffles = torch.Generator(device=device).manual_seed(1)
    kept = {"rollout": None, "at": 0}

    def window():
        rollout = kept["rollout"] = env.rollout(policy, STEPS, seed=1, first_step=kept["at"], out=kept["rollout"])
        kept["at"] += STEPS
        advantages, returns = S.gae(rollout, 0.99, 0.95)
        indices = S.minibatch_indices(STEPS * 1024, MINIBATCHES, EPOCHS, generator=shuffles, device=device)
        S.ppo_update(policy, optimizer, rollout, advantages, returns, indices)

    window()
    ms = timed(window)
    env.close()
    return ms


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
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: measure the plain calls against it")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)  # a child imports the package from here
    ap.add_argument("--iteration-case", nargs=2, help=argparse.SUPPRESS)
    ap.add_argument("--plain-window", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    from madrona_rl_envs_playground_amd import _lib
    if args.iteration_case is not None:
        print(json.dumps(measure_iteration(int(args.iteration_case[0]), int(args.iteration_case[1]))), flush=True)
        return 0
    if args.plain_window:
        print(json.dumps({"ms": plain_window(), "build_hash": _lib.build_hash()}), flush=True)
        return 0
    report = {"build_hash": _lib.source_hash(), "windows": WINDOWS,
              "unit": "ms per iteration: a rollout of 128 steps, gae and 16 update rows (device events around the whole window)", "iteration": []}
    for case in ITERATION_CASES:
        status, result = child(["--iteration-case"] + [str(x) for x in case])
        if status:
            print(f"iteration {case} ended with status {status}: nothing more is started", file=sys.stderr)
            return status
        print("iteration", json.dumps(result), flush=True)
        report["iteration"].append(result)
    if args.parent_tree:
        times, hashes = {"this_build": [], "parent_build": []}, {}
        for _ in range(WINDOWS):
            for name, tree in (("parent_build", os.path.abspath(args.parent_tree)), ("this_build", REPO)):
                status, result = child(["--plain-window"], tree)
                if status:
                    print(f"the plain iteration of {name} ended with status {status}: nothing more is started", file=sys.stderr)
                    return status
                times[name].append(result["ms"])
                hashes[name] = result["build_hash"]
        entry = {"calls": "rollout_policy, gae, ppo_update", "game": "cartpole", "worlds": 1024, "build_hashes": hashes,
                 "unit": "ms per plain iteration, one window per process, processes alternating"}
        entry.update({name: summary(xs) for name, xs in times.items()})
        entry["inside_parent_spread"] = entry["this_build"]["median_ms"] <= entry["parent_build"]["max_ms"]
        print("plain", json.dumps(entry), flush=True)
        report["plain"] = entry
    else:
        report["plain"] = "NOT MEASURED (no --parent-tree)"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
    print("->", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
