#!/usr/bin/env python3
"""What training a population in one call costs: ``mappo_update_bank`` (``mrl_mappo_bank_update``, ``mrl_mappo_mlp_bank_update``:
2 + 3 R launches for every member together) against the members one after another through ``mappo_update``, ms per update, written
to profiles/bank_update_cost.json under the library's build hash.

    python tools/bank_update_probe.py                          measure (needs the GPU)
    python tools/bank_update_probe.py --parent-tree DIR        also the plain updates of this build against the build in DIR

Every comparison runs its sides in ALTERNATING windows, five windows each after one that warms all sides up; medians and extremes
are reported as they come, nothing is asserted.  An update is R = 15 rows (15 epochs, one minibatch) over each member's own
samples of one bank rollout (world n under member n mod K, both seats; T = 200 steps on the beam, 128 in the kitchen).
  a  ``update``     one ``mappo_update_bank`` of K members against K ``mappo_update`` calls in sequence (each through
                    ``optimizer.member(k)`` and ``value_norms.member(k)``) on the same index rows: the beam at 1024 worlds with K =
                    4 and K = 16 and at 8192 worlds with K = 4, ``cramped_room`` at 1024 worlds with K = 4.
  b  ``iteration``  rollout, advantages and update of the population on one batch of 1024 worlds (``rollout_bank``,
                    ``mappo_advantages_bank``, ``mappo_update_bank``) against K = 4 simulators of 256 worlds trained one after
                    another (``rollout``, ``mappo_advantages``, ``mappo_update``), both families.
  c  ``plain``      with ``--parent-tree``: ``mappo_update`` (beam and ``cramped_room``, 1024 worlds, 15 rows) and ``ppo_update``
                    (Cartpole, 1024 worlds, 16 rows; it shares the optimiser tail) of this build against the same calls of the
                    build in DIR, a checkout of the parent commit with its library built, in ALTERNATING PROCESSES, a window
                    each.  ``inside_parent_spread`` says whether this build's median lies at or below the parent build's maximum.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "bank_update_cost.json")
WINDOWS, ROWS = 5, 15
STEPS = {"balance": 200, "overcooked": 128}
UPDATE_CASES = (("balance", 1024, 4), ("balance", 1024, 16), ("balance", 8192, 4), ("overcooked", 1024, 4))
ITERATION_CASES = (("balance", 1024, 4), ("overcooked", 1024, 4))
PLAIN_CASES = ("balance", "overcooked", "cartpole")
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


def population(game, n, k):
    """-> (tool, env, bank, owner, cells): the training tool's env and bank of K seeds and the members' samples"""
    import torch
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import population_train_device as tool
    from madrona_rl_envs_playground_amd.simulators import member_samples
    env = tool.make_env(game, n)
    bank = tool.make_bank(game, env, list(range(k)))
    owner = (torch.arange(n, device=bank.params.device) % k).view(n, 1).expand(n, 2).to(torch.int32).contiguous()
    return tool, env, bank, owner, member_samples(owner, range(k), STEPS[game])


def bank_rollout(game, env, bank, owner, at, buffers):
    """one ``rollout_bank`` into ``buffers`` (kept from call to call) -> (record, ring or None)"""
    if game == "balance":
        buffers["record"], buffers["ids"] = env.rollout_bank(bank, owner, STEPS[game], seed=1, first_step=at, record=buffers.get("record"),
                                                             ids_record=buffers.get("ids"))
        return buffers["record"], None
    buffers["record"], buffers["ring"], buffers["ids"] = env.rollout_bank(bank, owner, STEPS[game], seed=1, first_step=at,
                                                                          record=buffers.get("record"), ring=buffers.get("ring"),
                                                                          ids_record=buffers.get("ids"))
    return buffers["record"], buffers["ring"]


def measure_update(game, n, k):
    import torch
    from madrona_rl_envs_playground_amd.simulators import (MappoBankOptimizer, ValueNormBank, mappo_advantages_bank, mappo_update,
                                                             mappo_update_bank)
    tool, env, bank, owner, cells = population(game, n, k)
    record, ring = bank_rollout(game, env, bank, owner, 0, {})
    norms = ValueNormBank(k, bank.params.device)
    advantages, returns = mappo_advantages_bank(record, cells, norms)
    indices = tool.member_rows(cells, ROWS, 1, torch.Generator(device=bank.params.device).manual_seed(1))
    optimizer = MappoBankOptimizer(bank, lr=1e-5, critic_lr=1e-5)  # (small steps: the windows repeat on one record)
    rows = [indices[z].contiguous() for z in range(k)]
    alone = [(bank.policy(z), optimizer.member(z), norms.member(z)) for z in range(k)]  # views of the bank's rows, made once

    def banked():
        mappo_update_bank(bank, optimizer, record, ring, advantages, returns, indices, norms)

    def sequential():
        for (policy, member, norm), own in zip(alone, rows):
            mappo_update(policy, member, record, ring, advantages, returns, own, value_norm=norm)

    out = {"game": game, "worlds": n, "members": k, "rows": ROWS, "minibatch_size": int(indices.shape[2])}
    out.update(alternate({"sequential_updates": sequential, "bank_update": banked}))
    out["bank_over_sequential"] = round(out["bank_update"]["median_ms"] / out["sequential_updates"]["median_ms"], 3)
    out["parameters_finite"] = bool(torch.isfinite(bank.params).all())
    env.close()
    return out


def measure_iteration(game, n, k):
    import torch
    from madrona_rl_envs_playground_amd.simulators import (MappoBankOptimizer, MappoOptimizer, ValueNorm, ValueNormBank, mappo_advantages,
                                                             mappo_advantages_bank, mappo_update, mappo_update_bank, minibatch_indices)
    tool, env, bank, owner, cells = population(game, n, k)
    device = bank.params.device
    optimizer, norms = MappoBankOptimizer(bank, lr=1e-5, critic_lr=1e-5), ValueNormBank(k, device)
    shuffles = torch.Generator(device=device).manual_seed(1)
    buffers, at = {}, {"bank": 0, "small": 0}
    steps = STEPS[game]

    def banked():
        record, ring = bank_rollout(game, env, bank, owner, at["bank"], buffers)
        at["bank"] += steps
        advantages, returns = mappo_advantages_bank(record, cells, norms)
        mappo_update_bank(bank, optimizer, record, ring, advantages, returns, tool.member_rows(cells, ROWS, 1, shuffles), norms)

    # the only way without the bank calls: a simulator of N / K worlds per member, each trained through the plain calls
    small = tool.make_bank(game, env, list(range(k)))
    members = []
    for z in range(k):
        members.append({"env": tool.make_env(game, n // k), "policy": small.policy(z), "optimizer": MappoOptimizer(small.policy(z), 1e-5, 1e-5),
                        "norm": ValueNorm(device), "record": None, "ring": None})

    def one_by_one():
        for m in members:
            if game == "balance":
                m["record"] = m["env"].rollout(m["policy"], steps, seed=1, first_step=at["small"], record=m["record"])
            else:
                m["record"], m["ring"] = m["env"].rollout(m["policy"], steps, seed=1, first_step=at["small"], record=m["record"], ring=m["ring"])
            advantages, returns = mappo_advantages(m["record"], m["norm"])
            indices = minibatch_indices(steps * (n // k) * 2, 1, ROWS, generator=shuffles, device=device)
            mappo_update(m["policy"], m["optimizer"], m["record"], m["ring"], advantages, returns, indices, value_norm=m["norm"])
        at["small"] += steps

    out = {"game": game, "worlds": n, "members": k, "rows": ROWS, "num_steps": steps}
    out.update(alternate({"simulators_one_by_one": one_by_one, "population_on_one_batch": banked}))
    out["bank_over_one_by_one"] = round(out["population_on_one_batch"]["median_ms"] / out["simulators_one_by_one"]["median_ms"], 3)
    for m in members:
        m["env"].close()
    env.close()
    return out


def plain_window(what):
    """one window of a plain update in this process, after one that warms up -> ms; only calls the parent commit has"""
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    device = torch.device("cuda", 0)
    torch.manual_seed(1)
    if what == "cartpole":
        from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
        env = CartpoleMadronaTorch(1024, 0)
        policy = S.MlpPolicy.from_module(S.MlpAgent(4, 2).cuda())
        rollout = env.rollout(policy, 128)
        advantages, returns = S.gae(rollout, 0.99, 0.95)
        optimizer = S.PpoOptimizer(policy, lr=1e-5)
        indices = S.minibatch_indices(128 * 1024, 4, 4, generator=torch.Generator(device=device).manual_seed(1), device=device)
        window = lambda: S.ppo_update(policy, optimizer, rollout, advantages, returns, indices)  # noqa: E731
    else:
        steps = STEPS[what]
        if what == "balance":
            from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
            env = BalanceMadronaTorch(1024, 0)
            policy = S.MlpBasePolicy.from_module(S.MlpBaseActorCritic(), device=device)
            record, ring = env.rollout(policy, steps, seed=1), None
        else:
            from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
            env = OvercookedMadrona("cramped_room", 1024, 0, horizon=400)
            _, _, height, width, channels = env.static_world_major_observations.shape
            policy = S.CnnPolicy.from_module(S.CnnActorCritic(width, height, channels), device=device)
            record, ring = env.rollout(policy, steps, seed=1)
        norm = S.ValueNorm(device)
        advantages, returns = S.mappo_advantages(record, norm)
        optimizer = S.MappoOptimizer(policy, lr=1e-5, critic_lr=1e-5)
        indices = S.minibatch_indices(steps * 1024 * 2, 1, ROWS, generator=torch.Generator(device=device).manual_seed(1), device=device)
        window = lambda: S.mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=norm)  # noqa: E731
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
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: measure the plain updates against it")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--tree", default=REPO, help=argparse.SUPPRESS)  # a child imports the package from here
    ap.add_argument("--update-case", nargs=3, help=argparse.SUPPRESS)
    ap.add_argument("--iteration-case", nargs=3, help=argparse.SUPPRESS)
    ap.add_argument("--plain-window", help=argparse.SUPPRESS)
    args = ap.parse_args()
    sys.path.insert(0, args.tree)
    from madrona_rl_envs_playground_amd import _lib
    for case, measure in ((args.update_case, measure_update), (args.iteration_case, measure_iteration)):
        if case is not None:
            print(json.dumps(measure(case[0], int(case[1]), int(case[2]))), flush=True)
            return 0
    if args.plain_window is not None:
        print(json.dumps({"ms": plain_window(args.plain_window), "build_hash": _lib.build_hash()}), flush=True)
        return 0
    report = {"build_hash": _lib.source_hash(), "unit": "ms per update of 15 rows (device events around the whole window)", "windows": WINDOWS}
    for key, flag, cases in (("update", "--update-case", UPDATE_CASES), ("iteration", "--iteration-case", ITERATION_CASES)):
        report[key] = []
        for case in cases:
            status, result = child([flag] + [str(x) for x in case])
            if status:
                print(f"{key} {case} ended with status {status}: nothing more is started", file=sys.stderr)
                return status
            print(key, json.dumps(result), flush=True)
            report[key].append(result)
    if args.parent_tree:
        report["plain"] = {"unit": "ms per plain update, one window per process, processes alternating", "cases": []}
        for what in PLAIN_CASES:
            times, hashes = {"this_build": [], "parent_build": []}, {}
            for _ in range(WINDOWS):
                for name, tree in (("parent_build", os.path.abspath(args.parent_tree)), ("this_build", REPO)):
                    status, result = child(["--plain-window", what], tree)
                    if status:
                        print(f"the plain update ({what}) of {name} ended with status {status}: nothing more is started", file=sys.stderr)
                        return status
                    times[name].append(result["ms"])
                    hashes[name] = result["build_hash"]
            entry = {"call": "ppo_update" if what == "cartpole" else "mappo_update", "game": what, "worlds": 1024, "build_hashes": hashes}
            entry.update({name: summary(xs) for name, xs in times.items()})
            entry["inside_parent_spread"] = entry["this_build"]["median_ms"] <= entry["parent_build"]["max_ms"]
            print("plain", json.dumps(entry), flush=True)
            report["plain"]["cases"].append(entry)
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
