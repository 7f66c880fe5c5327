#!/usr/bin/env python3
"""What episode statistics on the device cost (mrl_enable_episode_stats): us per step, written to
profiles/episode_stats_cost.json under the library's build hash.

    python tools/episode_stats_probe.py --build-variants [--parent REV]   compile the other builds (hipcc, no GPU needed)
    python tools/episode_stats_probe.py                                   measure (needs the GPU and those builds)

Three builds take part, each loaded by a process of its own (MRL_ENVS_LIB) that stays alive for the whole session, so
that the builds ALTERNATE window by window on the same GPU:
  new      the library of this tree;
  general  the same sources with -DMRL_STATS_GENERAL_ONLY: Cartpole, Acrobot and the balance beam take the statistics
           with the general update launch behind the step instead of inside their single-launch step;
  parent   the parent commit (REV, default HEAD~1): its csrc/ and Python package extracted with `git archive` into
           madrona_rl_envs_playground_amd/variants/parent_tree and built there with the Makefile's OUT= / OBJDIR=.
Two questions:
  1. statistics NOT enabled: does the step cost what the parent's costs?  `new_plain` against `parent_plain`; the margin is
     the spread (max - min) of the parent build's own repeated windows in this session.
  2. statistics enabled: `in_kernel` (new) and `general_launch` (general; for Overcooked the new build itself) against
     `parent_torch_lines` -- the parent's plain step followed by the four torch lines with which the reference's training
     scripts keep episode returns (scripts/cartpole_train_torch.py:223-226), i.e. what a user does today.
What is timed: `steps` calls of step_with_actions over a pool of eight action tensors between two device events, after a
warm-up of the same calls; `repeats` rounds over all builds and forms, the median and the extremes reported."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "madrona_rl_envs_playground_amd")
VARIANTS = os.path.join(PKG, "variants")
PARENT_TREE = os.path.join(VARIANTS, "parent_tree")
LIBS = {"new": os.path.join(PKG, "libmrl_envs.so"), "general": os.path.join(VARIANTS, "libmrl_envs_stats_general.so"),
        "parent": os.path.join(VARIANTS, "libmrl_envs_parent.so")}
OUT = os.path.join(REPO, "profiles", "episode_stats_cost.json")
CONFIGS = [("cartpole", 1024), ("cartpole", 1 << 20), ("acrobot", 1024), ("acrobot", 1 << 20), ("balance", 1024), ("balance", 1 << 20),
           ("overcooked", 32768)]
# (build, form) -> row name; the order of a round
FORMS = [("parent", "plain", "parent_plain"), ("new", "plain", "new_plain"), ("parent", "torch_lines", "parent_torch_lines"),
         ("new", "stats", "in_kernel"), ("general", "stats", "general_launch")]


def build_variants(parent_rev):
    jobs = str(min(6, os.cpu_count() or 1))
    os.makedirs(PARENT_TREE, exist_ok=True)
    archive = subprocess.run(["git", "-C", REPO, "archive", parent_rev, "madrona_rl_envs_playground_amd", "include"], check=True,
                             capture_output=True).stdout
    subprocess.run(["tar", "-x", "-C", PARENT_TREE], input=archive, check=True)
    subprocess.run(["make", "-C", os.path.join(PARENT_TREE, "madrona_rl_envs_playground_amd", "csrc"), "-j", jobs, "OUT=" + LIBS["parent"],
                    "OBJDIR=" + os.path.join(VARIANTS, "obj_parent")], check=True)
    subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j", jobs, "OUT=../variants/libmrl_envs_stats_general.so",
                    "OBJDIR=../variants/obj_stats_general", "EXTRA_CXXFLAGS=-DMRL_STATS_GENERAL_ONLY"], check=True)
    for lib in LIBS.values():
        print(lib, os.path.exists(lib))


# ---- a child: one build, loaded once, answers one window per request line -------------------------------------------
def child(tree, steps, warmup):
    sys.path.insert(0, tree)
    import torch
    from madrona_rl_envs_playground_amd import _lib, layouts, simulators as S
    made = {}

    def make(game, n, stats):
        key = (game, n, stats)
        if key in made:
            return made[key]
        g = torch.Generator().manual_seed(n)
        if game == "cartpole":
            sim, high, shape = S.CartpoleSimulator(exec_mode=S.ExecMode.CUDA, gpu_id=0, num_worlds=n), 2, (n, 1)
        elif game == "acrobot":
            sim, high, shape = S.AcrobotSimulator(exec_mode=S.ExecMode.CUDA, gpu_id=0, num_worlds=n), 3, (n, 1)
        elif game == "balance":
            sim, high, shape = S.BalanceBeamSimulator(exec_mode=S.ExecMode.CUDA, gpu_id=0, num_worlds=n), 4, (2, n, 1)
        else:
            params = layouts.get_base_layout_params("cramped_room", 400)
            sim, high, shape = S.OvercookedSimulator(exec_mode=S.ExecMode.CUDA, gpu_id=0, num_worlds=n, **params), 6, (2, n, 1)
        pool = [torch.randint(0, high, shape, dtype=torch.int32, generator=g).cuda() for _ in range(8)]
        if stats:
            sim.enable_episode_stats()
        made[key] = (sim, pool)
        return made[key]

    def window(game, n, form):
        sim, pool = make(game, n, form == "stats")
        after = None
        if form == "torch_lines":
            rewards = sim.reward_tensor().to_torch()
            next_done = (sim.reset_tensor() if hasattr(sim, "reset_tensor") else sim.done_tensor()).to_torch()
            ep_rewards = torch.zeros_like(rewards)
            rewsum = torch.zeros((), dtype=rewards.dtype, device="cuda")
            numfin = torch.zeros((), dtype=next_done.dtype, device="cuda")

            def after():  # scripts/cartpole_train_torch.py:223-226 of the reference, line by line
                nonlocal ep_rewards, rewsum, numfin
                ep_rewards += rewards
                rewsum += torch.sum(torch.where(next_done == 1, ep_rewards, 0))
                numfin += torch.sum(next_done)
                ep_rewards *= 1 - next_done

        def run(count):
            for i in range(count):
                sim.step_with_actions(pool[i % 8])
                if after:
                    after()

        run(warmup)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(steps)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps * 1e3, sim.kernel_name

    print("READY " + json.dumps({"build": _lib.build_hash()}), flush=True)
    for line in sys.stdin:
        request = json.loads(line)
        if request.get("quit"):
            break
        us, kernel = window(request["game"], request["n"], request["form"])
        print("R " + json.dumps({"us": us, "kernel": kernel}), flush=True)
    for sim, _ in made.values():
        sim.close()


class Child:
    def __init__(self, build, steps, warmup):
        tree = PARENT_TREE if build == "parent" else REPO
        self.proc = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", tree, "--steps", str(steps), "--warmup", str(warmup)],
                                     env={**os.environ, "MRL_ENVS_LIB": LIBS[build]}, stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                     text=True, bufsize=1)
        self.build = build
        self.hash = self.read("READY ")["build"]

    def read(self, tag):
        while True:
            line = self.proc.stdout.readline()
            if not line:
                raise SystemExit(f"the process of the {self.build} build ended (exit status {self.proc.wait()})")
            if line.startswith(tag):
                return json.loads(line[len(tag):])

    def ask(self, game, n, form):
        self.proc.stdin.write(json.dumps({"game": game, "n": n, "form": form}) + "\n")
        self.proc.stdin.flush()
        return self.read("R ")

    def close(self):
        try:
            self.proc.stdin.write(json.dumps({"quit": True}) + "\n")
            self.proc.stdin.close()
        except OSError:
            pass
        self.proc.wait()


def summary(times):
    t = sorted(times)
    return {"us_per_step": [round(v, 3) for v in times], "median": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--parent", default="HEAD~1", help="the parent commit (--build-variants)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.build_variants:
        build_variants(args.parent)
        return
    if args.child:
        child(args.child, args.steps, args.warmup)
        return
    missing = [lib for lib in LIBS.values() if not os.path.exists(lib)]
    if missing:
        raise SystemExit("not built: " + ", ".join(missing) + " (tools/episode_stats_probe.py --build-variants)")
    children = {}
    try:
        for build in LIBS:
            children[build] = Child(build, args.steps, args.warmup)
        if children["general"].hash != children["new"].hash:
            raise SystemExit("the general-launch build is of other sources than the library")
        times, kernels = {}, {}
        for rep in range(args.repeats + 1):  # the first round warms every build and form up
            for game, n in CONFIGS:
                for build, form, name in FORMS:
                    if game == "overcooked" and build == "general":
                        continue  # the new build's own statistics ARE the general launch there
                    answer = children[build].ask(game, n, form)
                    kernels[(game, n, name)] = answer["kernel"]
                    if rep:
                        times.setdefault((game, n, name), []).append(answer["us"])
    finally:
        for c in children.values():
            c.close()
    rows = {}
    for game, n in CONFIGS:
        row = {name: dict(summary(times[(game, n, name)]), kernel=kernels[(game, n, name)]) for _, _, name in FORMS if (game, n, name) in times}
        if game == "overcooked":
            row["general_launch"] = row.pop("in_kernel")
        spread = row["parent_plain"]["max"] - row["parent_plain"]["min"]
        row["not_enabled"] = {"parent_spread_us": round(spread, 3),
                              "new_minus_parent_median_us": round(row["new_plain"]["median"] - row["parent_plain"]["median"], 3),
                              "within_parent_spread": row["new_plain"]["median"] - row["parent_plain"]["median"] <= spread}
        row["enabled"] = {name + "_below_torch_lines": row[name]["median"] < row["parent_torch_lines"]["median"]
                          for name in ("in_kernel", "general_launch") if name in row}
        rows[f"{game}@{n}"] = row
        print(f"{game}@{n}", json.dumps(row), flush=True)
    record = {"build_hash": children["new"].hash, "parent_build_hash": children["parent"].hash,
              "what": "us per step, device events around `steps` step_with_actions calls; `repeats` rounds alternating the builds and forms",
              "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
