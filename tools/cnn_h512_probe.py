#!/usr/bin/env python3
"""What one step of the MAPPO-style rollout loop in a kitchen costs at the reference trainer's hidden_size 512 with the policy on the
device (mrl_cnn_act_h512) against the torch loop of the same ``CnnActorCritic(hidden=512)`` on the same simulator: us per loop step,
written to profiles/cnn_h512_cost.json under the library's build hash.

    python tools/cnn_h512_probe.py                        measure (needs the GPU)
    python tools/cnn_h512_probe.py --plain TREE           also the plain hidden-64 rollout, this build against the package built in
                                                          TREE (a checkout of the parent commit), one window per process, alternating

One loop step is the act for both seats plus the step into the ring's next slot.  Two loops over the same environment, in
ALTERNATING windows of T = 128 steps, five windows each after one that warms both up, medians and extremes reported:
  torch    both nets of the module on the slot's (N P, W, H, F) view, ``Categorical.sample``, ``env.n_step(actions, out=next slot)``;
  device   ``env.rollout(policy, T)`` (mrl_rollout_cnn): per step one launch for both seats and both nets, then the ordinary step.
Sizes: cramped_room at 1024 and 32768 worlds, asymmetric_advantages at 1024.
``floor_us``: the arithmetic floor of the two nets, multiply-adds x 2 flop x samples at the 155 TF f32 matrix peak (DESIGN.md
section 15's way).  ``winner``: the side whose median is lower; ``apart``: by more than the two loops' spreads (max - min) added.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MRL_PROBE_TREE") or REPO)  # a --plain child of the other tree imports that tree's package
OUT = os.path.join(REPO, "profiles", "cnn_h512_cost.json")
CASES = (("cramped_room", 1024), ("cramped_room", 32768), ("asymmetric_advantages", 1024))
PLAIN_CASE = ("cramped_room", 32768)
WINDOWS, T = 5, 128
CASE_TIMEOUT_S = 300
PEAK_F32_MATRIX = 155e12


def summary(xs):
    return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    start = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - start) * 1e6 / T


def setup(layout, n, hidden):
    import torch
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnRecord
    device = torch.device("cuda", 0)
    env = OvercookedMadrona(layout, n, 0, horizon=400)
    w, h, p = env.width, env.height, env.num_players
    torch.manual_seed(0)
    policy = CnnPolicy.from_module(CnnActorCritic(w, h, 5 * p + 16, hidden=hidden), device=device)
    ring = torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=device)
    return env, policy, CnnRecord(T, n, p, device), ring


def measure(layout, n):
    import torch
    env, policy, record, ring = setup(layout, n, 512)
    w, h, p, f = env.width, env.height, env.num_players, policy.channels
    module, state = policy.module(), {"step": 0, "last": env.static_world_major_observations}
    values = torch.empty((T, n * p), device=ring.device)

    @torch.no_grad()
    def torch_window():
        ring[0].copy_(state["last"])
        state["last"] = ring[T]  # where this window's last step writes, and where a rollout leaves the state's observations
        for k in range(T):
            x = ring[k].view(n * p, h, w, f).transpose(1, 2).float()
            logits = module.actor(x)
            values[k] = module.critic(x)[:, 0]
            actions = torch.distributions.Categorical(logits=logits).sample().view(n, p).t().contiguous().unsqueeze(-1)
            env.n_step(actions, out=ring[k + 1])

    def device_window():
        env.rollout(policy, T, seed=1, first_step=state["step"], record=record, ring=ring)
        state["step"] += T

    torch_window(), device_window()  # warm-up
    times = {"torch_step": [], "device_step": []}
    for _ in range(WINDOWS):
        times["torch_step"].append(timed(torch_window))
        times["device_step"].append(timed(device_window))
    env.close()
    npos = (w - 2) * (h - 2)
    macs = npos * 256 * 9 * f + 256 * npos * 512 + 512 * 512 + 512 * 6  # one net; the critic's head is smaller
    out = {"layout": layout, "worlds": n, "steps_per_window": T, "samples_per_step": n * p, "multiply_adds_per_net": macs,
           "floor_us": round(2 * macs * 2 * n * p / PEAK_F32_MATRIX * 1e6, 1)}
    out.update({k: summary(v) for k, v in times.items()})
    dev, ref = times["device_step"], times["torch_step"]
    low, high = (dev, ref) if statistics.median(dev) <= statistics.median(ref) else (ref, dev)
    out["winner"] = "device" if low is dev else "torch"
    out["apart"] = statistics.median(low) + (max(dev) - min(dev)) + (max(ref) - min(ref)) < statistics.median(high)
    return out


def plain_window(layout, n):
    """one window of the hidden-64 rollout with the package this process imported, after a warm-up window"""
    env, policy, record, ring = setup(layout, n, 64)
    env.rollout(policy, T, seed=1, first_step=0, record=record, ring=ring)
    us = timed(lambda: env.rollout(policy, T, seed=1, first_step=T, record=record, ring=ring))
    env.close()
    return {"us": us}


def child(args, env=None):
    proc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__)] + args, capture_output=True,
                          text=True, env=env)
    if proc.returncode != 0:
        print(proc.stdout + proc.stderr, file=sys.stderr)
        print(f"{args} ended with status {proc.returncode}: nothing more is started", file=sys.stderr)
        sys.exit(proc.returncode)
    line = [x for x in proc.stdout.splitlines() if x.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    if len(sys.argv) == 4 and sys.argv[1] in ("--case", "--plain-window"):
        run = measure if sys.argv[1] == "--case" else plain_window
        print(json.dumps(run(sys.argv[2], int(sys.argv[3]))), flush=True)
        return 0
    from madrona_rl_envs_playground_amd import _lib
    report = {"build_hash": _lib.source_hash(), "unit": "us per loop step (both seats act, the step writes the ring's next slot)",
              "windows": WINDOWS, "steps_per_window": T, "cases": [child(["--case", layout, str(n)]) for layout, n in CASES]}
    if len(sys.argv) == 3 and sys.argv[1] == "--plain":
        other = dict(os.environ, MRL_PROBE_TREE=os.path.abspath(sys.argv[2]))
        times = {"this_build": [], "parent_build": []}
        for _ in range(WINDOWS):
            times["parent_build"].append(child(["--plain-window", *map(str, PLAIN_CASE)], other)["us"])
            times["this_build"].append(child(["--plain-window", *map(str, PLAIN_CASE)])["us"])
        plain = {"layout": PLAIN_CASE[0], "worlds": PLAIN_CASE[1], **{k: summary(v) for k, v in times.items()}}
        plain["median_inside_parents_spread"] = min(times["parent_build"]) <= statistics.median(times["this_build"]) <= max(times["parent_build"])
        report["plain_hidden_64_rollout"] = plain
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
