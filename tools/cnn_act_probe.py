#!/usr/bin/env python3
"""What one step of the MAPPO-style rollout loop on Overcooked costs with the policy on the device against the torch loop:
us per loop step, written to profiles/cnn_act_cost.json under the library's build hash.

    python tools/cnn_act_probe.py           measure (needs the GPU)

Two loops over the same environment, in ALTERNATING windows of T = 128 steps, five windows each after one that warms both up,
medians and extremes reported:
  torch    ``rollout`` of tools/mappo_rollout_loop.py as it stands: that file's two CNN networks for both seats,
           ``Categorical.sample``, ``env.step(act, out=slot)``, the reward and done rows copied;
  device   ``env.rollout(policy, T)`` (mrl_rollout_cnn): per step one ``mrl_cnn_act`` launch for both seats and both nets, then
           the ordinary step writing the next ring slot; log-probs, values, rewards and dones recorded.
Sizes: cramped_room at 1024 and 32768 worlds, asymmetric_advantages at 32768.
``floor_us``: the arithmetic floor of the policy alone, 2 nets x multiply-adds x 2 flop x samples at the 155 TF f32 matrix peak.
``device_below_torch``: the device loop's median lies below the torch loop's by more than the two loops' spreads (max - min) added.
Every case runs in a child process of its own under ``timeout``; after a child that fails nothing more is started."""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
OUT = os.path.join(REPO, "profiles", "cnn_act_cost.json")
CASES = (("cramped_room", 1024), ("cramped_room", 32768), ("asymmetric_advantages", 32768))
WINDOWS, T = 5, 128
CASE_TIMEOUT_S = 300
PEAK_F32_MATRIX = 155e12


def measure(layout, n):
    import torch
    import mappo_rollout_loop as loop
    from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnRecord
    device = torch.device("cuda", 0)
    env, ego, buffers = loop.build(layout, n, steps_in_buffer=T, seed=0, in_place=True)
    w, h, p, f = env.width, env.height, env.num_players, 5 * env.num_players + 16
    torch.manual_seed(0)
    policy = CnnPolicy.from_module(CnnActorCritic(w, h, f), device=device)
    record = CnnRecord(T, n, p, device)
    ring = torch.empty((T + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=device)
    state = {"ob": env.reset(), "step": 0}

    def torch_window():
        state["ob"] = loop.rollout(env, ego, buffers, state["ob"], T)

    def device_window():
        env.rollout(policy, T, seed=1, first_step=state["step"], record=record, ring=ring)
        state["step"] += T

    def timed(fn):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e6 / T

    torch_window(), device_window()  # warm-up
    times = {"torch_step": [], "device_step": []}
    for _ in range(WINDOWS):
        times["torch_step"].append(timed(torch_window))
        times["device_step"].append(timed(device_window))
    env.close()

    def summary(xs):
        return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    npos = (w - 2) * (h - 2)
    macs = npos * 32 * 9 * f + 32 * npos * 64 + 64 * 64 + 64 * 6  # one net; the critic's head is smaller
    out = {"layout": layout, "worlds": n, "steps_per_window": T, "samples_per_step": n * p, "multiply_adds_per_net": macs,
           "floor_us": round(2 * macs * 2 * n * p / PEAK_F32_MATRIX * 1e6, 1)}
    out.update({k: summary(v) for k, v in times.items()})
    dev, ref = times["device_step"], times["torch_step"]
    out["device_below_torch"] = statistics.median(dev) + (max(dev) - min(dev)) + (max(ref) - min(ref)) < statistics.median(ref)
    return out


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        print(json.dumps(measure(sys.argv[2], int(sys.argv[3]))), flush=True)
        return 0
    from madrona_rl_envs_playground_amd import _lib
    results = []
    for layout, n in CASES:
        proc = subprocess.run(["timeout", "-k", "10", str(CASE_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--case", layout, str(n)],
                              capture_output=True, text=True)
        if proc.returncode != 0:
            print(proc.stdout + proc.stderr, file=sys.stderr)
            print(f"{layout} at {n} worlds ended with status {proc.returncode}: nothing more is started", file=sys.stderr)
            return proc.returncode
        line = [x for x in proc.stdout.splitlines() if x.startswith("{")][-1]
        print(line, flush=True)
        results.append(json.loads(line))
    report = {"build_hash": _lib.source_hash(), "unit": "us per loop step (both seats act, the step writes the next buffer slot)",
              "windows": WINDOWS, "steps_per_window": T, "cases": results}
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
