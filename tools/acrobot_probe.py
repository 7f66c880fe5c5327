#!/usr/bin/env python3
"""Acrobot step cost: us per step at 1024, 65 536 and 1 M worlds for the single-launch step, the two-launch step and the
measurement builds of the same sources (csrc/acrobot.hip): `plain`, the plain-libm variant (-DMRL_ACROBOT_PLAIN), and
`four_waves`, the step kernels held to 128 VGPRs = four waves per SIMD instead of the compiler's own budget
(-DMRL_ACROBOT_WAVES=4).
Written to profiles/acrobot_step_cost.json under the library's build hash.

    python tools/acrobot_probe.py --build-variants      compile the measurement builds (hipcc, no GPU needed)
    python tools/acrobot_probe.py                    measure (needs the GPU; a measurement build only if it has been built)

What is timed: `steps` calls of step_with_actions over a pool of eight action tensors between two device events, after a
warm-up of the same calls; `repeats` such windows, alternating the forms of the step, the median and the spread reported.
The worlds start from a spread of swinging states and run under a uniform random policy, so episodes end all the time.  The
measurement builds are other builds of the same sources, each measured by a child process that loads it (MRL_ENVS_LIB)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = os.path.join(REPO, "madrona_rl_envs_playground_amd")
VARIANTS = {"plain": "-DMRL_ACROBOT_PLAIN", "four_waves": "-DMRL_ACROBOT_WAVES=4"}


def variant_lib(name):
    return os.path.join(PKG, "variants", f"libmrl_envs_acrobot_{name}.so")
OUT = os.path.join(REPO, "profiles", "acrobot_step_cost.json")
SIZES = [1024, 65536, 1 << 20]
HBM_PEAK = 6.29e12    # bytes / s: float4 copy measured on MI355X
VALU_LANES = 1024 * 16 * 2.4e9  # lane-instructions / s: 1024 SIMDs x 16 lanes per clock at 2.4 GHz, unpacked fp32


def build_variants():
    os.makedirs(os.path.join(PKG, "variants"), exist_ok=True)
    for name, flag in VARIANTS.items():
        cmd = ["make", "-C", os.path.join(PKG, "csrc"), "-j", str(min(6, os.cpu_count() or 1)), f"OUT=../variants/libmrl_envs_acrobot_{name}.so",
               f"OBJDIR=../variants/obj_acrobot_{name}", "EXTRA_CXXFLAGS=" + flag]
        subprocess.run(cmd, check=True)
        print(variant_lib(name))


def measure(forms, sizes, steps, warmup, repeats):
    import numpy as np
    import torch
    from madrona_rl_envs_playground_amd import _lib
    from madrona_rl_envs_playground_amd.simulators import AcrobotSimulator, ExecMode
    rows = {}
    for n in sizes:
        rng = np.random.default_rng(n)
        start = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-3, 3, n),
                          rng.uniform(-6, 6, n)], axis=1).astype(np.float32)
        pool = [torch.randint(0, 3, (n, 1), dtype=torch.int32, device="cuda") for _ in range(8)]
        sims = {}
        for form, fused in forms.items():
            with _lib.debug_knobs({"fused_step": fused}):
                sims[form] = AcrobotSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
            sims[form].observation_tensor().to_torch().copy_(torch.from_numpy(start))
        times = {form: [] for form in forms}
        for rep in range(repeats + 1):  # the first round is the warm-up of every form
            for form, sim in sims.items():
                for i in range(warmup):
                    sim.step_with_actions(pool[i % 8])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(steps):
                    sim.step_with_actions(pool[i % 8])
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[form].append(e0.elapsed_time(e1) / steps * 1e3)
        for form, sim in sims.items():
            t = sorted(times[form])
            rows[f"{form}@{n}"] = {"worlds": n, "kernel": sim.kernel_name, "us_per_step_median": round(statistics.median(t), 3),
                                   "us_per_step_min": round(t[0], 3), "us_per_step_max": round(t[-1], 3),
                                   "byte_bound_us": round(sim.bytes_per_world_step * n / HBM_PEAK * 1e6, 3)}
            print(f"{form:>12s} {n:8d} worlds {sim.kernel_name:24s} {rows[f'{form}@{n}']}", flush=True)
            sim.close()
    return rows, _lib.build_hash()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-variants", action="store_true")
    ap.add_argument("--child", choices=sorted(VARIANTS), help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.build_variants:
        build_variants()
        return
    if args.child:  # this process has loaded that measurement build
        rows, build = measure({args.child + "_one_launch": 1}, args.sizes, args.steps, args.warmup, args.repeats)
        print("ROWS " + json.dumps({"rows": rows, "build": build}))
        return
    rows, build = measure({"one_launch": 1, "two_launches": 2}, args.sizes, args.steps, args.warmup, args.repeats)
    for name in VARIANTS:
        if not os.path.exists(variant_lib(name)):
            print(f"{name} build not there (tools/acrobot_probe.py --build-variants): not measured")
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--repeats", str(args.repeats), "--sizes"] + [str(n) for n in args.sizes]
        proc = subprocess.run(cmd, env={**os.environ, "MRL_ENVS_LIB": variant_lib(name)}, capture_output=True, text=True)
        sys.stdout.write(proc.stdout)
        if proc.returncode != 0:
            raise SystemExit(f"the {name} build's run failed:\n" + proc.stderr[-4000:])
        child = json.loads([line for line in proc.stdout.splitlines() if line.startswith("ROWS ")][-1][5:])
        if child["build"] != build:
            raise SystemExit(f"the {name} build is of other sources ({child['build']}) than the library ({build})")
        rows.update(child["rows"])
        for n in args.sizes:
            rows[f"one_launch@{n}"][name + "_over_default"] = round(rows[f"{name}_one_launch@{n}"]["us_per_step_median"] /
                                                                     rows[f"one_launch@{n}"]["us_per_step_median"], 3)
    record = {"build_hash": build, "what": "us per Acrobot step, device events around `steps` step_with_actions calls, median of `repeats` windows",
              "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats, "hbm_peak_bytes_per_s": HBM_PEAK,
              "valu_lane_instructions_per_s": VALU_LANES, "rows": rows}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
