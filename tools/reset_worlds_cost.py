"""GPU time of mrl_reset_worlds next to one mrl_step on the same simulator (HIP events, median of many calls).

    python tools/reset_worlds_cost.py --out profiles/reset_worlds_cost.json

Mask densities 0, 1 %, 30 % and 100 % on cramped_room (32768 worlds), Hanabi (65536) and Cartpole (1 M).  Two figures each:
`*_us` is the median span between events recorded around ONE Python call (reset_worlds: the copy of a device mask into the
simulator's buffer plus the launches; it includes whatever host time separates the launches), `*_us_back_to_back` the
average over many C calls issued back to back (mrl_reset_worlds on the device mask: the launches alone -- Overcooked /
Simplecooked one, the counter games two: mask -> per-workgroup counts, then the re-seeding launch of the two-launch step).
Hanabi's step is the single-launch step kernel drawing legal moves itself (rollout_random(1) without the persistent kernel)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from madrona_rl_envs_playground_amd import _lib, layouts  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import CartpoleSimulator, ExecMode, HanabiSimulator, OvercookedSimulator  # noqa: E402

DENSITIES = [0.0, 0.01, 0.3, 1.0]


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for start, end in events:
        start.record()
        fn()
        end.record()
    torch.cuda.synchronize()
    return statistics.median(s.elapsed_time(e) * 1000.0 for s, e in events)


def back_to_back(fn, calls, warmup):
    """Average GPU time per call of `calls` calls issued back to back between two events (the launches queue up, so host
    overhead is hidden as long as the GPU is the slower side)."""
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1000.0 / calls


def make(name):
    if name == "cramped_room_32768":
        return OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=32768, **layouts.get_base_layout_params("cramped_room", 400))
    if name == "hanabi_65536":
        with _lib.debug_knobs({"hanabi.no_persistent": 1}):  # rollout_random(1) = one single-launch step drawing legal moves
            return HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=65536, colors=5, ranks=5, players=2,
                                   max_information_tokens=8, max_life_tokens=3)
    return CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=1 << 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    args = ap.parse_args()
    results = {"build_hash": _lib.build_hash(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "unit": "us", "configs": {}}
    for name in ["cramped_room_32768", "hanabi_65536", "cartpole_1048576"]:
        sim = make(name)
        n = sim.num_worlds
        # the step: the simulator's own ACTION tensor (Hanabi: legal moves drawn by the step kernel)
        if name.startswith("hanabi"):
            step = lambda: sim.rollout_random(1, seed=1)  # noqa: E731
        else:
            step = sim.step
        row = {"num_worlds": n, "step_kernel": sim.kernel_name, "step_us": timed(step, args.calls, args.warmup),
               "step_us_back_to_back": back_to_back(step, args.calls, args.warmup), "reset_us": {}, "reset_us_back_to_back": {}}
        gen = torch.Generator().manual_seed(0)
        L, stream = sim._L, torch.cuda.current_stream().cuda_stream
        for d in DENSITIES:
            mask = (torch.rand(n, generator=gen) < d).to(torch.uint8).cuda()
            row["reset_us"][f"{d:g}"] = timed(lambda: sim.reset_worlds(mask), args.calls, args.warmup)  # Python call: mask copy + launches
            raw = lambda: L.mrl_reset_worlds(sim._handle, mask.data_ptr(), stream)  # noqa: E731  (the C call alone: the launches)
            row["reset_us_back_to_back"][f"{d:g}"] = back_to_back(raw, args.calls, args.warmup)
        assert not sim.scan_timed_out
        results["configs"][name] = row
        print(json.dumps({name: row}), flush=True)
        sim.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
