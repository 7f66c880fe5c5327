#!/usr/bin/env python3
"""What one MAPPO update of the hidden-512 CNN actor-critic costs on the device (``mappo_update_h512``: mrl_mappo_h512_update, the
layered update of DESIGN.md section 31) against the loop of the reference's ``R_MAPPO.train`` written in torch on
``policy.module()`` at 512 (tools/cnn_update_probe.py's ``torch_update``, the reference here): us per update, written to
profiles/cnn_h512_update_cost.json under the library's build hash.

    python tools/cnn_h512_update_probe.py                              measure every case (needs the GPU)
    python tools/cnn_h512_update_probe.py --cases cramped_room@1024 --no-torch --repeats 1     the device loop alone (for a kernel trace)

One update is E = 15 epochs of one minibatch over T = 128 rows of both seats.  The two loops run in one process in ALTERNATING
windows on the same record and ring, five windows each after one that warms both up; medians and extremes are reported.
``floor_us``: 6 x the forward pass's multiply-adds per sample and net at 155 TFLOP/s of float32 matrix throughput."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import cnn_update_probe as base  # noqa: E402

OUT = os.path.join(REPO, "profiles", "cnn_h512_update_cost.json")
CASES = ("cramped_room@1024", "asymmetric_advantages@1024")


def measure(layout, n, repeats, with_torch):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    env = OvercookedMadrona(layout, n, 0)
    _, players, h, w, f = env.static_world_major_observations.shape
    torch.manual_seed(1)
    policy = S.CnnPolicy.from_module(S.CnnActorCritic(w, h, f, hidden=512), device="cuda:0")
    record, ring = env.rollout(policy, base.T)
    value_norm = S.ValueNorm("cuda:0")
    advantages, returns = S.mappo_advantages(record, value_norm)
    device_policy = S.CnnPolicy.from_module(policy.module(), device="cuda:0")
    device_optimizer, device_norm = S.MappoOptimizerH512(device_policy), S.ValueNorm("cuda:0")
    module = policy.module()
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=5e-4, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=5e-4, eps=1e-5)
    shuffles = torch.Generator(device="cuda").manual_seed(1)
    count = base.T * n * players

    def device_update():
        indices = S.minibatch_indices(count, base.MINIBATCHES, base.EPOCHS, generator=shuffles, device="cuda")
        S.mappo_update_h512(device_policy, device_optimizer, record, ring, advantages, returns, indices, value_norm=device_norm,
                            clip_param=base.CLIP, entropy_coef=base.ENT, value_loss_coef=base.VCOEF, max_grad_norm=base.MAX_NORM,
                            huber_delta=base.DELTA)

    times = {"torch_loop": [], "mappo_update_h512": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = base.timed(lambda: base.torch_update(module, actor_opt, critic_opt, value_norm, record, ring, advantages, returns)) if with_torch else None
        d = base.timed(device_update)
        if rep:
            times["mappo_update_h512"].append(d)
            if with_torch:
                times["torch_loop"].append(a)
    row = {name: base.summary(v) for name, v in times.items() if v}
    npos = (w - 2) * (h - 2)
    macs = 2 * (256 * 9 * f * npos + 512 * 256 * npos + 512 * 512) + 512 * 6 + 512  # both nets, one forward pass of one sample
    row["floor_us"] = round(6 * macs * 2 * count * base.EPOCHS / base.PEAK_FLOPS * 1e6, 1)
    row["minibatch_size"] = count // base.MINIBATCHES
    if with_torch:
        spread = (row["mappo_update_h512"]["max"] - row["mappo_update_h512"]["min"]) + (row["torch_loop"]["max"] - row["torch_loop"]["min"])
        row["spread_us"] = round(spread, 1)
        row["device_below_torch"] = row["torch_loop"]["median"] - row["mappo_update_h512"]["median"] > spread
    else:
        row["torch_loop"] = "not measured"
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--no-torch", action="store_true", help="time the device loop alone")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for case in args.cases:
        layout, n = case.split("@")
        rows[case] = measure(layout, int(n), args.repeats, not args.no_torch)
        print(case, json.dumps(rows[case]), flush=True)
    record = {"build_hash": _lib.build_hash(), "num_steps": base.T, "epochs": base.EPOCHS, "minibatches": base.MINIBATCHES,
              "repeats": args.repeats, "rows": rows,
              "what": "us per update of E minibatch steps at hidden 512: device events around one whole update, windows of the two "
                      "loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
