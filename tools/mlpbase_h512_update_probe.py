#!/usr/bin/env python3
"""What one MAPPO update of the hidden-512 MLPBase actor-critic costs on the device (``mappo_update_h512`` on an
``MlpBasePolicyH512``: mrl_mappo_mlp_update with MRL_MLPBASE_H512, the layered update of DESIGN.md section 33) against
tools/balance_mappo_train_device.py's ``autograd_update``, the same losses in torch autograd on ``policy.module()``: us per
update, written to profiles/mlpbase_h512_update_cost.json under the library's build hash.

    python tools/mlpbase_h512_update_probe.py                          measure every size (needs the GPU)
    python tools/mlpbase_h512_update_probe.py --worlds 1024 --no-torch --repeats 1     the device loop alone (for a kernel trace)

One update is the training tool's default: 15 epochs of one minibatch over 200 rows of both seats.  The two loops run in one
process in ALTERNATING windows on the same record, ``--repeats`` windows each after one that warms both up; medians and extremes
are reported.  ``device_below_torch`` is the rule by which the training tool's default at 512 is chosen: the device's median
below torch's by more than the two ranges added; it must hold at every size."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import balance_mappo_train_device as tool  # noqa: E402
import cnn_update_probe as base  # noqa: E402

OUT = os.path.join(REPO, "profiles", "mlpbase_h512_update_cost.json")
WORLDS = (1024, 32768)
T, EPOCHS, MINIBATCHES = tool.DEFAULTS["num_steps"], tool.DEFAULTS["ppo_epoch"], tool.DEFAULTS["num_mini_batch"]


def measure(n, repeats, with_torch, layer_N=tool.DEFAULTS["layer_N"]):
    import torch
    from madrona_rl_envs_playground_amd import _lib, simulators as S
    env = tool.make_env(n)
    torch.manual_seed(1)
    policy = S.MlpBasePolicyH512.from_module(S.MlpBaseActorCritic(hidden=512, layer_N=layer_N), device="cuda:0")
    record = env.rollout(policy, T)
    value_norm = S.ValueNorm("cuda:0")
    advantages, returns = S.mappo_advantages(record, value_norm)
    device_policy = S.MlpBasePolicyH512.from_module(policy.module(), device="cuda:0")
    device_optimizer, device_norm = S.MappoOptimizerH512(device_policy), S.ValueNorm("cuda:0")
    module = policy.module()
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=5e-4, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=5e-4, eps=1e-5)
    shuffles = torch.Generator(device="cuda").manual_seed(1)
    count, rows = T * n * env.n_players, EPOCHS * MINIBATCHES
    stats = torch.zeros((rows, len(_lib.MAPPO_STATS)), dtype=torch.float32, device="cuda:0")

    def indices():
        return S.minibatch_indices(count, MINIBATCHES, EPOCHS, generator=shuffles, device="cuda")

    def device_update():
        S.mappo_update_h512(device_policy, device_optimizer, record, None, advantages, returns, indices(), value_norm=device_norm,
                            clip_param=base.CLIP, entropy_coef=base.ENT, value_loss_coef=base.VCOEF, max_grad_norm=base.MAX_NORM,
                            huber_delta=base.DELTA)

    def torch_update():
        tool.autograd_update(module, actor_opt, critic_opt, value_norm, record, advantages, returns, indices(), stats, base.CLIP, base.ENT,
                             base.VCOEF, base.MAX_NORM, base.DELTA)

    times = {"autograd_update": [], "mappo_update_h512": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = base.timed(torch_update) if with_torch else None
        d = base.timed(device_update)
        if rep:
            times["mappo_update_h512"].append(d)
            if with_torch:
                times["autograd_update"].append(a)
    row = {name: base.summary(v) for name, v in times.items() if v}
    row["minibatch_size"] = count // MINIBATCHES
    if with_torch:
        spread = (row["mappo_update_h512"]["max"] - row["mappo_update_h512"]["min"]) + (row["autograd_update"]["max"] - row["autograd_update"]["min"])
        row["spread_us"] = round(spread, 1)
        row["device_below_torch"] = row["autograd_update"]["median"] - row["mappo_update_h512"]["median"] > spread
    else:
        row["autograd_update"] = "not measured"
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--worlds", type=int, nargs="*", default=list(WORLDS))
    ap.add_argument("--no-torch", action="store_true", help="time the device loop alone")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for n in args.worlds:
        rows[str(n)] = measure(n, args.repeats, not args.no_torch)
        print(n, json.dumps(rows[str(n)]), flush=True)
    record = {"build_hash": _lib.build_hash(), "num_steps": T, "epochs": EPOCHS, "minibatches": MINIBATCHES, "repeats": args.repeats,
              "rows": rows,
              "what": "us per update of E minibatch steps of the MLPBase actor-critic at hidden 512, keyed by worlds: device events "
                      "around one whole update, windows of the two loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
