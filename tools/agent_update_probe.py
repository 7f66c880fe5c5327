#!/usr/bin/env python3
"""What one update of ``CleanPPOAgent`` costs with ``device_update = True`` (``mrl_agent_update``) against the same agent's torch
epochs (the default): milliseconds per update, written to profiles/agent_update_cost.json under the library's build
hash.

    python tools/agent_update_probe.py                      measure every case (needs the GPU)
    python tools/agent_update_probe.py --cases balance@120x128

What is timed is the learning phase alone -- ``update_epochs = 4`` whole-batch epochs and the update's host read; the bootstrap
act and the advantages run once, in front -- from a synchronised device to the return of the call, which ends in a host read
on either path.  Both agents hold the same initial parameters and update on the same record, which one rollout of the device
agent filled.  Windows of the two paths alternate in one process, ``--repeats`` each after one round that warms both up;
medians and extremes are reported.  ``floor_ms`` is the arithmetic floor of the device's update: 3 x the forward pass's
multiply-adds per sample (forward, two products per layer backwards) at 155 TFLOP/s of float32 matrix throughput."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "agent_update_cost.json")
EPOCHS = 4
# the reference's scripts' sizes (hanabi_train.py: 1000 worlds x 128 steps; balance_train.py: 120 worlds) and one large size each
CASES = ("hanabi_full@1000x128", "balance@120x128", "hanabi_full@65536x4", "balance@32768x4")
PEAK_FLOPS = 155e12


def summary(times):
    t = sorted(times)
    return {"ms": [round(v, 3) for v in times], "median": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3)}


def measure(game, n, steps, repeats, with_torch):
    import torch
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona, config_choice
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent
    from madrona_rl_envs_playground_amd.simulators import agent_act, gae_active
    torch.manual_seed(1)
    env = BalanceMadronaTorch(n, 0) if game == "balance" else HanabiMadrona(n, 0, False, config_choice[game[len("hanabi_"):]])
    device = torch.device("cuda", 0)
    common = dict(device=device, num_updates=1000, verbose=False, num_steps=steps, anneal_lr=False, num_minibatches=1, update_epochs=EPOCHS)
    agents = {"device": CleanPPOAgent(env, "ego", seed=2, **common), "torch": CleanPPOAgent(env, "ego_torch", seed=2, **common)}
    agents["device"].device_update = True
    partner = CleanPPOAgent(env.getDummyEnv(1), "partner", seed=3, **common)
    partner.device_update = True
    env.add_partner_agent(partner)
    ego = agents["device"]
    agents["torch"].policy.params.copy_(ego.policy.params)
    obs = env.reset()
    for _ in range(steps):
        action = ego.get_action(obs)
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    agent_act(ego._sim, ego.seat, ego.policy, ego.record, value_only=True)
    advantages, returns = gae_active(ego.record, ego.gamma, ego.gae_lambda)
    agents["torch"]._sim, agents["torch"].record = ego._sim, ego.record  # the same record for both paths
    samples = int(ego.record.active.sum())

    def timed(fn):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e3

    times = {"torch": [], "device": []}
    for rep in range(repeats + 1):  # the first round warms both paths up
        for name in ("torch", "device"):
            if name == "torch" and not with_torch:
                continue
            ms = timed(lambda: agents[name]._learn_device(advantages, returns) if name == "device" else
                       agents[name]._learn_torch(advantages, returns))
            if rep:
                times[name].append(ms)
    row = {name: summary(v) for name, v in times.items() if v}
    row["samples"], row["cells"] = samples, n * steps
    d, s, a = ego.policy.obs_dim, ego.policy.state_dim, ego.policy.num_actions
    macs = (s + d) * 512 + 4 * 512 * 512 + 512 * (1 + a)
    row["floor_ms"] = round(3 * macs * 2 * samples * EPOCHS / PEAK_FLOPS * 1e3, 3)
    row["workspace_bytes"] = ego.optimizer.workspace_bytes(n * steps)
    row["last_losses"] = {name: {k: agents[name].last_losses[k] for k in ("policy_loss", "value_loss", "entropy", "approx_kl")}
                          for name in times if times[name]}
    if with_torch:
        spread = (row["device"]["max"] - row["device"]["min"]) + (row["torch"]["max"] - row["torch"]["min"])
        row["spread_ms"] = round(spread, 3)
        row["device_below_torch"] = row["torch"]["median"] - row["device"]["median"] > spread
    env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cases", nargs="*", default=list(CASES))
    ap.add_argument("--no-torch", action="store_true", help="time the device path alone")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    rows = {}
    for case in args.cases:
        game, size = case.split("@")
        n, steps = (int(x) for x in size.split("x"))
        rows[case] = measure(game, n, steps, args.repeats, not args.no_torch)
        print(case, json.dumps(rows[case]), flush=True)
    record = {"build_hash": _lib.build_hash(), "epochs": EPOCHS, "repeats": args.repeats, "rows": rows,
              "what": "ms per update of 4 whole-batch epochs and the host read behind them, advantages excluded: wall clock from a "
                      "synchronised device to the call's return, windows of the two paths alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
