#!/usr/bin/env python3
"""What one MAPPO update costs on the device (``mappo_update``: mrl_mappo_update, three launches per minibatch step) against the
loop of the reference's ``R_MAPPO.train`` (train/MAPPO/r_mappo.py:166-219) written in torch on ``policy.module()``: us per update,
written to profiles/cnn_update_cost.json under the library's build hash.

    python tools/cnn_update_probe.py                              measure every case (needs the GPU)
    python tools/cnn_update_probe.py --cases cramped_room@1024    one case

One update is E = 15 epochs of M = 1 minibatch over T = 128 rows of both seats.  Two loops, in one process, in ALTERNATING
windows on the same record and ring, five windows each after one that warms both up, medians and extremes reported:
  torch_loop     per step: the float32 copy of the int8 observations, both forward passes, ValueNorm, the clipped losses, two
                 backward passes, two clip_grad_norm_ and two Adam steps on the module whose parameters alias the flat tensor;
  mappo_update   ``minibatch_indices`` + ``mappo_update`` on the flat parameter tensor.
``floor_us`` is the arithmetic floor of the device's update: 6 x the forward pass's multiply-adds per sample and net (forward,
two products per layer backwards) at 155 TFLOP/s of float32 matrix throughput."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "cnn_update_cost.json")
T, EPOCHS, MINIBATCHES = 128, 15, 1
CASES = ("cramped_room@1024", "cramped_room@32768", "asymmetric_advantages@1024")
CLIP, ENT, VCOEF, MAX_NORM, DELTA = 0.2, 0.01, 1.0, 10.0, 10.0
PEAK_FLOPS = 155e12  # float32 on the matrix cores, as tools/cnn_act_probe.py takes it


def huber_loss(e, d):
    a = (abs(e) <= d).float()
    b = (e > d).float()
    return a * e ** 2 / 2 + b * d * (abs(e) - d / 2)


def torch_update(module, actor_opt, critic_opt, value_norm, record, ring, advantages, returns):
    import torch
    t = record.num_steps
    obs = ring[:t].reshape((-1,) + tuple(ring.shape[3:]))
    flat = [record.actions.reshape(-1), record.logprobs.reshape(-1), advantages.reshape(-1), returns.reshape(-1), record.values[:t].reshape(-1)]
    count = flat[0].numel()
    for _ in range(EPOCHS):
        for rows in torch.randperm(count, device=obs.device).chunk(MINIBATCHES):
            x = obs[rows].transpose(1, 2).float()
            actions, old_logp, adv, ret, old_v = (f[rows] for f in flat)
            dist = torch.distributions.Categorical(logits=module.actor(x))
            ratio = torch.exp(dist.log_prob(actions.long()) - old_logp)
            policy_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv).mean()
            actor_opt.zero_grad()
            (policy_loss - dist.entropy().mean() * ENT).backward()
            torch.nn.utils.clip_grad_norm_(module.actor.parameters(), MAX_NORM)
            actor_opt.step()
            values = module.critic(x).squeeze(1)
            clipped = old_v + (values - old_v).clamp(-CLIP, CLIP)
            value_norm.update(ret)
            target = value_norm.normalize(ret)
            value_loss = torch.max(huber_loss(target - values, DELTA), huber_loss(target - clipped, DELTA)).mean()
            critic_opt.zero_grad()
            (value_loss * VCOEF).backward()
            torch.nn.utils.clip_grad_norm_(module.critic.parameters(), MAX_NORM)
            critic_opt.step()


def timed(fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(times):
    t = sorted(times)
    return {"us": [round(v, 1) for v in times], "median": round(statistics.median(t), 1), "min": round(t[0], 1), "max": round(t[-1], 1)}


def measure(layout, n, repeats, with_torch):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    env = OvercookedMadrona(layout, n, 0)
    _, players, h, w, f = env.static_world_major_observations.shape
    torch.manual_seed(1)
    policy = S.CnnPolicy.from_module(S.CnnActorCritic(w, h, f), device="cuda:0")
    record, ring = env.rollout(policy, T)
    value_norm = S.ValueNorm("cuda:0")
    advantages, returns = S.mappo_advantages(record, value_norm)
    device_policy = S.CnnPolicy.from_module(policy.module(), device="cuda:0")
    device_optimizer, device_norm = S.MappoOptimizer(device_policy), S.ValueNorm("cuda:0")
    module = policy.module()
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=5e-4, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=5e-4, eps=1e-5)
    shuffles = torch.Generator(device="cuda").manual_seed(1)
    count = T * n * players

    def device_update():
        indices = S.minibatch_indices(count, MINIBATCHES, EPOCHS, generator=shuffles, device="cuda")
        S.mappo_update(device_policy, device_optimizer, record, ring, advantages, returns, indices, value_norm=device_norm, clip_param=CLIP,
                       entropy_coef=ENT, value_loss_coef=VCOEF, max_grad_norm=MAX_NORM, huber_delta=DELTA)

    times = {"torch_loop": [], "mappo_update": []}
    for rep in range(repeats + 1):  # the first round warms both loops up
        a = timed(lambda: torch_update(module, actor_opt, critic_opt, value_norm, record, ring, advantages, returns)) if with_torch else None
        d = timed(device_update)
        if rep:
            times["mappo_update"].append(d)
            if with_torch:
                times["torch_loop"].append(a)
    row = {name: summary(v) for name, v in times.items() if v}
    npos = (w - 2) * (h - 2)
    macs = 2 * (32 * 9 * f * npos + 64 * 32 * npos + 64 * 64) + 64 * 6 + 64  # both nets, one forward pass of one sample
    row["floor_us"] = round(6 * macs * 2 * count * EPOCHS / PEAK_FLOPS * 1e6, 1)
    row["minibatch_size"] = count // MINIBATCHES
    if with_torch:
        spread = (row["mappo_update"]["max"] - row["mappo_update"]["min"]) + (row["torch_loop"]["max"] - row["torch_loop"]["min"])
        row["spread_us"] = round(spread, 1)
        row["device_below_torch"] = row["torch_loop"]["median"] - row["mappo_update"]["median"] > spread
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
    record = {"build_hash": _lib.build_hash(), "num_steps": T, "epochs": EPOCHS, "minibatches": MINIBATCHES, "repeats": args.repeats,
              "rows": rows, "what": "us per update of E x M minibatch steps: device events around one whole update, windows of the two "
                                    "loops alternating in one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
