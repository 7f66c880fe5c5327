#!/usr/bin/env python3
"""What one iteration of the reference's MAPPO recipe costs on the balance beam -- the MLP actor-critic (hidden 64, layer_N 2) at
train/config.py's defaults: T = 200 steps, 15 epochs of one minibatch over all T N 2 samples -- with every phase on the device
against the torch loop of the same networks on the same simulator: ms per iteration and per phase at 1024 and at 32 768 worlds,
written to profiles/balance_mappo_cost.json under the library's build hash.  There was no device path before this one, so the
torch loop is the baseline.

    python tools/balance_mappo_probe.py            measure (needs the GPU)

Two loops on one env, in ALTERNATING windows, five windows each after one that warms both up, medians and extremes reported.  A
window is one iteration, timed as a whole (one wait at its end) and, in a second pass of the same window, phase by phase (a wait
after each phase):
  torch    rollout: per step the int32 -> float cast of OBSERVATION, ``module.actor`` / ``module.critic`` (the
           ``MlpBaseActorCritic`` whose parameters alias the flat tensor), ``Categorical.sample``, ``env.n_step``, reward and
           done rows copied; advantages: the reference's ``compute_returns`` loop over the T rows in torch; update: the loop of
           ``R_MAPPO.train`` (randperm, both losses, two backward passes, two ``clip_grad_norm_``, two Adam steps per epoch);
  device   ``env.rollout`` (mrl_rollout_mlpbase), ``mappo_advantages`` (mrl_gae + a handful of torch ops), ``minibatch_indices`` +
           ``mappo_update`` (mrl_mappo_mlp_update).
No ratio is asserted or required: the numbers are what was measured."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "balance_mappo_cost.json")
WORLDS, T, EPOCHS, MINIBATCHES = (1024, 32768), 200, 15, 1
LR, ENT, GAMMA, LAMBDA, CLIP, DELTA, MAX_NORM = 5e-4, 0.01, 0.99, 0.95, 0.2, 10.0, 10.0
WINDOWS = 5
PHASES = ("rollout", "advantages", "update")


def torch_rollout(env, module, record, num_steps):
    """the rollout loop of train/MAPPO/main_player.py on the env's own tensors: both seats through both nets, a step, the rows of
    the record filled as ``mrl_rollout_mlpbase`` fills them"""
    import torch
    p = env.n_players
    with torch.no_grad():
        for k in range(num_steps + 1):
            record.obs[k].copy_(env.static_observations.transpose(0, 1))
            x = record.obs[k].view(-1, 7).float()
            record.values[k].view(-1).copy_(module.critic(x).squeeze(1))
            if k:
                record.rewards[k - 1].copy_(env.static_rewards.view(p, -1).t())
            done = env.static_dones.view(-1, 1).expand(-1, p).float()
            if k == num_steps:
                record.next_done.copy_(done)
                break
            record.dones[k].copy_(done)
            dist = torch.distributions.Categorical(logits=module.actor(x))
            action = dist.sample()
            record.actions[k].view(-1).copy_(action)
            record.logprobs[k].view(-1).copy_(dist.log_prob(action))
            env.n_step(action.view(-1, p).t().reshape(p, -1, 1).to(torch.int32).contiguous())


def torch_advantages(record, value_norm):
    """``SharedReplayBuffer.compute_returns`` with ``use_gae`` and ValueNorm (utils/shared_buffer.py:216-228), then ``R_MAPPO.train``'s
    normalisation (r_mappo.py:174-182): a loop over the T rows, as the reference runs it"""
    import torch
    t = record.num_steps
    values = value_norm.denormalize(record.values)
    masks = 1.0 - torch.cat([record.dones, record.next_done[None]])
    returns, gae = torch.zeros_like(record.rewards), 0
    for step in reversed(range(t)):
        delta = record.rewards[step] + GAMMA * values[step + 1] * masks[step + 1] - values[step]
        gae = delta + GAMMA * LAMBDA * masks[step + 1] * gae
        returns[step] = gae + values[step]
    advantages = returns - values[:-1]
    return (advantages - advantages.mean()) / (advantages.std() + 1e-5), returns


def torch_update(module, actor_opt, critic_opt, value_norm, record, advantages, returns):
    """``R_MAPPO.train`` / ``ppo_update`` (train/MAPPO/r_mappo.py:91-164, 166-215) in torch: per epoch one permutation cut into the
    minibatches, the gathered rows cast to float, both losses, two backward passes, two clips and two Adam steps"""
    import torch
    t = record.num_steps
    obs = record.obs[:t].view(-1, 7)
    count = obs.shape[0]
    flat = lambda a: a.reshape(-1)  # noqa: E731
    actions, old_logp, old_v, adv, ret = flat(record.actions), flat(record.logprobs), flat(record.values[:t]), flat(advantages), flat(returns)
    for _ in range(EPOCHS):
        perm = torch.randperm(count, device=obs.device)
        for inds in perm.view(MINIBATCHES, -1):
            x = obs[inds].float()
            dist = torch.distributions.Categorical(logits=module.actor(x))
            ratio = (dist.log_prob(actions[inds].long()) - old_logp[inds]).exp()
            a = adv[inds]
            policy_loss = -torch.min(ratio * a, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * a).mean()
            actor_opt.zero_grad()
            (policy_loss - dist.entropy().mean() * ENT).backward()
            torch.nn.utils.clip_grad_norm_(module.actor.parameters(), MAX_NORM)
            actor_opt.step()
            v, old = module.critic(x).squeeze(1), old_v[inds]
            value_norm.update(ret[inds])
            target = value_norm.normalize(ret[inds])
            e, e_c = target - v, target - (old + (v - old).clamp(-CLIP, CLIP))

            def huber(err):
                return (err.abs() <= DELTA).float() * err ** 2 / 2 + (err > DELTA).float() * DELTA * (err.abs() - DELTA / 2)
            value_loss = torch.max(huber(e), huber(e_c)).mean()
            critic_opt.zero_grad()
            value_loss.backward()
            torch.nn.utils.clip_grad_norm_(module.critic.parameters(), MAX_NORM)
            critic_opt.step()


def measure(worlds, windows):
    import torch
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    dev = torch.device("cuda", 0)
    env = BalanceMadronaTorch(worlds, 0)
    players = env.n_players
    count = T * worlds * players
    torch.manual_seed(1)
    start = S.MlpBaseActorCritic()
    sides = {name: {"policy": S.MlpBasePolicy.from_module(start, device=dev), "value_norm": S.ValueNorm(dev),
                    "record": S.MlpBaseRecord(T, worlds, players, dev)} for name in ("torch", "device")}
    module = sides["torch"]["policy"].module()
    # (fc_h has no gradient: torch's Adam skips it, as the reference's does)
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=LR, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=LR, eps=1e-5)
    optimizer = S.MappoOptimizer(sides["device"]["policy"], lr=LR, critic_lr=LR)
    shuffles = torch.Generator(device=dev).manual_seed(1)
    step = {"first": 0}

    def torch_phases():
        s = sides["torch"]
        yield lambda: torch_rollout(env, module, s["record"], T)
        yield lambda: s.update(zip(("advantages", "returns"), torch_advantages(s["record"], s["value_norm"])))
        yield lambda: torch_update(module, actor_opt, critic_opt, s["value_norm"], s["record"], s["advantages"], s["returns"])

    def device_update(s):
        indices = S.minibatch_indices(count, MINIBATCHES, EPOCHS, generator=shuffles, device=dev)
        S.mappo_update(s["policy"], optimizer, s["record"], None, s["advantages"], s["returns"], indices, value_norm=s["value_norm"],
                       entropy_coef=ENT)

    def device_phases():
        s = sides["device"]

        def rollout():
            env.rollout(s["policy"], T, seed=1, first_step=step["first"], record=s["record"])
            step["first"] += T
        yield rollout
        yield lambda: s.update(zip(("advantages", "returns"), S.mappo_advantages(s["record"], s["value_norm"], GAMMA, LAMBDA)))
        yield lambda: device_update(s)

    def window(phases, split):
        """ms of one iteration: as a whole, or the three phases each behind a wait of its own"""
        torch.cuda.synchronize()
        times, begin = [], time.perf_counter()
        for phase in phases():
            phase()
            if split:
                torch.cuda.synchronize()
                times.append((time.perf_counter() - begin) * 1e3)
                begin = time.perf_counter()
        torch.cuda.synchronize()
        return times if split else (time.perf_counter() - begin) * 1e3

    loops = [("torch", torch_phases), ("device", device_phases)]
    torch_failure = None
    try:
        window(torch_phases, False)  # warm-up
    except (ValueError, RuntimeError) as exc:
        # the baseline itself may not run at a size: torch's float32 forward has returned NaN rows for a 13 M-row minibatch, which
        # Categorical refuses.  The device loop is then measured alone and the file says so.
        torch_failure = str(exc).splitlines()[0][:300]
        loops = loops[1:]
        torch.cuda.synchronize()
    window(device_phases, False)  # warm-up
    names = [f"{side}_{what}" for side, _ in loops for what in ("iteration",) + PHASES]
    times = {name: [] for name in names}
    for _ in range(windows):
        for side, phases in loops:
            times[f"{side}_iteration"].append(window(phases, False))
            for what, ms in zip(PHASES, window(phases, True)):
                times[f"{side}_{what}"].append(ms)
    finite = all(bool(torch.isfinite(sides[side]["policy"].params).all()) for side, _ in loops)
    env.close()

    def summary(xs):
        return {"ms": [round(x, 2) for x in xs], "median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2),
                "max_ms": round(max(xs), 2)}

    out = {name: summary(xs) for name, xs in times.items()}
    out["parameters_finite"] = finite
    out["samples"] = count
    out["env_steps_per_s"] = {side: round(T * worlds / (out[f"{side}_iteration"]["median_ms"] * 1e-3)) for side, _ in loops}
    if torch_failure:
        out["torch"] = "NOT MEASURED: the torch loop failed in its first window: " + torch_failure
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--worlds", type=int, nargs="+", default=list(WORLDS))
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from madrona_rl_envs_playground_amd import _lib
    record = {"build_hash": _lib.build_hash(), "game": "balance", "hidden": 64, "layer_N": 2, "num_steps": T, "epochs": EPOCHS,
              "minibatches": MINIBATCHES, "lr": LR, "entropy_coef": ENT, "windows": args.windows, "rows": {},
              "what": "ms per iteration (rollout of T steps, advantages, E x M minibatch steps): host clock around one window behind a "
                      "device wait; *_iteration one wait at the end, the phases a wait each; windows of the two loops alternating in "
                      "one process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):  # sizes measured by an earlier call on the same build stay in the file
        with open(args.out) as f:
            earlier = json.load(f)
        if earlier.get("build_hash") == record["build_hash"] and earlier.get("windows") == args.windows:
            record["rows"].update(earlier.get("rows", {}))
    for worlds in args.worlds:
        record["rows"][str(worlds)] = measure(worlds, args.windows)
        print(worlds, json.dumps(record["rows"][str(worlds)]), flush=True)
        with open(args.out, "w") as f:  # (after every size: a later, larger one that runs out of time leaves the earlier ones)
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")
    print("->", args.out)


if __name__ == "__main__":
    main()
