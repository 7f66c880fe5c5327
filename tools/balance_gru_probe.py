#!/usr/bin/env python3
"""What one iteration of the reference's RECURRENT MAPPO recipe costs on the balance beam -- the MLP actor-critic with a GRU
(hidden 64, layer_N 2, ``--use_recurrent_policy``) at train/config.py's defaults: T = 200 steps, 15 epochs of one minibatch over
all (T / 10) N 2 chunks of ``data_chunk_length`` 10 -- with every phase on the device against the torch loop of the same recurrent
modules on the same simulator: ms per iteration and per phase at 1024 and at 8192 worlds, written to
profiles/balance_gru_cost.json under the library's build hash.

    python tools/balance_gru_probe.py                          measure (needs the GPU)
    python tools/balance_gru_probe.py --parent-tree DIR        also: the PLAIN path of this build against the build in DIR

Two loops on one env, in ALTERNATING windows, five windows each after one that warms both up, medians and extremes reported
(tools/balance_mappo_probe.py's windows: an iteration timed as a whole, then again phase by phase).
  torch    rollout: per step both nets' ``forward(obs, h, mask)`` on the ``MlpBaseGruActorCritic`` whose parameters alias the flat
           tensor, ``Categorical.sample``, ``env.n_step``, the states carried and written to ``h0`` every L rows; advantages: the
           reference's ``compute_returns`` loop; update: ``R_MAPPO.train`` with ``recurrent_generator``'s chunks, each minibatch
           evaluated the way ``RNNLayer.forward`` evaluates a flattened (L, n) batch (utils/rnn.py:41-69: one ``nn.GRU`` call per run
           of steps without a zero mask), two backward passes through time, two clips, two Adam steps per epoch;
  device   ``env.rollout`` (mrl_rollout_mlpbase), ``mappo_advantages``, ``chunk_indices`` + ``mappo_update`` (mrl_mappo_mlp_update).
``--parent-tree``: the plain ``MlpBasePolicy``'s rollout and ``mappo_update`` at 1024 worlds, this build against the build in DIR, a
checkout of the parent commit with its library built (tools/ppo_bank_probe.py's convention), a window per fresh process,
alternating; sizes measured by an earlier call on the same build stay in the file; the criterion is the project's usual one: this
build's median inside the parent build's own min - max spread, or below it.  No ratio is asserted or required: the numbers are what was measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a --plain-window child of --parent-tree imports the package of that tree: only calls the parent commit has)
sys.path.insert(0, os.environ.get("MRL_PROBE_TREE") or REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "profiles", "balance_gru_cost.json")
WORLDS, T, CHUNK, EPOCHS = (1024, 8192), 200, 10, 15
LR, ENT, GAMMA, LAMBDA, CLIP, DELTA, MAX_NORM = 5e-4, 0.01, 0.99, 0.95, 0.2, 10.0, 10.0
WINDOWS = 5
PHASES = ("rollout", "advantages", "update")


def torch_rollout(env, module, state, record, num_steps):
    """the rollout loop of train/MAPPO/main_player.py with rnn states: both seats through both nets from the carried states, masked
    where DONE is set; the rows of the record filled as ``mrl_rollout_mlpbase`` fills them"""
    import torch
    p, L = env.n_players, record.chunk_length
    h_a, h_c = state.actor.view(-1, 64), state.critic.view(-1, 64)
    with torch.no_grad():
        for k in range(num_steps + 1):
            record.obs[k].copy_(env.static_observations.transpose(0, 1))
            x = record.obs[k].view(-1, 7).float()
            done = env.static_dones.view(-1, 1).expand(-1, p).float()
            mask = 1.0 - done.reshape(-1)
            if k < num_steps and k % L == 0:
                record.h0_actor[k // L].view(-1, 64).copy_(h_a)
                record.h0_critic[k // L].view(-1, 64).copy_(h_c)
            value, new_c = module.critic(x, h_c, mask)
            record.values[k].view(-1).copy_(value.squeeze(1))
            if k:
                record.rewards[k - 1].copy_(env.static_rewards.view(p, -1).t())
            if k == num_steps:
                record.next_done.copy_(done)
                break
            h_c.copy_(new_c)
            record.dones[k].copy_(done)
            logits, new_a = module.actor(x, h_a, mask)
            h_a.copy_(new_a)
            dist = torch.distributions.Categorical(logits=logits)
            action = dist.sample()
            record.actions[k].view(-1).copy_(action)
            record.logprobs[k].view(-1).copy_(dist.log_prob(action))
            env.n_step(action.view(-1, p).t().reshape(p, -1, 1).to(torch.int32).contiguous())


def rnn_layer(layer, x, h, masks):
    """``RNNLayer.forward`` for a flattened (L, n) batch (utils/rnn.py:41-69): x (L, n, 64), h (n, 64), masks (L, n); one ``nn.GRU``
    call per run of steps in which no chunk has a zero mask, the state masked where a run begins -> the LayerNorm's output"""
    import torch
    L = x.shape[0]
    zeros = ((masks[1:] == 0.0).any(dim=-1).nonzero().squeeze(-1) + 1).cpu().tolist()  # (the reference waits for the host here too)
    cuts = [0] + zeros + [L]
    h, outs = h.unsqueeze(0), []
    for begin, end in zip(cuts[:-1], cuts[1:]):
        scores, h = layer.rnn(x[begin:end], (h * masks[begin].view(1, -1, 1)).contiguous())
        outs.append(scores)
    return layer.norm(torch.cat(outs, dim=0))


def torch_update(module, actor_opt, critic_opt, value_norm, record, advantages, returns):
    """``R_MAPPO.train`` / ``ppo_update`` with ``recurrent_generator``: per epoch one permutation of the chunks, one minibatch"""
    import torch
    t, L, n, p = record.num_steps, record.chunk_length, record.num_worlds, record.num_players
    cells = n * p
    chunked = lambda a: a[:t].reshape(t // L, L, cells, *a.shape[3:]).transpose(0, 1).reshape(L, (t // L) * cells, *a.shape[3:])  # noqa: E731
    obs, masks = chunked(record.obs).float(), 1.0 - chunked(record.dones)
    actions, old_logp, old_v, adv, ret = (chunked(a) for a in (record.actions, record.logprobs, record.values, advantages, returns))
    h0_a, h0_c = record.h0_actor.view(-1, 64), record.h0_critic.view(-1, 64)
    for _ in range(EPOCHS):
        inds = torch.randperm(obs.shape[1], device=obs.device)
        x, m = obs[:, inds], masks[:, inds]
        features = rnn_layer(module.actor.rnn, module.actor.base(x), h0_a[inds], m)
        dist = torch.distributions.Categorical(logits=module.actor.act.action_out.linear(features))
        ratio = (dist.log_prob(actions[:, inds].long()) - old_logp[:, inds]).exp()
        a = adv[:, inds]
        policy_loss = -torch.min(ratio * a, ratio.clamp(1.0 - CLIP, 1.0 + CLIP) * a).mean()
        actor_opt.zero_grad()
        (policy_loss - dist.entropy().mean() * ENT).backward()
        torch.nn.utils.clip_grad_norm_(module.actor.parameters(), MAX_NORM)
        actor_opt.step()
        v = module.critic.v_out(rnn_layer(module.critic.rnn, module.critic.base(x), h0_c[inds], m)).squeeze(-1)
        old, target_raw = old_v[:, inds], ret[:, inds]
        value_norm.update(target_raw)
        target = value_norm.normalize(target_raw)
        e, e_c = target - v, target - (old + (v - old).clamp(-CLIP, CLIP))

        def huber(err):
            return (err.abs() <= DELTA).float() * err ** 2 / 2 + (err > DELTA).float() * DELTA * (err.abs() - DELTA / 2)
        value_loss = torch.max(huber(e), huber(e_c)).mean()
        critic_opt.zero_grad()
        value_loss.backward()
        torch.nn.utils.clip_grad_norm_(module.critic.parameters(), MAX_NORM)
        critic_opt.step()


def window(phases, split):
    """ms of one iteration: as a whole, or the three phases each behind a wait of its own"""
    import torch
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


def summary(xs):
    return {"ms": [round(x, 2) for x in xs], "median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2), "max_ms": round(max(xs), 2)}


def measure(worlds, windows):
    import torch
    from balance_mappo_probe import torch_advantages
    from madrona_rl_envs_playground_amd import simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    dev = torch.device("cuda", 0)
    env = BalanceMadronaTorch(worlds, 0)
    players = env.n_players
    torch.manual_seed(1)
    start = S.MlpBaseGruActorCritic()
    sides = {name: {"policy": S.MlpBaseGruPolicy.from_module(start, device=dev), "value_norm": S.ValueNorm(dev),
                    "record": S.MlpBaseGruRecord(T, worlds, players, dev, chunk_length=CHUNK)} for name in ("torch", "device")}
    for side in sides.values():
        side["state"] = side["policy"].state(worlds)
    module = sides["torch"]["policy"].module()
    actor_opt = torch.optim.Adam(module.actor.parameters(), lr=LR, eps=1e-5)
    critic_opt = torch.optim.Adam(module.critic.parameters(), lr=LR, eps=1e-5)
    optimizer = S.MappoOptimizer(sides["device"]["policy"], lr=LR, critic_lr=LR)
    shuffles = torch.Generator(device=dev).manual_seed(1)
    step = {"first": 0}

    def torch_phases():
        s = sides["torch"]
        yield lambda: torch_rollout(env, module, s["state"], s["record"], T)
        yield lambda: s.update(zip(("advantages", "returns"), torch_advantages(s["record"], s["value_norm"])))
        yield lambda: torch_update(module, actor_opt, critic_opt, s["value_norm"], s["record"], s["advantages"], s["returns"])

    def device_phases():
        s = sides["device"]

        def rollout():
            env.rollout(s["policy"], T, seed=1, first_step=step["first"], record=s["record"])
            step["first"] += T
        yield rollout
        yield lambda: s.update(zip(("advantages", "returns"), S.mappo_advantages(s["record"], s["value_norm"], GAMMA, LAMBDA)))
        yield lambda: S.mappo_update(s["policy"], optimizer, s["record"], None, s["advantages"], s["returns"],
                                     S.chunk_indices(s["record"], 1, EPOCHS, generator=shuffles, device=dev), value_norm=s["value_norm"],
                                     entropy_coef=ENT)

    loops = [("torch", torch_phases), ("device", device_phases)]
    for _, phases in loops:
        window(phases, False)  # warm-up
    times = {f"{side}_{what}": [] for side, _ in loops for what in ("iteration",) + PHASES}
    for _ in range(windows):
        for side, phases in loops:
            times[f"{side}_iteration"].append(window(phases, False))
            for what, ms in zip(PHASES, window(phases, True)):
                times[f"{side}_{what}"].append(ms)
    finite = all(bool(torch.isfinite(sides[side]["policy"].params).all()) for side, _ in loops)
    env.close()
    out = {name: summary(xs) for name, xs in times.items()}
    out["parameters_finite"] = finite
    out["chunks"] = T // CHUNK * worlds * players
    out["device_over_torch"] = round(out["device_iteration"]["median_ms"] / out["torch_iteration"]["median_ms"], 3)
    return out


def plain_window(worlds):
    """one window of the PLAIN path in this process (whose package MRL_PROBE_TREE chose): ms of a rollout of T steps and of
    ``mappo_update`` over 15 epochs of one minibatch, each behind a wait, after one warm-up of both"""
    import torch
    from madrona_rl_envs_playground_amd import _lib, simulators as S
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    dev = torch.device("cuda", 0)
    env = BalanceMadronaTorch(worlds, 0)
    torch.manual_seed(1)
    policy = S.MlpBasePolicy.from_module(S.MlpBaseActorCritic(), device=dev)
    optimizer, value_norm = S.MappoOptimizer(policy, lr=LR, critic_lr=LR), S.ValueNorm(dev)
    record = S.MlpBaseRecord(T, worlds, env.n_players, dev)
    shuffles = torch.Generator(device=dev).manual_seed(1)
    out = {}
    for timed in (False, True):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        env.rollout(policy, T, seed=1, first_step=0, record=record)
        torch.cuda.synchronize()
        out["rollout_ms"] = (time.perf_counter() - begin) * 1e3
        advantages, returns = S.mappo_advantages(record, value_norm, GAMMA, LAMBDA)
        indices = S.minibatch_indices(T * worlds * env.n_players, 1, EPOCHS, generator=shuffles, device=dev)
        torch.cuda.synchronize()
        begin = time.perf_counter()
        S.mappo_update(policy, optimizer, record, None, advantages, returns, indices, value_norm=value_norm, entropy_coef=ENT)
        torch.cuda.synchronize()
        out["update_ms"] = (time.perf_counter() - begin) * 1e3
    env.close()
    out["build_hash"] = _lib.build_hash()
    return out


def plain_ab(parent_tree, windows, worlds=1024):
    """this build against the parent's, a window per fresh process, alternating"""
    rows = {"this": [], "parent": []}
    for _ in range(windows):
        for side, tree in (("parent", os.path.abspath(parent_tree)), ("this", REPO)):
            env = dict(os.environ, MRL_PROBE_TREE=tree)
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--plain-window", str(worlds)], env=env, capture_output=True,
                                  text=True, timeout=300)
            if done.returncode:
                raise RuntimeError(f"the {side} window failed: {done.stderr[-500:]}")
            rows[side].append(json.loads(done.stdout.strip().splitlines()[-1]))
    out = {"worlds": worlds, "windows": windows}
    for side, got in rows.items():
        out[side] = {"build_hash": got[0]["build_hash"], "rollout": summary([g["rollout_ms"] for g in got]),
                     "update": summary([g["update_ms"] for g in got])}
    for what in ("rollout", "update"):
        out[f"{what}_inside_parent_spread_or_below"] = out["this"][what]["median_ms"] <= out["parent"][what]["max_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=WINDOWS)
    ap.add_argument("--worlds", type=int, nargs="*", default=list(WORLDS))
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its library built: also measure the plain path against it")
    ap.add_argument("--plain-window", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    if args.plain_window:
        print(json.dumps(plain_window(args.plain_window)), flush=True)
        return
    from madrona_rl_envs_playground_amd import _lib
    record = {"build_hash": _lib.build_hash(), "game": "balance", "hidden": 64, "layer_N": 2, "num_steps": T, "data_chunk_length": CHUNK,
              "epochs": EPOCHS, "minibatches": 1, "lr": LR, "entropy_coef": ENT, "windows": args.windows, "rows": {},
              "what": "ms per iteration (rollout of T steps, advantages, E minibatch steps over all chunks): host clock around one window "
                      "behind a device wait; *_iteration one wait at the end, the phases a wait each; windows of the two loops alternating "
                      "in one process.  plain_path: the non-recurrent rollout and update, this build against the parent's, a window per "
                      "process"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if os.path.exists(args.out):  # what an earlier call measured on the same build stays in the file
        with open(args.out) as f:
            earlier = json.load(f)
        if earlier.get("build_hash") == record["build_hash"] and earlier.get("windows") == args.windows:
            record["rows"].update(earlier.get("rows", {}))
            if "plain_path" in earlier:
                record["plain_path"] = earlier["plain_path"]

    def write():
        with open(args.out, "w") as f:  # (after every part: a later one that runs out of time leaves the earlier ones)
            json.dump(record, f, indent=1, sort_keys=True)
            f.write("\n")

    for worlds in args.worlds:
        record["rows"][str(worlds)] = measure(worlds, args.windows)
        print(worlds, json.dumps(record["rows"][str(worlds)]), flush=True)
        write()
    if args.parent_tree:
        record["plain_path"] = plain_ab(args.parent_tree, args.windows)
        print("plain path", json.dumps(record["plain_path"]), flush=True)
        write()
    print("->", args.out)


if __name__ == "__main__":
    main()
