#!/usr/bin/env python3
"""What the collection phase of ``CleanPPOAgent`` costs on the device against the torch loop of the reference's agent: us per
collected step and per update-boundary advantage pass, written to profiles/agent_act_cost.json under the library's build hash.

    python tools/agent_act_probe.py           measure (needs the GPU)

One collected step = ego act, partner act, environment step, two credits.  Two loops, in one process, in ALTERNATING windows,
five windows each after one that warms both up, medians and extremes reported:
  device   ``agent_act`` x 2, ``sim.step()``, ``agent_credit`` x 2 (mrl_agent_act / mrl_agent_credit), recording;
  torch    the same agent written with torch on ``policy.module()`` as the reference's lines do it
           (pantheonrl_extension/vectoragent.py:197-219, :352-372): float casts of observation and state, both nets for every
           world, the masked ``Categorical``, ``log_prob``, the buffer row writes into float buffers, and in ``update`` the
           ``torch.any(dones)`` the host waits for.  (Its reward credit uses the per-world cell ``rewards[last_active, w]``,
           which is cheaper than the reference's row selection.)
The advantage pass: ``gae_active`` (mrl_gae_active) against the reference's backward loop with boolean-mask indexing (:231-262),
on the same recorded buffers.
Sizes: the balance beam at 120 and 32768 worlds, Hanabi `full` at 1000 and 65536; T = 128 rows (the 65536-world buffers hold 16
rows, written round and round: 128 rows of float copies would not fit beside the device path's).
``device_below_torch``: the device loop's median lies below the torch loop's by more than the two loops' spreads (max - min) added."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
OUT = os.path.join(REPO, "profiles", "agent_act_cost.json")
CASES = (("balance", 120), ("balance", 32768), ("hanabi_full", 1000), ("hanabi_full", 65536))
WINDOWS = 5


def make_sim(game, n):
    from madrona_rl_envs_playground_amd.envs.hanabi_env import FULL_CONFIG as c
    from madrona_rl_envs_playground_amd.simulators import BalanceBeamSimulator, ExecMode, HanabiSimulator
    if game == "balance":
        return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n), (7, 7, 4)
    sim = HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, colors=c["colors"], ranks=c["ranks"], players=c["players"],
                          max_information_tokens=c["max_information_tokens"], max_life_tokens=c["max_life_tokens"])
    return sim, (658, 783, 20)


class TorchAgent:
    """the reference's per-step work, on policy.module()"""

    def __init__(self, module, rows, n, dims, device):
        import torch
        d, s, a = dims
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
        self.module, self.rows, self.step = module, rows, 0
        self.obs, self.states, self.masks = z(rows, n, d), z(rows, n, s), z(rows, n, a)
        self.actions, self.logprobs, self.rewards, self.dones, self.values = (z(rows, n) for _ in range(5))
        self.active = z(rows, n, dtype=torch.bool)
        self.next_done, self.new_game = z(n, dtype=torch.bool), z(n, dtype=torch.bool)
        self.running, self.last_active = z(n), z(n, dtype=torch.long)
        self.worlds = torch.arange(n, device=device)
        self.return_sum, self.returns = 0, 0

    def act(self, active, obs, state, mask):
        import torch
        with torch.no_grad():
            action, logprob, _, value = self.module.get_action_and_value(obs.float(), state.float(), mask)
        k = self.step % self.rows
        self.values[k] = value.flatten()
        self.obs[k], self.states[k], self.masks[k] = obs, state, mask
        self.dones[k], self.active[k], self.actions[k], self.logprobs[k] = self.next_done, active, action, logprob
        self.next_done[:] = False
        self.rewards[k] = 0
        self.last_active[active] = k
        self.new_game[active] = False
        return action

    def update(self, rewards, dones):
        import torch
        dones = dones.to(torch.bool)
        self.running += rewards
        self.rewards[self.last_active, self.worlds] += torch.where(self.new_game, 0, rewards)
        self.next_done |= dones
        if torch.any(dones):  # the host waits here, every step
            self.return_sum += torch.mean(self.running[dones])
            self.returns += 1
            self.running[dones] = 0.0
            self.new_game[dones] = True
        self.step += 1


def torch_gae(active, rewards, values, dones, next_done, next_value, next_active, gamma, lam):
    """the reference's backward loop (:231-262) on clones of the buffers"""
    import torch
    active = active.clone()
    num_steps, n = rewards.shape
    advantages = torch.zeros_like(rewards)
    delta, lastgaelam = torch.zeros(n, device=rewards.device), torch.zeros(n, device=rewards.device)
    bootstrapped = next_active.clone()
    nnt, nv = torch.zeros_like(delta), torch.zeros_like(delta)
    nnt[bootstrapped] = 1.0 - next_done[bootstrapped].float()
    nv[bootstrapped] = next_value[bootstrapped]
    for t in reversed(range(num_steps)):
        mask = active[t]
        compute = mask
        if not torch.all(bootstrapped):
            compute = mask & ~bootstrapped
            bootstrapped |= mask
            active[t, compute] = False
        delta[compute] = rewards[t, compute] + gamma * nv[compute] * nnt[compute] - values[t, compute]
        advantages[t, compute] = lastgaelam[compute] = delta[compute] + gamma * lam * nnt[compute] * lastgaelam[compute]
        nnt[mask] = 1.0 - dones[t, mask]
        nv[mask] = values[t, mask]
    return advantages, advantages + values


def measure(game, n):
    import torch
    from madrona_rl_envs_playground_amd.simulators import AgentRecord, WideAgent, WidePolicy, agent_act, agent_credit, gae_active
    device = torch.device("cuda", 0)
    sim, dims = make_sim(game, n)
    d, s, a = dims
    rows = 128 if n < 65536 else 16
    steps = 32 if n <= 1000 else 8
    torch.manual_seed(0)
    policies = [WidePolicy.from_module(WideAgent(d, s, a, orthogonal=True), device=device) for _ in range(2)]
    obs_t, state_t = sim.observation_tensor().to_torch(), sim.agent_state_tensor().to_torch()
    mask_t, active_t = sim.action_mask_tensor().to_torch(), sim.active_agent_tensor().to_torch()
    action_t, reward_t, done_t = sim.action_tensor().to_torch(), sim.reward_tensor().to_torch(), sim.done_tensor().to_torch()
    records = [AgentRecord(rows, n, d, s, a, obs_t.dtype, state_t.dtype, device) for _ in range(2)]
    torch_agents = [TorchAgent(p.module(), rows, n, dims, device) for p in policies]
    counter = [0]

    def device_window():
        for _ in range(steps):
            k = counter[0]
            for p in range(2):
                agent_act(sim, p, policies[p], records[p], row=k % rows, seed=1, step=k)
            sim.step()
            for p in range(2):
                agent_credit(records[p], reward_t[p], done_t)
            counter[0] += 1

    def torch_window():
        for _ in range(steps):
            for p in range(2):
                action = torch_agents[p].act(active_t[p].to(torch.bool), obs_t[p, :, :d], state_t[p, :, :s], mask_t[p, :, :a].to(torch.bool))
                action_t[p, :, 0] = action
            sim.step()
            for p in range(2):
                torch_agents[p].update(reward_t[p], done_t)

    def timed(fn, per):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - start) * 1e6 / per

    r = records[0]

    def device_gae():
        agent_act(sim, 0, policies[0], r, value_only=True)
        r.active.copy_(saved_active)
        gae_active(r, 0.99, 0.95)

    def reference_gae():
        with torch.no_grad():
            next_value = policies[0].module().get_value(state_t[0, :, :s].float()).reshape(-1)
        torch_gae(saved_active.bool(), r.rewards, r.values, r.dones, r.next_done.bool(), next_value, active_t[0].to(torch.bool), 0.99, 0.95)

    device_window(), torch_window()  # warm-up; the record now holds real rows
    for _ in range(rows // steps):
        device_window()
    saved_active = r.active.clone()
    device_gae(), reference_gae()
    times = {"device_step": [], "torch_step": [], "device_gae": [], "torch_gae": []}
    for _ in range(WINDOWS):
        times["device_step"].append(timed(device_window, steps))
        times["torch_step"].append(timed(torch_window, steps))
        times["device_gae"].append(timed(device_gae, 1))
        times["torch_gae"].append(timed(reference_gae, 1))
    sim.close()

    def summary(xs):
        return {"median_us": round(statistics.median(xs), 1), "min_us": round(min(xs), 1), "max_us": round(max(xs), 1)}

    out = {"game": game, "worlds": n, "rows": rows, "steps_per_window": steps}
    out.update({k: summary(v) for k, v in times.items()})
    for kind in ("step", "gae"):
        dev, ref = times[f"device_{kind}"], times[f"torch_{kind}"]
        out[f"{kind}_device_below_torch"] = statistics.median(dev) + (max(dev) - min(dev)) + (max(ref) - min(ref)) < statistics.median(ref)
    return out


def main():
    from madrona_rl_envs_playground_amd import _lib
    results = [measure(game, n) for game, n in CASES]
    for r in results:
        print(json.dumps(r))
    report = {"build_hash": _lib.build_hash(), "unit": "us per collected step (two acts, the step, two credits) / per advantage pass",
              "windows": WINDOWS, "cases": results}
    if os.path.isdir(os.path.dirname(OUT)):
        with open(OUT, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")

if __name__ == "__main__":
    main()
