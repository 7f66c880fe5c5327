"""Container-only generator of tests/golden/cleanppo_gae.npz: the reference's own ``CleanPPOAgent``
(/root/reference/pantheonrl_extension/vectoragent.py) driven on the CPU through T = 8 recorded steps and one update boundary,
for N = 5 and N = 70 worlds in two regimes each.  The fixture holds inputs and outputs only: what the agent was fed (activity,
rewards, dones), its bookkeeping arrays after every ``update`` call, its buffers in front of the boundary, and the advantages,
returns and cleared ``active`` flags its advantage loop produced.

  "coupled":   worlds take turns (a random parity each) and every fifth world falls silent three steps before the end, so some
               worlds are bootstrapped from the closing observation and others only at T - 4 or earlier: the reference's
               ``if not torch.all(bootstrapped)`` branch is taken down to that step.
  "together":  every world is active at every step and at the closing observation: the branch is never taken.

The advantages are locals of ``get_action``; they are read from its frame when it calls ``np.var`` (vectoragent.py:329), with
``update_epochs=0`` so that nothing is trained in between.

    python tests/golden/make_cleanppo_golden.py
"""
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()
from pantheonrl_extension.vectoragent import CleanPPOAgent  # noqa: E402  (the reference's)
from pantheonrl_extension.vectorobservation import VectorObservation  # noqa: E402

T, D, A = 8, 3, 4


def activity(regime, n, rng):
    """(T + 1, n) bool: row T is the closing observation's flag"""
    if regime == "together":
        return np.ones((T + 1, n), bool)
    parity = rng.integers(0, 2, size=n)
    parity[:5] = np.arange(5) % 2  # (both kinds of world at N = 5 too: 0, 2, 4 act at the closing observation, 3 last acts at t = 3)
    act = (np.arange(T + 1)[:, None] + parity[None, :]) % 2 == 0
    act[T - 3:, np.arange(n) % 5 == 3] = False
    return act


def run(regime, n, seed):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    space = SimpleNamespace(shape=(D,))
    envs = SimpleNamespace(num_envs=n, observation_space=space, share_observation_space=space,
                           action_space=SimpleNamespace(n=A, shape=()))
    agent = CleanPPOAgent(envs, "golden", torch.device("cpu"), num_updates=4, verbose=False, num_steps=T, update_epochs=0)
    act = activity(regime, n, rng)
    rewards_in = rng.choice([0.0, 1.0, -1.0, 0.5], size=(T, n)).astype(np.float32)
    dones_in = rng.uniform(size=(T, n)) < 0.15
    obs = rng.integers(0, 3, size=(T + 1, n, D)).astype(np.float32)

    def observation(t):
        x = torch.from_numpy(obs[t])
        return VectorObservation(torch.from_numpy(act[t]), x, x, torch.ones((n, A), dtype=torch.bool))

    trace = {k: [] for k in ("running_rewards", "next_done", "new_game", "last_active", "rewards")}
    for t in range(T):
        agent.get_action(observation(t))
        agent.update(torch.from_numpy(rewards_in[t]), torch.from_numpy(dones_in[t]))
        for k in trace:
            trace[k].append(getattr(agent, k).clone().numpy())
    before = {k: getattr(agent, k).clone().numpy() for k in ("rewards", "values", "dones", "active", "next_done")}

    grabbed = {}
    real_var = np.var

    def var_hook(*args, **kwargs):
        frame = sys._getframe(1)
        if "advantages" in frame.f_locals and "advantages" not in grabbed:
            for k in ("advantages", "returns", "next_value"):
                grabbed[k] = frame.f_locals[k].clone().numpy()
            grabbed["active_after"] = frame.f_locals["self"].active.clone().numpy()
        return real_var(*args, **kwargs)

    np.var = var_hook
    try:
        agent.get_action(observation(T))
    finally:
        np.var = real_var
    assert set(grabbed) == {"advantages", "returns", "next_value", "active_after"}
    out = {"activity": act, "rewards_in": rewards_in, "dones_in": dones_in, "gamma": np.float64(agent.gamma),
           "gae_lambda": np.float64(agent.gae_lambda)}
    out.update({"trace_" + k: np.stack(v) for k, v in trace.items()})
    out.update({"before_" + k: v for k, v in before.items()})
    out.update(grabbed)
    return out


def main():
    fixture = {}
    for n in (5, 70):
        for regime in ("coupled", "together"):
            for k, v in run(regime, n, 1000 * n + len(regime)).items():
                fixture[f"{regime}_{n}_{k}"] = v
    path = os.path.join(HERE, "cleanppo_gae.npz")
    np.savez_compressed(path, **fixture)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
