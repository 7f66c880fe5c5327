"""Generator of tests/golden/balance_mlpbase_ref.npz: the reference's own ``R_Actor`` / ``R_Critic`` (train/MAPPO/
r_actor_critic.py, imported at run time from a reference checkout: ``oracle.ref.default_reference_dir()``) built over this
repository's ``spaces`` for the balance beam, with a seeded initialisation, in float64 on the CPU.  The file is data only: per
``layer_N`` in (1, 2) the state-dict tensors of both nets under their own names, 64 observation rows, and the logits, greedy
actions and values the reference computes for them.  It pins the twin (tests/mlpbase_twin.py) and ``MlpBaseActorCritic`` to the
reference on machines without the reference tree; tests/test_balance_mappo_api.py regenerates and compares it where the tree is
present.

    python tests/golden/make_balance_mlpbase_golden.py          # rewrites the file
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
OUT = os.path.join(HERE, "balance_mlpbase_ref.npz")
ROWS, SEED = 64, 20260
LAYER_NS = (1, 2)


def reference_dir():
    from oracle import ref
    return os.path.abspath(ref.default_reference_dir())


def reference_present():
    return os.path.isfile(os.path.join(reference_dir(), "train", "MAPPO", "r_actor_critic.py"))


def reference_classes():
    """(R_Actor, R_Critic) of the reference checkout"""
    root = reference_dir()
    if root not in sys.path:
        sys.path.insert(1, root)
    module = importlib.import_module("train.MAPPO.r_actor_critic")
    return module.R_Actor, module.R_Critic


def arguments(layer_N):
    """what R_Actor / R_Critic read of train/config.py's namespace, at its defaults but hidden_size 64"""
    return argparse.Namespace(hidden_size=64, layer_N=layer_N, gain=0.01, use_orthogonal=True, use_policy_active_masks=True,
                              use_naive_recurrent_policy=False, use_recurrent_policy=False, recurrent_N=1, use_feature_normalization=True,
                              use_ReLU=True, stacked_frames=1, use_popart=False)


def observation_rows():
    """64 rows in the balance beam's range: positions 0..8, 0..2 steps left; row 0 is seven equal values"""
    rng = np.random.default_rng(SEED)
    rows = rng.integers(0, 9, size=(ROWS, 7)).astype(np.int32)
    rows[:, 6] = rng.integers(0, 3, size=ROWS)
    rows[0] = 2
    return rows


def generate():
    from madrona_rl_envs_playground_amd.spaces import Discrete, MultiDiscrete
    R_Actor, R_Critic = reference_classes()
    obs_space, act_space = MultiDiscrete([9] * 6 + [3]), Discrete(4)
    rows = observation_rows()
    out = {"rows": rows}
    for layer_N in LAYER_NS:
        torch.manual_seed(SEED + layer_N)
        actor, critic = R_Actor(arguments(layer_N), obs_space, act_space).double(), R_Critic(arguments(layer_N), obs_space).double()
        with torch.no_grad():
            # away from the initial values a wrong order would not show at: biases 0, LayerNorm (1, 0)
            gen = torch.Generator().manual_seed(SEED + 10 + layer_N)
            for net in (actor, critic):
                for p in net.parameters():
                    if p.dim() == 1:
                        p.add_(0.25 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
            x = torch.from_numpy(rows).double()
            features = actor.base(x)
            logits = actor.act.action_out(features).logits  # the Categorical's, normalised: log-probabilities
            raw = actor.act.action_out.linear(features)
            values = critic.v_out(critic.base(x))[:, 0]
        tag = f"n{layer_N}"
        names = {"actor": [], "critic": []}
        for which, net in (("actor", actor), ("critic", critic)):
            for name, tensor in net.state_dict().items():
                out[f"{tag}/{which}/{name}"] = tensor.numpy().copy()
                names[which].append(name)
            out[f"{tag}/{which}/names"] = np.array(names[which])
            out[f"{tag}/{which}/parameter_names"] = np.array([name for name, _ in net.named_parameters()])
        out[f"{tag}/logits"] = raw.numpy().copy()
        out[f"{tag}/logp"] = logits.numpy().copy()
        out[f"{tag}/greedy"] = raw.argmax(dim=1).numpy().astype(np.int32)
        out[f"{tag}/values"] = values.numpy().copy()
    return out


def main():
    if not reference_present():
        raise SystemExit(f"no reference tree at {reference_dir()}")
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
