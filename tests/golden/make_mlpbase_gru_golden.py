"""Generator of tests/golden/mlpbase_gru_ref.npz: the reference's own ``R_Actor`` / ``R_Critic`` (train/MAPPO/r_actor_critic.py,
imported at run time from a reference checkout, as tests/golden/make_balance_mlpbase_golden.py imports them) built with
``use_recurrent_policy=True``, ``hidden_size=64``, ``recurrent_N=1`` over this repository's ``spaces`` for the balance beam, with a
seeded initialisation, in float64 on the CPU.  The file is data only: per ``layer_N`` in (1, 2) the parameters' names and sizes in ``parameters_to_vector`` order, and for
``layer_N`` 2 the flat parameter vector (actor, then critic; float32 values, every one exact); 16 observation rows, states and masks with the logits,
values and new states of one step through the reference's ``base``, ``rnn`` (``RNNLayer``) and head; and one evaluation of an
(L = 3, N = 5) chunk batch whose masks are zero in the middle step of two chunks and at the first step of one -- ``RNNLayer``'s
segment logic (utils/rnn.py:41-69) -- with the log-probabilities of given actions, the entropy and the values.  It pins the twin
(tests/mlpbase_gru_twin.py) and ``MlpBaseGruActorCritic`` to the reference on machines without the reference tree;
tests/test_balance_gru_api.py regenerates and compares it where the tree is present.

    python tests/golden/make_mlpbase_gru_golden.py          # rewrites the file
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mlpbase_gru_ref.npz")
ROWS, SEED, L, N = 16, 20270, 3, 5
LAYER_NS = (1, 2)
NUMBERS_OF = 2  # the layer_N whose parameters and outputs the file holds; the other's names and sizes only (the file's size)


def plain_generator():
    """the non-recurrent generator beside this file: where the reference is, its classes, the arguments they read"""
    spec = importlib.util.spec_from_file_location("make_balance_mlpbase_golden", os.path.join(HERE, "make_balance_mlpbase_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def reference_present():
    return plain_generator().reference_present()


def arguments(layer_N):
    args = plain_generator().arguments(layer_N)
    args.use_recurrent_policy = True
    return args


def inputs():
    rng = np.random.default_rng(SEED)

    def rows(count):
        out = rng.integers(0, 9, size=(count, 7)).astype(np.int32)
        out[:, 6] = rng.integers(0, 3, size=count)
        return out

    act_masks = (rng.random(ROWS) < 0.7).astype(np.float64)
    act_masks[0], act_masks[1] = 0.0, 1.0
    chunk_masks = np.ones((L, N))
    chunk_masks[1, 1] = chunk_masks[1, 3] = chunk_masks[0, 2] = 0.0
    return {"rows": rows(ROWS), "h_actor": 0.5 * rng.normal(size=(ROWS, 64)), "h_critic": 0.5 * rng.normal(size=(ROWS, 64)), "masks": act_masks,
            "chunk_rows": rows(L * N).reshape(L, N, 7), "chunk_h_actor": 0.5 * rng.normal(size=(N, 64)),
            "chunk_h_critic": 0.5 * rng.normal(size=(N, 64)), "chunk_masks": chunk_masks,
            "chunk_actions": rng.integers(0, 4, size=(L, N)).astype(np.int64)}


def generate():
    from madrona_rl_envs_playground_amd.spaces import Discrete, MultiDiscrete
    R_Actor, R_Critic = plain_generator().reference_classes()
    obs_space, act_space = MultiDiscrete([9] * 6 + [3]), Discrete(4)
    out = inputs()
    t = lambda a: torch.from_numpy(np.asarray(a)).double()  # noqa: E731
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
                    p.copy_(p.float().double())  # float32 values, so that the file can hold them as float32 without loss
            tag = f"n{layer_N}"
            for which, net in (("actor", actor), ("critic", critic)):
                out[f"{tag}/{which}/parameter_names"] = np.array([name for name, _ in net.named_parameters()])
                out[f"{tag}/{which}/parameter_sizes"] = np.array([p.numel() for p in net.parameters()])
            if layer_N != NUMBERS_OF:
                continue
            flat = torch.cat([torch.nn.utils.parameters_to_vector(net.parameters()) for net in (actor, critic)])
            out[f"{tag}/params"] = flat.float().numpy().copy()
            # one step: rnn_states are (n, recurrent_N, hidden), masks (n, 1)
            x, masks = t(out["rows"]), t(out["masks"]).unsqueeze(1)
            features, h_actor = actor.rnn(actor.base(x), t(out["h_actor"]).unsqueeze(1), masks)
            out[f"{tag}/logits"] = actor.act.action_out.linear(features).numpy().copy()
            out[f"{tag}/new_h_actor"] = h_actor[:, 0].numpy().copy()
            features, h_critic = critic.rnn(critic.base(x), t(out["h_critic"]).unsqueeze(1), masks)
            out[f"{tag}/values"] = critic.v_out(features)[:, 0].numpy().copy()
            out[f"{tag}/new_h_critic"] = h_critic[:, 0].numpy().copy()
            # a chunk batch, flattened (L * N, ...) with N states: the branch of RNNLayer.forward that cuts at zero masks
            x, masks = t(out["chunk_rows"]).reshape(L * N, 7), t(out["chunk_masks"]).reshape(L * N, 1)
            features, h_actor = actor.rnn(actor.base(x), t(out["chunk_h_actor"]).unsqueeze(1), masks)
            dist = actor.act.action_out(features)
            out[f"{tag}/chunk_logp"] = dist.log_probs(torch.from_numpy(out["chunk_actions"]).reshape(L * N, 1)).reshape(L, N).numpy().copy()
            out[f"{tag}/chunk_entropy"] = np.array(dist.entropy().mean().item())
            out[f"{tag}/chunk_h_actor_out"] = h_actor[:, 0].numpy().copy()
            features, h_critic = critic.rnn(critic.base(x), t(out["chunk_h_critic"]).unsqueeze(1), masks)
            out[f"{tag}/chunk_values"] = critic.v_out(features).reshape(L, N).numpy().copy()
            out[f"{tag}/chunk_h_critic_out"] = h_critic[:, 0].numpy().copy()
    return out


def main():
    if not reference_present():
        raise SystemExit("no reference tree")
    np.savez_compressed(OUT, **generate())
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
