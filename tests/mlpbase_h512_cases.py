"""Weights, inputs, cases and the reference of the hidden-512 MLPBase tests: the torch module ``MlpBaseActorCritic(hidden=512)`` in
float64; d is the float32 module's distance from it on the same case.  Nothing here touches a GPU."""
import functools

import numpy as np
import torch

import balance_mappo_cases as beam
import mlpbase_twin as twin
from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic

HIDDEN = 512
SIZES = {2: (798226, 796687), 1: (534546, 533007)}  # layer_N -> (actor, critic) floats
FC_H, FC_H_AT = HIDDEN * HIDDEN + 3 * HIDDEN, 14 + HIDDEN * 7 + 3 * HIDDEN  # the unused block's floats per net and where it starts
WEIGHTS = ("init", "trained", "dead")
SHAPES = ((1, (0, 1)), (33, (0, 1)), (65, (1,)))    # (worlds, seats): one row pair, a tile edge, two tiles and a ragged one
WIDE = (2049, (0, 1))                               # 4098 samples: the 64-row tiles, the last one ragged
FORWARD = [(l, w, n, s) for l in (1, 2) for w in WEIGHTS for n, s in SHAPES] + [(2, "init") + WIDE]  # (layer_N, weights, worlds, seats)
SEED, STEP, ROW = 17, 5, 1


@functools.lru_cache(maxsize=None)
def make_module(layer_N, weights):
    """``init``: the module's own initialisation (seeded).  ``trained``: perturbed as tests/balance_mappo_cases.py does.  ``dead``:
    the trained one with both fc1 biases at -1000: the first layer is dead behind the ReLU and its LayerNorm rows have variance 0."""
    torch.manual_seed(2000 + layer_N)
    module = MlpBaseActorCritic(hidden=HIDDEN, layer_N=layer_N)
    if weights != "init":
        gen = torch.Generator().manual_seed(177 + layer_N)
        with torch.no_grad():
            for name, p in module.named_parameters():
                noise = torch.randn(p.shape, generator=gen)
                p.add_((0.3 if name.endswith("action_out.linear.weight") else 0.05 if p.dim() == 2 else 0.2) * noise)
            if weights == "dead":
                for net in (module.actor, module.critic):
                    net.base.mlp.fc1[0].bias.fill_(-1000.0)
    return module


@functools.lru_cache(maxsize=None)
def observations(n):
    """(P, n, 7) int32 over the beam's whole value range, read-only; world 0, seat 1 is seven 2s: a LayerNorm(7) row of variance 0"""
    obs = beam.synthetic_observations(n, 500 + n)  # (another seed where more than one draw of a case lies within 1e-5 of a boundary)
    obs[0, 0, :] = np.arange(7) % 3
    obs[1, 0, :] = 2
    obs.setflags(write=False)
    return obs


def head(module, rows, u):
    """mlpbase_twin.act's arrays for ``module`` (of any dtype)"""
    with torch.no_grad():
        values, logits, _ = twin.forward(module, rows)
        logp = torch.log_softmax(logits, dim=1)
    values, logits, logp = (t.double().numpy() for t in (values, logits, logp))
    cdf = np.cumsum(np.exp(logp), axis=1)[:, :-1]
    return {"values": values, "logits": logits, "logp": logp, "cdf": cdf,
            "actions": (np.asarray(u, np.float64)[:, None] >= cdf).sum(axis=1).astype(np.int32)}


@functools.lru_cache(maxsize=None)
def forward_case(layer_N, weights, n, seats):
    """rows, u, ``exact`` (the float64 reference), ``d`` (the float32 module's distance from it), ``near`` (draws within 1e-5 of a boundary)"""
    module = make_module(layer_N, weights)
    rows = beam.rows_of(observations(n)[list(seats)])
    u = beam.draws(SEED, STEP, n, seats)
    wide = MlpBaseActorCritic(hidden=HIDDEN, layer_N=layer_N).double()  # the float32 values, exactly
    wide.load_state_dict({k: v.double() for k, v in module.state_dict().items()})
    exact, single = head(wide, rows, u), head(module, rows, u)
    return {"rows": rows, "u": u, "exact": exact, "near": twin.near_boundary(exact["cdf"], u),
            "d": tuple(float(np.abs(single[k] - exact[k]).max()) for k in ("values", "logp", "logits"))}
