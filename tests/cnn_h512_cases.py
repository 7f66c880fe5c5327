"""The cases of the hidden-512 CNN act's tests (tests/test_cnn_h512_api.py, tests/test_gpu_cnn_h512.py): kitchens, modules, inputs,
and the reference -- ``CnnActorCritic(W, H, F, hidden=512)`` in float64 on the CPU, on the (N, W, H, F) view.  d of a case is the
distance of the same module in float32 from it, per kind.  Nothing here touches a GPU."""
import copy
import functools

import numpy as np
import torch

import cnn_twin as twin
import kitchen_shape_cases
import simplecooked_cnn_cases
from madrona_rl_envs_playground_amd import layouts
from madrona_rl_envs_playground_amd.simulators import CnnActorCritic

HIDDEN, CHANNELS, HORIZON = 512, 256, 400
# key: (simulator class's name, its parameters, (W, H, P, F)).  npos 1 (the smallest); npos 6; F = 15, 9 F odd: the padded product;
# npos 21: fc1's longest K and the largest channel-loop image of the named layouts
KITCHENS = {
    "k3x3p1": ("OvercookedSimulator", lambda h: kitchen_shape_cases.layout_params("k3x3p1", h), (3, 3, 1, 21)),
    "cramped_room": ("OvercookedSimulator", lambda h: layouts.get_base_layout_params("cramped_room", h), (5, 4, 2, 26)),
    "simple/1p": ("SimplecookedSimulator", lambda h: simplecooked_cnn_cases.layout_params("simple/1p", h), (5, 4, 1, 15)),
    "asymmetric_advantages": ("OvercookedSimulator", lambda h: layouts.get_base_layout_params("asymmetric_advantages", h), (9, 5, 2, 26)),
}
WORLDS = (3, 33, 65)  # N * P is never a multiple of 32: one tile, a ragged second tile, five tiles
WEIGHTS = twin.WEIGHTS
# (key, worlds, weights, seats): all seats everywhere, seat 1 alone where there is one
FORWARD = [(key, n, weights, seats) for key in KITCHENS for n in WORLDS for weights in WEIGHTS
           for seats in ((None, 2) if KITCHENS[key][2][2] > 1 else (None,))]
INTEGER_KEYS = ("cramped_room", "asymmetric_advantages")

@functools.lru_cache(maxsize=None)
def module_of(w, h, f, weights):
    """the reference's initialisation (head gain 0.01), or ``cnn_twin.make_module``'s "trained" perturbation of it"""
    torch.manual_seed(twin.MODULE_SEED)
    module = CnnActorCritic(w, h, f, hidden=HIDDEN)
    if weights == "trained":
        with torch.no_grad():
            for name, p in module.named_parameters():
                if name.endswith("bias"):
                    p.normal_(0.0, 0.1)
                else:
                    p.normal_(0.0, 0.3 if "action_out" in name or "v_out" in name else (2.0 / p[0].numel()) ** 0.5)
    return module

def make_module(key, weights):
    w, h, _, f = KITCHENS[key][2]
    return module_of(w, h, f, weights)

@functools.lru_cache(maxsize=None)
def observations(key, n, seed):
    """(N, P, H, W, F) int8: a quarter ones, some counts up to 20, a few negative"""
    w, h, p, f = KITCHENS[key][2]
    rng = np.random.default_rng(seed)
    size = (n, p, h, w, f)
    obs = np.where(rng.uniform(size=size) < 1.0 / 16, rng.integers(-3, 21, size=size), rng.uniform(size=size) < 0.25).astype(np.int8)
    obs.setflags(write=False)
    return obs

def evaluate(module, obs, dtype):
    """values (N P,), logits and log-probs (N P, 6) as float64 arrays, of the module cast to ``dtype``"""
    with torch.no_grad():
        net = copy.deepcopy(module).to(dtype)
        x = torch.from_numpy(np.array(twin.rows_of(obs))).transpose(1, 2).to(dtype)
        logits = net.actor(x)
        return net.critic(x)[:, 0].double().numpy(), logits.double().numpy(), torch.log_softmax(logits, dim=1).double().numpy()

@functools.lru_cache(maxsize=None)
def reference(key, n, weights):
    """the float64 module on the case's observations, the draws, and d per kind"""
    seed = 7919 * n + 104729 * WEIGHTS.index(weights) + 41 * list(KITCHENS).index(key) + 3
    module, obs = make_module(key, weights), observations(key, n, seed)
    values, logits, logp = evaluate(module, obs, torch.float64)
    v32, l32, lp32 = evaluate(module, obs, torch.float32)
    u = twin.draws(seed, 0, n, obs.shape[1])
    cdf = np.cumsum(np.exp(logp), axis=1)[:, :-1]
    return {"obs": obs, "seed": seed, "values": values, "logits": logits, "logp": logp, "u": u, "cdf": cdf,
            "actions": (u[:, None] >= cdf).sum(axis=1).astype(np.int32), "near": twin.near_boundary(cdf, u),
            "d_value": float(np.abs(v32 - values).max()), "d_logp": float(np.abs(lp32 - logp).max()),
            "d_logits": float(np.abs(l32 - logits).max())}

@functools.lru_cache(maxsize=None)
def integer_case_of(w, h, p, f, n=33, seed=99, fc1_one_in=64):
    """small-integer layers and observations as ``cnn_twin.integer_layers`` builds them at 64, every partial sum below 2^24; one
    weight of fc1 in ``fc1_one_in`` is nonzero"""
    k2, rng, layers = CHANNELS * (w - 2) * (h - 2), np.random.default_rng(seed), {}
    sparse = lambda shape, lo, hi, one_in: (rng.integers(lo, hi, size=shape) * (rng.uniform(size=shape) < 1.0 / one_in)).astype(np.int64)  # noqa: E731
    for name, out in (("actor", twin.A), ("critic", 1)):
        c, ff, i, j = np.meshgrid(np.arange(CHANNELS), np.arange(f), np.arange(3), np.arange(3), indexing="ij")
        conv = ((c * 131 + ff * 31 + i * 7 + j * 3) % 9 - 4 + rng.integers(-1, 2, size=c.shape)).astype(np.int64)
        o, k = np.meshgrid(np.arange(HIDDEN), np.arange(k2), indexing="ij")
        fc1 = (((o * 17 + k * 5) % 7 - 3) * (rng.uniform(size=o.shape) < 1.0 / fc1_one_in)).astype(np.int64)
        bias = lambda size: rng.integers(-3, 4, size=size).astype(np.int64)  # noqa: E731
        layers[name] = [(conv, bias(CHANNELS)), (fc1, bias(HIDDEN)), (sparse((HIDDEN, HIDDEN), -1, 2, 32), bias(HIDDEN)),
                        (sparse((out, HIDDEN), -2, 3, 16), bias(out))]
    size = (n, p, h, w, f)
    obs = (rng.integers(-1, 4, size=size) * (rng.uniform(size=size) < 0.2)).astype(np.int8)
    return layers, obs

def integer_case(key, n=33, seed=99):
    return integer_case_of(*KITCHENS[key][2], n=n, seed=seed)
