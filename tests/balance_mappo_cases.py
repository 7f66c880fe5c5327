"""Weights, inputs, cases and seeds of the balance beam's MAPPO tests (tests/test_balance_mappo_api.py on the CPU,
tests/test_gpu_balance_mappo.py on the device); the twin is tests/mlpbase_twin.py.  The input conditions of every parity case --
properties of the twin, not of the device -- are asserted by the CPU test; a case that fails one gets another seed in ``SEEDS``.
Nothing here touches a GPU."""
import functools

import numpy as np
import torch

import mlpbase_twin as twin
from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic

WEIGHTS = ("reference", "trained")
INPUTS = ("stepped", "synthetic")
LAYER_NS = (1, 2)
T, N, P = 4, 33, 2      # the records of the update's cases: S = T * N * P = 264 samples
DISTINCT = 257          # distinct samples the width beyond the workgroup cap repeats
ACT_WORLDS = (3, 33, 65)  # 6, 66 and 130 samples: one ragged tile, a tile edge, two full tiles plus a ragged one
FIXED_SIZES = [1, 31, 33, 65, 257]
BEYOND_CAP = 8197       # 256 partial vectors x 32 samples + 5
CONSTANT_ROW = 0        # the synthetic inputs' sample of seven equal values: its variance is 0

# (layer_N, weights, inputs, B, variant)
UPDATE_CASES = ([(l, w, i, b, "default") for l in LAYER_NS for w in WEIGHTS for i in INPUTS for b in FIXED_SIZES + [BEYOND_CAP]] +
                [(2, "trained", "synthetic", 65, v) for v in sorted(twin.VARIANTS) if v != "default"])
# seed of a case's batch and index rows where the derived one fails the input conditions: replaced here, not excused there
SEEDS = {
    (1, 'reference', 'synthetic', 257, 'default'): 401899,
    (1, 'reference', 'synthetic', 8197, 'default'): 257479,
    (1, 'trained', 'stepped', 8197, 'default'): 358391,
    (1, 'trained', 'synthetic', 65, 'default'): 201564,
    (1, 'trained', 'synthetic', 8197, 'default'): 258488,
    (2, 'reference', 'synthetic', 31, 'default'): 300320,
    (2, 'reference', 'synthetic', 33, 'default'): 300334,
    (2, 'reference', 'synthetic', 257, 'default'): 1401902,
    (2, 'reference', 'synthetic', 8197, 'default'): 1457482,
    (2, 'trained', 'stepped', 65, 'default'): 301470,
    (2, 'trained', 'synthetic', 257, 'default'): 502911,
    (2, 'trained', 'synthetic', 8197, 'default'): 358491,
    (2, 'trained', 'synthetic', 65, 'no_valuenorm'): 301606,
}


@functools.lru_cache(maxsize=None)
def make_module(layer_N, weights):
    """``reference``: a fresh initialisation (seeded).  ``trained``: the same perturbed so that no tensor is at its initial value --
    LayerNorm weights away from 1 and biases from 0, Linear biases non-zero, heads of ordinary size."""
    torch.manual_seed(1000 + layer_N)
    module = MlpBaseActorCritic(layer_N=layer_N)
    if weights == "trained":
        gen = torch.Generator().manual_seed(77 + layer_N)
        with torch.no_grad():
            for name, p in module.named_parameters():
                noise = torch.randn(p.shape, generator=gen)
                if name.endswith("action_out.linear.weight"):
                    p.add_(0.3 * noise)
                elif p.dim() == 2:
                    p.add_(0.05 * noise)
                else:
                    p.add_(0.2 * noise)
    return module


@functools.lru_cache(maxsize=None)
def params_of(layer_N, weights):
    return twin.flat(make_module(layer_N, weights)).astype(np.float32)


def stepped_observations(n, seed, steps):
    """(P, n, 7) int32 of ``n`` worlds the CPU oracle stepped ``steps`` times with random actions: the rows real steps leave"""
    from oracle import oracle
    oracle.build()
    rng = np.random.default_rng(seed)
    orc = oracle.BalanceOracle(n)
    for _ in range(steps):
        orc.step(rng.integers(0, 4, size=(2, n)).astype(np.int32))
    obs = np.array(orc.obs, np.int32)
    orc.close()
    return obs


def synthetic_observations(n, seed):
    """(P, n, 7) int32: positions 0..8 and 0..2 steps left, independent of each other; sample ``CONSTANT_ROW`` (world 0, seat 0) is
    seven 2s"""
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 9, size=(P, n, 7)).astype(np.int32)
    obs[:, :, 6] = rng.integers(0, 3, size=(P, n))
    obs[0, 0, :] = 2
    return obs


# seeds of the act's inputs: 11 unless that puts a pre-activation too close to 0 at one of the weight sets
ACT_SEEDS = {(33, "stepped"): 12, (33, "synthetic"): 15, (65, "synthetic"): 20}


@functools.lru_cache(maxsize=None)
def act_inputs(n, inputs):
    """(P, n, 7) int32, read-only: what a test plants in OBSERVATION (the observation is the simulator's whole state)"""
    seed = ACT_SEEDS.get((n, inputs), 11)
    obs = stepped_observations(n, seed, 5) if inputs == "stepped" else synthetic_observations(n, seed)
    obs.setflags(write=False)
    return obs


def rows_of(obs):
    """the samples of a (P, n, 7) block in the kernels' order (n, p): (n * P, 7)"""
    return np.ascontiguousarray(obs.transpose(1, 0, 2)).reshape(-1, obs.shape[2])


def draws(seed, step, n, seats=(0, 1)):
    """u of every sample in (n, seat) order: ``(hash >> 8) * 2^-24`` of (seed, step, world, seat), float64 (exact)"""
    from madrona_rl_envs_playground_amd.simulators import random_hash
    world = np.repeat(np.arange(n), len(seats))
    seat = np.tile(np.asarray(seats), n)
    return (random_hash(seed, step, world, seat) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def record_obs(inputs, seed):
    """(T * N * P, 7) int32, samples in (t, n, p) order, read-only"""
    slots = [rows_of(stepped_observations(N, seed + t, 1 + t) if inputs == "stepped" else synthetic_observations(N, seed + t)) for t in range(T)]
    obs = np.ascontiguousarray(np.concatenate(slots))
    obs.setflags(write=False)
    return obs


def make_batch(params, layer_N, obs, seed, delta, valuenorm):
    """``mappo_twin.make_batch`` on this network: uniform actions, old log-prob = current + U(-0.4, 0.4), old value = current +
    U(-0.5, 0.5), targets = old value + N(0, 1.5 delta), advantages N(0, 1); with ValueNorm the returns are the targets
    denormalised by STATE0's mean and standard deviation"""
    rng = np.random.default_rng(seed)
    size = len(obs)
    now = twin.act(params, obs, np.zeros(size), layer_N)
    actions = rng.integers(0, twin.A, size=size).astype(np.int32)
    logprobs = (now["logp"][np.arange(size), actions] + rng.uniform(-0.4, 0.4, size=size)).astype(np.float32)
    values = (now["values"] + rng.uniform(-0.5, 0.5, size=size)).astype(np.float32)
    returns = values + rng.normal(scale=1.5 * delta, size=size)
    returns = ((twin.mappo_twin.RETURN_MEAN + twin.mappo_twin.RETURN_STD * returns) if valuenorm else returns).astype(np.float32)
    advantages = rng.normal(size=size).astype(np.float32)
    return twin.Batch(obs, actions, logprobs, values, returns, advantages)


def seed_of(case):
    layer_N, weights, inputs, width, variant = case
    derived = 100003 * layer_N + 1009 * WEIGHTS.index(weights) + 97 * INPUTS.index(inputs) + 7 * width + 13 * sorted(twin.VARIANTS).index(variant)
    return SEEDS.get(case, derived)


@functools.lru_cache(maxsize=None)
def fixed_case(case, rows=1):
    """Parameters, batch and index rows of a case, and for row 0 the twin and the float32 computation.  The width beyond the record
    repeats DISTINCT of its samples."""
    layer_N, weights, inputs, width, variant = case
    cfg = twin.VARIANTS[variant]
    params, seed = params_of(layer_N, weights), seed_of(case)
    batch = make_batch(params, layer_N, record_obs(inputs, 1000 + seed % 97), seed, cfg.huber_delta, cfg.valuenorm)
    size = len(batch.obs)
    if width > size:
        rng = np.random.default_rng(seed + 1)
        indices = rng.permutation(size)[:DISTINCT][rng.integers(0, min(DISTINCT, size), size=(rows, width))].astype(np.int32)
    else:
        indices = twin.make_indices(rows, width, size, seed)
    return {"layer_N": layer_N, "params": params, "batch": batch, "indices": indices, "cfg": cfg,
            "twin": twin.row(params, layer_N, batch, indices[0], cfg, twin.STATE0),
            "f32": twin.row(params, layer_N, batch, indices[0], cfg, twin.STATE0, dtype=torch.float32)}


@functools.lru_cache(maxsize=None)
def stat_margins(layer_N, weights):
    """d of every scalar stat at one (layer_N, weight set): the largest distance of the float32 computation from the twin over
    its cases (tests/ppo_twin.py ``stat_margins`` and DESIGN.md section 13 say why one row's own distance bounds nothing)"""
    d = {name: 0.0 for name in twin.STATS}
    for case in UPDATE_CASES:
        if case[:2] != (layer_N, weights):
            continue
        fixed = fixed_case(case)
        own = twin.row_margins(fixed["twin"], fixed["f32"])
        for name in twin.STATS:
            d[name] = max(d[name], own[name])
    return d


@functools.lru_cache(maxsize=None)
def act_margins(layer_N, weights):
    """(d of the values, d of the log-probs, d of the logits) at one (layer_N, weight set): the largest over the act's cases"""
    per_case = [twin.act_margins(params_of(layer_N, weights), rows_of(act_inputs(n, inputs)), layer_N) for n in ACT_WORLDS for inputs in INPUTS]
    return tuple(max(m[k] for m in per_case) for k in range(3))
