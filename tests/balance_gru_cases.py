"""Weights, inputs, cases and seeds of the recurrent balance-beam tests (tests/test_balance_gru_api.py on the CPU,
tests/test_gpu_balance_gru.py on the device); the twin is tests/mlpbase_gru_twin.py.  The input conditions of every case --
properties of the twin, not of the device -- are asserted by the CPU test; a case that fails one gets another seed in ``SEEDS``.
Nothing here touches a GPU."""
import functools

import numpy as np
import torch

import balance_mappo_cases as plain
import mlpbase_gru_twin as twin
from madrona_rl_envs_playground_amd.simulators import MlpBaseGruActorCritic

WEIGHTS = ("initial", "trained")
LAYER_NS = (1, 2)
STATES = ("zero", "nonzero")
ACT_WORLDS = plain.ACT_WORLDS  # 3, 33, 65 worlds: one ragged tile, a tile edge, two full tiles plus a ragged one
ACT_SEATS = ((0, 1), (1,))
P = 2
N = 17                  # worlds of the update's records: T = 2 L rows give 2 N P = 68 chunks
CHUNKS = (1, 31, 32, 33, 65)   # Bc: one chunk, a ragged tile, a full tile, one chunk past it, two tiles and one -- from 33 on two workgroups per net
LENGTHS = (1, 2, 10)    # L
# (layer_N, weights, Bc, L, variant)
UPDATE_CASES = ([(l, "trained", bc, length, "default") for l in LAYER_NS for bc in CHUNKS for length in LENGTHS] +
                [(2, "initial", 33, 10, "default"), (1, "initial", 33, 2, "default")] +
                [(2, "trained", 33, 10, v) for v in sorted(twin.VARIANTS) if v != "default"])
# seed of a case's batch and index rows where the derived one fails the input conditions: replaced here, not excused there
SEEDS = {}


@functools.lru_cache(maxsize=None)
def make_module(layer_N, weights):
    """``initial``: a fresh initialisation (seeded): orthogonal GRU weights, zero GRU biases.  ``trained``: the same perturbed so
    that no tensor is at its initial value -- the GRU's weights off the orthogonal ones, its biases non-zero, LayerNorm weights
    away from 1 and biases from 0, heads of ordinary size."""
    torch.manual_seed(2000 + layer_N)
    module = MlpBaseGruActorCritic(layer_N=layer_N)
    if weights == "trained":
        gen = torch.Generator().manual_seed(177 + layer_N)
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


rows_of, draws = plain.rows_of, plain.draws


@functools.lru_cache(maxsize=None)
def act_inputs(n, states):
    """What a test plants before an act, read-only: ``obs`` (P, n, 7) int32 drawn from ``common_pool``, ``h_actor`` / ``h_critic`` (n, P, 64) float32 (zero or
    N(0, 0.5)), ``done`` (n) int32 set in about a third of the worlds, world 0 among them and world 1 not"""
    rng = np.random.default_rng(31 * n + STATES.index(states))
    pool = common_pool()
    obs = np.ascontiguousarray(pool[rng.integers(0, len(pool), size=(P, n))])
    shape = (n, P, twin.HIDDEN)
    h_actor, h_critic = ((0.5 * rng.normal(size=shape)).astype(np.float32) if states == "nonzero" else np.zeros(shape, np.float32) for _ in range(2))
    done = (rng.random(n) < 0.35).astype(np.int32)
    done[0], done[min(1, n - 1)] = 1, 0
    out = {"obs": obs, "h_actor": h_actor, "h_critic": h_critic, "done": done}
    for a in out.values():
        a.setflags(write=False)
    return out


def act_twin_inputs(inputs, seats):
    """the twin's arguments for the samples of ``seats`` in (n, seat) order: rows, h_actor, h_critic, mask"""
    pick = list(seats)
    rows = rows_of(inputs["obs"][pick])
    h_actor, h_critic = (inputs[k][:, pick].reshape(-1, twin.HIDDEN) for k in ("h_actor", "h_critic"))
    mask = np.repeat(1.0 - inputs["done"].astype(np.float64), len(pick))
    return rows, h_actor, h_critic, mask


@functools.lru_cache(maxsize=None)
def act_margins(layer_N, weights):
    """d of every kind of ``twin.ACT_KINDS`` at one (layer_N, weight set): the largest over the act's cases"""
    d = {k: 0.0 for k in twin.ACT_KINDS}
    for n in ACT_WORLDS:
        for states in STATES:
            own = twin.act_margins(params_of(layer_N, weights), *act_twin_inputs(act_inputs(n, states), (0, 1)), layer_N)
            d = {k: max(d[k], own[k]) for k in d}
    return d


POOL_MARGIN = 1e-4  # a pool row's pre-activations in front of every ReLU are exactly 0 or at least this far from 0 (in the twin)


@functools.lru_cache(maxsize=None)
def obs_pool(layer_N, weights):
    """(k, 7) int32: the synthetic observation rows none of whose ReLU inputs, in either net of this weight set, lies within
    ``POOL_MARGIN`` of 0 -- a float32 evaluation, whose pre-activations are within about 3e-6 of the twin's, then takes every
    ReLU the way the twin does.  (The base sees the observation alone, so this is a property of the row, whatever the state.)"""
    rows = np.unique(rows_of(plain.synthetic_observations(200, 5)), axis=0)
    module = twin.module_from(params_of(layer_N, weights), layer_N)
    x = torch.from_numpy(rows).double()
    with torch.no_grad():
        pre = twin.net_forward(module.actor, x, lambda y: y)[1] + twin.net_forward(module.critic, x, lambda y: y)[1]
    pre = np.abs(np.concatenate([z.numpy() for z in pre], axis=1))
    keep = np.where(pre == 0, np.inf, pre).min(axis=1) > POOL_MARGIN
    assert keep.sum() >= 100
    return rows[keep]


@functools.lru_cache(maxsize=None)
def common_pool():
    """the rows that are in ``obs_pool`` of every (layer_N, weight set): the acts' observations, whatever the policy"""
    pools = [set(map(tuple, obs_pool(l, w))) for l in LAYER_NS for w in WEIGHTS]
    rows = np.array(sorted(set.intersection(*pools)), np.int32)
    assert len(rows) >= 100
    return rows


def seed_of(case):
    layer_N, weights, width, length, variant = case
    derived = 100003 * layer_N + 1009 * WEIGHTS.index(weights) + 7 * width + 131 * length + 13 * sorted(twin.VARIANTS).index(variant)
    return SEEDS.get(case, derived)


def make_batch(params, layer_N, pool, length, seed, delta, valuenorm, planted=()):
    """A record of T = 2 L rows of N worlds as a ``twin.Batch``: observations drawn from ``pool``, dones set in a quarter of the cells, h0
    N(0, 0.5), uniform actions, old log-prob = current + U(-0.4, 0.4), old value = current + U(-0.5, 0.5), targets = old value +
    N(0, 1.5 delta), advantages N(0, 1); with ValueNorm the returns are the targets denormalised by STATE0's mean and standard
    deviation.  "current" is the twin's evaluation of every chunk from its h0 under the dones.  The chunks ``planted`` have dones
    set at their first, their middle and their last step."""
    rng = np.random.default_rng(seed)
    t = 2 * length
    obs = pool[rng.integers(0, len(pool), size=(t, N, P))]  # (T, N, P, 7)
    dones = (rng.random((t, N, P)) < 0.25).astype(np.float32)
    for c in planted:
        j, rest = divmod(c, N * P)
        for i in (0, length // 2, length - 1):
            dones[j * length + i, rest // P, rest % P] = 1.0
    h0 = [(0.5 * rng.normal(size=(2, N, P, twin.HIDDEN))).astype(np.float32) for _ in range(2)]
    zeros = np.zeros((t, N, P), np.float32)
    bare = twin.Batch(obs, zeros.astype(np.int32), zeros, zeros, zeros, zeros, dones, h0[0], h0[1], length)
    with torch.no_grad():
        values, logits, _, _, (steps, n, p), _ = twin.evaluate(twin.module_from(params, layer_N), bare, np.arange(2 * N * P))
        logp = torch.log_softmax(logits, dim=-1).numpy()
    actions = rng.integers(0, twin.A, size=(t, N, P)).astype(np.int32)
    now_logp, now_v = np.zeros((t, N, P)), np.zeros((t, N, P))
    cols = np.broadcast_to(n[None, :], steps.shape), np.broadcast_to(p[None, :], steps.shape)
    now_v[steps, cols[0], cols[1]] = values.numpy()
    now_logp[steps, cols[0], cols[1]] = np.take_along_axis(logp, actions[steps, cols[0], cols[1]][..., None].astype(np.int64), axis=-1)[..., 0]
    logprobs = (now_logp + rng.uniform(-0.4, 0.4, size=(t, N, P))).astype(np.float32)
    old_values = (now_v + rng.uniform(-0.5, 0.5, size=(t, N, P))).astype(np.float32)
    returns = old_values + rng.normal(scale=1.5 * delta, size=(t, N, P))
    returns = ((twin.mappo_twin.RETURN_MEAN + twin.mappo_twin.RETURN_STD * returns) if valuenorm else returns).astype(np.float32)
    advantages = rng.normal(size=(t, N, P)).astype(np.float32)
    return twin.Batch(obs, actions, logprobs, old_values, returns, advantages, dones, h0[0], h0[1], length)


def masked_steps(batch, chunk_ids):
    """(L, Bc) bool: where the chunks' masks are zero"""
    j, n, p = twin.chunk_samples(batch, chunk_ids)
    steps = j[None, :] * batch.chunk_length + np.arange(batch.chunk_length)[:, None]
    return np.asarray(batch.dones)[steps, n[None, :], p[None, :]] != 0


@functools.lru_cache(maxsize=None)
def fixed_case(case, rows=1):
    """Parameters, batch and rows of chunk ids of a case, and for row 0 the twin and the float32 computation.  The first chunk of
    every row has its mask zero at the first step, the middle step and the last step (one and the same step where L = 1)."""
    layer_N, weights, width, length, variant = case
    cfg = twin.VARIANTS[variant]
    params, seed = params_of(layer_N, weights), seed_of(case)
    rng = np.random.default_rng(seed + 1)
    indices = np.stack([rng.permutation(2 * N * P)[:width] for _ in range(rows)]).astype(np.int32)
    batch = make_batch(params, layer_N, obs_pool(layer_N, weights), length, seed, cfg.huber_delta, cfg.valuenorm, tuple(int(ids[0]) for ids in indices))
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
