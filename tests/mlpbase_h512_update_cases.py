"""The cases of the hidden-512 MLPBase update's tests (tests/test_mlpbase_h512_update_api.py, tests/test_gpu_mlpbase_h512_update.py).
The reference is tests/mlpbase_twin.py's own ``row`` and ``step_both`` pointed at the 512 module: inside ``width_512()`` the twin
builds ``MlpBaseActorCritic(hidden=512)`` and knows that width's offsets.  Weights are tests/mlpbase_h512_cases.py's, batches
tests/balance_mappo_cases.py's synthetic records.  Nothing here touches a GPU."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import balance_mappo_cases as beam
import mlpbase_h512_cases as h512
import mlpbase_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import MlpBaseActorCritic

SLAB, SHARES = _lib.MLPBASE_H512_SLAB, _lib.H512_SHARES
# (layer_N, B, weights): one row, a ragged tile, two tiles and a ragged one; the dead first layer with the constant observation row
PARITY = [(l, b, "trained") for l in (1, 2) for b in (1, 33, 65)] + [(2, 33, "dead")]
CROSSING = [(2, SLAB + 33, "trained")]  # a slab, a tile and a sample more: 65 + 2 tiles over eight shares, two rows
DEAD = 14 + 512 * 7 + 512  # a net's leading floats behind a dead fc1: feature_norm, fc1's weight and bias
# seed of a case where the derived one fails the input conditions tests/test_mlpbase_h512_update_api.py asserts
SEEDS = {}


def seed_of(case):
    layer_N, width, weights = case
    return SEEDS.get(case, 7001 * layer_N + 11 * width + 131 * h512.WEIGHTS.index(weights) + 5)


def actor_size(layer_N):
    return h512.SIZES[layer_N][0]


def fc_h_slices(layer_N):
    na = actor_size(layer_N)
    return slice(h512.FC_H_AT, h512.FC_H_AT + h512.FC_H), slice(na + h512.FC_H_AT, na + h512.FC_H_AT + h512.FC_H)


@contextlib.contextmanager
def width_512():
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(twin, "MlpBaseActorCritic", functools.partial(MlpBaseActorCritic, hidden=h512.HIDDEN))
        patch.setattr(twin, "HIDDEN", h512.HIDDEN)
        patch.setattr(twin, "actor_size", actor_size)
        patch.setattr(twin, "fc_h_slices", fc_h_slices)
        yield


@functools.lru_cache(maxsize=None)
def fixed(layer_N, width, weights="trained", rows=1):
    """``balance_mappo_cases.fixed_case`` at width 512 on the synthetic record: parameters, batch, index rows (every row names the
    constant observation row), the twin's row 0 and the float32 one"""
    case = (layer_N, width, weights)
    cfg, seed = twin.VARIANTS["default"], seed_of(case)
    params = twin.flat(h512.make_module(layer_N, weights)).astype(np.float32)
    with width_512():
        batch = beam.make_batch(params, layer_N, beam.record_obs("synthetic", 1000 + seed % 97), seed, cfg.huber_delta, cfg.valuenorm)
        indices = twin.make_indices(rows, width, len(batch.obs), seed)
        for row in indices:
            if beam.CONSTANT_ROW not in row:
                row[0] = beam.CONSTANT_ROW
        return {"layer_N": layer_N, "params": params, "batch": batch, "indices": indices, "cfg": cfg,
                "twin": twin.row(params, layer_N, batch, indices[0], cfg, twin.STATE0),
                "f32": twin.row(params, layer_N, batch, indices[0], cfg, twin.STATE0, dtype=torch.float32)}


@functools.lru_cache(maxsize=None)
def stat_margins(cases):
    """d of every scalar stat, pooled over ``cases`` (``mappo_twin.stat_margins`` says why)"""
    d = {name: 0.0 for name in twin.STATS}
    for case in cases:
        own = twin.row_margins(fixed(*case)["twin"], fixed(*case)["f32"])
        d = {name: max(d[name], own[name]) for name in twin.STATS}
    return d


def step_both(*args):
    with width_512():
        return twin.step_both(*args)


def workspace_bytes(layer_N, minibatch_size, num_minibatches):
    """mlpbase_h512_update.hpp's formula, restated"""
    pad = lambda n: (n + 3) & ~3  # noqa: E731
    rows, layers = min(SLAB, (minibatch_size + 63) & ~63), 1 + layer_N
    stride = pad(actor_size(layer_N))
    blocks = (stride + 255) // 256
    narrow = 2 * rows * (8 + 8 + 2 + 8) + 2 * 2 * rows * 8                       # in0, y0, stat0, d_in0; out, d_out
    wide = 3 * 2 * layers * rows * 512 + 2 * layers * rows * 2                   # z, y, d_pre; stat
    floats = (2 * pad(2 * num_minibatches) + narrow + wide + 2 * layers * (rows // 32) * 1024 + 2 * SHARES * stride + 2 * 2 * stride +
              pad(2 * blocks) + 2 * (rows // 32) * 8 * 2 + 2 * 8 * 2)
    return 4 * floats
