"""The hidden-512 CNN act on the kitchen shape table: the cases of tests/test_cnn_h512_shapes_api.py and
tests/test_gpu_cnn_h512_shapes.py.  tests/kitchen_shape_cases.py gives the kitchens (its TABLE, ``layout_params``, ``shape``,
``synthetic_observations``), tests/cnn_h512_cases.py the module at a (W, H, F), ``evaluate`` and the exact-integer construction;
the three kitchens of the tile-edge and rollout cases that the table does not hold (cramped_room, simple/1p) are
``cnn_h512_cases.KITCHENS``' own.  Nothing here touches a GPU.

The LDS byte counts are literals: ``cnn_h512_lds(W, H, F).total`` is the larger of the table's act image (the channel loop runs on
exactly that) and what lies behind fc1, 32 rows of 513 floats and 32 x 8 outputs; tests/test_cnn_h512_shapes_api.py holds them
against ``kitchen_shape_cases.lds_bytes``."""
import functools

import numpy as np
import torch

import cnn_h512_cases as h512
import cnn_twin as twin
import kitchen_shape_cases as table

HIDDEN, CHANNELS, HORIZON = h512.HIDDEN, h512.CHANNELS, h512.HORIZON
N = table.N
LDS_LIMIT = table.LDS_LIMIT
BEHIND_FC1 = 32 * 513 * 4 + 32 * 8 * 4  # 66 688
# key: the 512 act's LDS image.  The three smallest kitchens run on the image behind fc1, every other one on the channel loop's
LDS = {
    "k3x3p1": 66688, "k4x3p2": 66688, "k3x5p1": 66688, "k4x4p3": 69040, "k6x5p4": 126224, "k15x3p2": 121696, "k3x9p2": 82016,
    "k7x3p3": 78256, "forced_coordination": 88672, "counter_circuit": 137824, "k8x5p4": 162320, "multiplayer_schelling/1p": 160512,
    "k10x5p2": 170848, "k9x5p3": 167600, "multiplayer_schelling": 201488,
}
KEYS, REFUSED_KEYS = table.KEYS, table.REFUSED_KEYS
OTHERS = ("cramped_room", "simple/1p")  # of cnn_h512_cases.KITCHENS, not of the table


def shape(key):
    """(W, H, P, F)"""
    return table.shape(key) if key in table.TABLE else h512.KITCHENS[key][2]


def simulator(key):
    """the simulator class's name"""
    return "OvercookedSimulator" if key in table.TABLE else h512.KITCHENS[key][0]


def layout_params(key, horizon=HORIZON):
    return table.layout_params(key, horizon) if key in table.TABLE else h512.KITCHENS[key][1](horizon)


def make_module(key, weights="trained"):
    w, h, _, f = shape(key)
    return h512.module_of(w, h, f, weights)


# (key, worlds, players mask or None).  Every admitted key at 33 worlds, all seats: npos 1, 2, 3, 4, 7, 12, 13 and 25 (fc1's
# kb = 32 npos per block, the w_row walk over 8 blocks, K2 up to 6400), F = 31 and 36 (P = 3 and 4 in seat_sample) ...
ALL_SEATS = [(key, N, None) for key in KEYS]
# ... masks with a gap over three and four seats ...
MASKED = [("k4x4p3", N, 0b101), ("k7x3p3", N, 0b010), ("k6x5p4", N, 0b1010), ("k8x5p4", N, 0b0111)]
# ... and N P a multiple of 32 (no ragged tile: one, two, three full tiles) or below 3 (the smallest calls, a single sample)
TILE_EDGES = [("cramped_room", 16, None), ("cramped_room", 32, None), ("cramped_room", 1, None), ("k3x3p1", 1, None), ("k4x4p3", 32, None)]
FORWARD = ALL_SEATS + MASKED + TILE_EDGES
INTEGER_KEYS = ("k3x3p1", "k4x4p3", "k7x3p3", "k6x5p4", "k15x3p2", "multiplayer_schelling/1p")
# (key, worlds, T, horizon): Simplecooked, and four seats; the horizon ends episodes inside the window
ROLLOUTS = [("simple/1p", N, 3, 2), ("k6x5p4", N, 3, 2)]

# seed of a forward case where the derived one fails a condition that tests/test_cnn_h512_shapes_api.py asserts: replaced here, not
# excused there.  No derived seed puts more than one draw within 1e-5 of a boundary.  The single sample of k3x3p1: one row's own
# float32 distance can fall anywhere below its kitchen's (with the derived seed 8.9e-07 on one host and 9.6e-06 on another, where
# the kitchen's 33 worlds give 1.5e-05 and 1.7e-05), and 8 d of it is then no margin at all (``small_case_unit``)
CASE_SEEDS = {("k3x3p1", 1): 122659}
# one weight of fc1 in this many is nonzero in the integer construction of a key (default: cnn_h512_cases' 64), thinned where the
# reference's own bound would pass 2^24.  At K2 = 6400 the default still holds, so no key is thinned.
FC1_ONE_IN = {}


def case_seed(key, n):
    """seed of the inputs and of the draws of one case"""
    if (key, n) in CASE_SEEDS:
        return CASE_SEEDS[(key, n)]
    return 7919 * n + 104729 + 43 * (list(KEYS) + list(OTHERS)).index(key) + 11


@functools.lru_cache(maxsize=None)
def reference(key, n, weights="trained"):
    """the float64 module on the case's synthetic observations (every seat's rows), the draws, ``near``, and d per kind"""
    seed = case_seed(key, n)
    module, obs = make_module(key, weights), table.synthetic_observations(key, n, seed)
    obs.setflags(write=False)
    values, logits, logp = h512.evaluate(module, obs, torch.float64)
    v32, l32, lp32 = h512.evaluate(module, obs, torch.float32)
    u = twin.draws(seed, 0, n, obs.shape[1])
    cdf = np.cumsum(np.exp(logp), axis=1)[:, :-1]
    return {"obs": obs, "seed": seed, "values": values, "logits": logits, "logp": logp, "u": u, "cdf": cdf,
            "actions": (u[:, None] >= cdf).sum(axis=1).astype(np.int32), "near": twin.near_boundary(cdf, u),
            "d_value": float(np.abs(v32 - values).max()), "d_logp": float(np.abs(lp32 - logp).max()),
            "d_logits": float(np.abs(l32 - logits).max())}


def integer_case(key):
    """(layers, observations (33, P, H, W, F)) of ``cnn_h512_cases``' exact-integer construction at a key's shape"""
    return h512.integer_case_of(*shape(key), fc1_one_in=FC1_ONE_IN.get(key, 64))


def small_case_unit(key, n):
    """{kind: (d of the case, d of the same kitchen's largest forward case)} for a case of fewer than 32 samples, else {}.  The
    condition on them: 8 d of the small case is at least the d of its kitchen's full case, that is, the margin admits at least
    torch float32's own error in that kitchen."""
    if n * shape(key)[2] >= 32:
        return {}
    full = reference(key, max(m for k, m, _ in FORWARD if k == key))
    return {kind: (reference(key, n)[kind], full[kind]) for kind in ("d_value", "d_logp", "d_logits")}
