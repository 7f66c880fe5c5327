"""The kitchens and team sizes of tests/test_kitchen_shapes_api.py and tests/test_gpu_kitchen_shapes.py: a table of shapes MAPPO's
CNN kernels take at run time (W, H, P; every one is Overcooked, F = 5P + 16) but no named layout of the other CNN tests has, the
terrain of each, and the cases built on them.  Every numeric function is ``cnn_twin``'s or ``mappo_twin``'s; those are
shape-agnostic apart from ``cnn_twin.shape``, which ``shapes()`` substitutes for its own duration with one that knows this table
and hands every other key on (as tests/simplecooked_cnn_cases.py does).  Nothing here touches a GPU.

A key ``kWxHpP`` is a custom kitchen in the reference's Config format, built deterministically: COUNTER border, AIR interior, one
POT, ONION, DISH and SERVING cell on the border beside the interior, the players on the first P interior cells in row-major
order, the base recipe tables.  The other keys are layouts of ``layouts.LAYOUTS``; ``name/1p`` keeps its first player only.

The LDS byte counts are literals: ``lds_bytes`` restates cnn_lds (cnn_policy.hpp) and cnn_update_lds (cnn_update.hpp), and
tests/test_kitchen_shapes_api.py holds the literals against it and against what the library accepts and refuses."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import cnn_twin
import mappo_twin
from madrona_rl_envs_playground_amd import layouts

HORIZON, STEPPED = cnn_twin.HORIZON, cnn_twin.STEPPED
N = 33  # worlds of every case: two 32-row tiles at P = 1, more at higher P, always a ragged last tile
LDS_LIMIT = 160 * 1024

# key: (W, H, P, the act's LDS image, the update's), and what the key is first to run
ACCEPTED = {
    "k3x3p1": (3, 3, 1, 38528, 56448),      # npos 1: three waves without a position; fc1's K = 32 is half a chunk; region A of the update
                                            # larger than the act's; rows of 189 bytes
    "k4x3p2": (4, 3, 2, 48992, 60544),      # npos 2, H = 3
    "k3x5p1": (3, 5, 1, 47616, 64640),      # npos 3, W = 3, W < H
    "k4x4p3": (4, 4, 3, 69040, 69296),      # npos 4 (one per wave); P = 3, F = 31: k1 = 279 odd, 9 slabs, last slab 23 wide
    "k6x5p4": (6, 5, 4, 126224, 126480),    # npos 12 (exactly one round); P = 4, F = 36: 11 slabs, db_conv on wave 3, last slab 4 wide
    "k15x3p2": (15, 3, 2, 121696, 121952),  # npos 13: a second round for wave 0 only; the widest row of positions
    "k3x9p2": (3, 9, 2, 82016, 82272),      # npos 7, tall and narrow
    "k7x3p3": (7, 3, 3, 78256, 78512),      # rows of 651 bytes (S % 4 = 3) at P = 3: all four row shifts within one tile
    "forced_coordination": (5, 5, 2, 88672, 89216),   # a standard layout; region A of the update larger than the act's
    "counter_circuit": (8, 5, 2, 137824, 138080),     # a standard layout
    "k8x5p4": (8, 5, 4, 162320, 162576),    # the largest image this table can reach
    "multiplayer_schelling/1p": (7, 7, 1, 160512, 160768),  # npos 25
}
REFUSED = {
    "k10x5p2": (10, 5, 2, 170848, 171104),
    "k9x5p3": (9, 5, 3, 167600, 167856),    # asymmetric_advantages' size with a third player
    "multiplayer_schelling": (7, 7, 4, 201488, 201744),  # as shipped
}
TABLE = {**ACCEPTED, **REFUSED}
KEYS, REFUSED_KEYS = tuple(ACCEPTED), tuple(REFUSED)
# the shapes the CNN kernels had run on before this table: (W, H, P, F) of the Overcooked and Simplecooked cases
OLD_SHAPES = ((5, 4, 2, 26), (9, 5, 2, 26), (5, 5, 2, 26), (5, 4, 2, 20), (9, 5, 2, 20), (5, 5, 2, 20), (5, 4, 1, 15), (5, 5, 1, 15))

# the update moves act_at up at these keys (region A of the act is below what back-propagation keeps there)
REGION_A_GROWS = ("k3x3p1", "k4x3p2", "k3x5p1", "forced_coordination")

_TERRAIN = {"AIR": " ", "POT": "P", "COUNTER": "X", "ONION": "O", "DISH": "D", "SERVING": "S"}
_others_shape = cnn_twin.shape


def lds_bytes(w, h, f):
    """(the act's LDS image, the update's, region A of the act, region A of the update) in bytes"""
    row = (w * h * f + 6) & ~3
    if (row // 4) % 2 == 0:
        row += 4
    k1_padded = (9 * f + 1) & ~1
    conv_ld = k1_padded | 1
    act_ld = 32 * (w - 2) * (h - 2) + 1
    koff_at = 32 * row + 32 * conv_ld * 4
    fc_bytes = 64 * 65 * 4 + 2 * 32 * 65 * 4 + 32 * 8 * 4
    update_fc_bytes = fc_bytes + 32 * 8 * 4 + 2 * 32 * 65 * 4
    region_a = max((koff_at + k1_padded * 2 + 15) & ~15, fc_bytes)
    region_a_update = max(region_a, update_fc_bytes)
    return region_a + 32 * act_ld * 4, region_a_update + 32 * act_ld * 4 + 32 * 2 * 4, region_a, region_a_update


def classes(w, h, f):
    """the shape-dependent classes of the kernels: {"npos", "slabs" (32-wide slabs of the conv gradient's k1 = 9F), "last_slab"}"""
    k1 = 9 * f
    slabs = -(-k1 // 32)
    return {"npos": (w - 2) * (h - 2), "slabs": slabs, "last_slab": k1 - 32 * (slabs - 1)}


def custom_grid(w, h, p):
    """the rows of a custom kitchen, in the glyphs of ``layouts``"""
    cells = [[_TERRAIN["COUNTER"]] * w for _ in range(h)]
    for y in range(1, h - 1):
        for x in range(1, w - 1):
            cells[y][x] = _TERRAIN["AIR"]
    cells[0][1], cells[1][0], cells[h - 2][w - 1], cells[h - 1][w - 2] = (_TERRAIN[k] for k in ("POT", "ONION", "DISH", "SERVING"))
    interior = [(x, y) for y in range(1, h - 1) for x in range(1, w - 1)]
    assert p <= len(interior)
    for seat, (x, y) in enumerate(interior[:p]):
        cells[y][x] = layouts.PLAYER_GLYPHS[seat]
    return ["".join(row) for row in cells]


def layout_params(key, horizon=HORIZON):
    """the simulator's and the oracle's parameters of a key of the table"""
    w, h, p, _, _ = TABLE[key]
    name, _, tail = key.partition("/")
    if name in layouts.LAYOUTS:
        params = layouts.get_base_layout_params(name, horizon, max_num_players=int(tail[:-1]) if tail else None)
    else:
        source = {"grid": "\n".join(custom_grid(w, h, p)), "start_all_orders": [{"ingredients": ["onion", "onion", "onion"]}],
                  "rew_shaping_params": None}
        params = layouts.get_base_layout_params(source, horizon)
    assert (params["width"], params["height"], params["num_players"]) == (w, h, p), key
    return params


def shape(key):
    """(W, H, P, F) of a key of the table; any other key: ``cnn_twin``'s own answer"""
    if key not in TABLE:
        return _others_shape(key)
    w, h, p, _, _ = TABLE[key]
    return w, h, p, 5 * p + 16


@contextlib.contextmanager
def shapes():
    """``cnn_twin.shape`` knows the table's keys inside this block (and is put back after it)"""
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(cnn_twin, "shape", shape)
        yield


# ---------------------------------------------------------------- the act's cases

STEPPED_KEYS = ("forced_coordination", "counter_circuit", "k4x4p3")
# (key, worlds, weights, inputs)
CASES = [(key, N, "trained", "synthetic") for key in KEYS] + [(key, N, "trained", "stepped") for key in STEPPED_KEYS]

# seed of a forward case where the derived one puts more than 1 % of the draws within 1e-5 of a boundary (a condition that
# tests/test_kitchen_shapes_api.py asserts): replaced here, not excused there.  None of the derived seeds does.
CASE_SEEDS = {}


def case_seed(key, n, weights, inputs):
    """seed of the inputs and of the draws of one case"""
    if (key, n, weights, inputs) in CASE_SEEDS:
        return CASE_SEEDS[(key, n, weights, inputs)]
    return 7919 * n + 104729 * cnn_twin.WEIGHTS.index(weights) + 1299709 * cnn_twin.INPUTS.index(inputs) + 37 * KEYS.index(key) + 17


def make_module(key, weights):
    with shapes():
        return cnn_twin.make_module(key, weights)


def stepped_observations(key, n, seed, steps=STEPPED, horizon=HORIZON):
    """``cnn_twin.stepped_observations`` on a key of the table: (N, P, H, W, F) int8 and the actions (steps, P, N) int32"""
    from oracle import oracle
    oracle.build()
    w, h, p, f = shape(key)
    orc = oracle.OvercookedOracle(layout_params(key, horizon), n)
    rng = np.random.default_rng(seed)
    actions = rng.integers(0, 6, size=(steps, p, n)).astype(np.int32)
    for t in range(steps):
        orc.step(actions[t])
    obs = orc.obs.reshape(n, p, h, w, f).astype(np.int8).copy()
    orc.close()
    return obs, actions


def synthetic_observations(key, n, seed):
    with shapes():
        return cnn_twin.synthetic_observations(key, n, seed)


@functools.lru_cache(maxsize=None)
def case_inputs(key, n, weights, inputs):
    """{"obs": (N, P, H, W, F) int8, "actions": the oracle's action stream or None} -- shared, never modified"""
    seed = case_seed(key, n, weights, inputs)
    if inputs == "stepped":
        obs, actions = stepped_observations(key, n, seed)
    else:
        obs, actions = synthetic_observations(key, n, seed), None
    obs.setflags(write=False)
    return {"obs": obs, "actions": actions}


@functools.lru_cache(maxsize=None)
def case_margins(key, n, weights, inputs):
    return cnn_twin.margins(make_module(key, weights), cnn_twin.rows_of(case_inputs(key, n, weights, inputs)["obs"]))


@functools.lru_cache(maxsize=None)
def layout_margins(key, weights):
    """d of a key at one weight set: the largest over the key's cases (as ``cnn_twin.layout_margins``)"""
    per_case = [case_margins(*case) for case in CASES if case[0] == key and case[2] == weights]
    return max(m[0] for m in per_case), max(m[1] for m in per_case)


def integer_case(key):
    """(layers, observations (N, P, H, W, F)) of the exact-integer construction at a key's shape"""
    with shapes():
        return cnn_twin.integer_layers(key), cnn_twin.integer_observations(key)


# ---------------------------------------------------------------- the update's cases

T = mappo_twin.T
B = 33  # one full tile and a tile of one sample
# (key, worlds, weights, inputs, B, variant): the ring of a case is (T, worlds, P) samples
MAPPO_CASES = [(key, N, "trained", "synthetic", B, "default") for key in KEYS]
# seed of a case's batch and index row where the derived one fails the input conditions of tests/test_kitchen_shapes_api.py (a
# sample within KINK of a kink, or a pre-activation too close to 0): replaced here, not excused there
SEEDS = {
    ('k6x5p4', 33, 'trained', 'synthetic', 33, 'default'): 1766164,
    ('counter_circuit', 33, 'trained', 'synthetic', 33, 'default'): 1866352,
    ('multiplayer_schelling/1p', 33, 'trained', 'synthetic', 33, 'default'): 1766423,
}


def seed_of(case):
    key, worlds, weights, inputs, width, variant = case
    derived = case_seed(key, worlds, weights, inputs) + 7 * width + 13 * sorted(mappo_twin.VARIANTS).index(variant)
    return SEEDS.get(case, derived)


@functools.lru_cache(maxsize=None)
def ring_of(key, worlds, inputs, seed):
    """``mappo_twin.ring_of`` on a key of the table: (T * worlds * P, H, W, F) int8 in sample order (t, n, p)"""
    assert inputs == "synthetic"
    ring = np.ascontiguousarray(np.concatenate([cnn_twin.rows_of(synthetic_observations(key, worlds, seed + t)) for t in range(T)]))
    ring.setflags(write=False)
    return ring


@functools.lru_cache(maxsize=None)
def params_of(key, weights):
    return cnn_twin.flat(make_module(key, weights)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def fixed_case(case):
    """``mappo_twin.fixed_case`` for a case of ``MAPPO_CASES``: parameters, batch and one index row, the twin and the float32
    computation of that row"""
    key, worlds, weights, inputs, width, variant = case
    cfg = mappo_twin.VARIANTS[variant]
    params, seed = params_of(key, weights), seed_of(case)
    batch = mappo_twin.make_batch(params, ring_of(key, worlds, inputs, 1000 + seed % 97), seed, cfg.huber_delta, cfg.valuenorm)
    size = len(batch.ring)
    assert width <= size
    indices = mappo_twin.make_indices(1, width, size, seed)
    with shapes():
        return {"layout": key, "worlds": worlds, "params": params, "batch": batch, "indices": indices, "cfg": cfg,
                "twin": mappo_twin.row(params, key, batch, indices[0], cfg, mappo_twin.STATE0),
                "f32": mappo_twin.row(params, key, batch, indices[0], cfg, mappo_twin.STATE0, dtype=torch.float32)}


@functools.lru_cache(maxsize=None)
def stat_margins(weights="trained"):
    """d of every scalar stat, pooled over the cases here (``mappo_twin.stat_margins`` and DESIGN.md section 13 say why one row's
    own distance bounds nothing)"""
    d = {name: 0.0 for name in mappo_twin.STATS}
    for case in MAPPO_CASES:
        if case[2] != weights:
            continue
        fixed = fixed_case(case)
        own = mappo_twin.row_margins(fixed["twin"], fixed["f32"])
        for name in mappo_twin.STATS:
            d[name] = max(d[name], own[name])
    return d


@functools.lru_cache(maxsize=None)
def update_integer_case(key):
    """``mappo_twin.integer_case`` at B = 64 on a key of the table"""
    with shapes():
        return mappo_twin.integer_case(key)
