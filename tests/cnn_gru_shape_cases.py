"""The recurrent CNN kernels on the kitchen shape table: the cases of tests/test_cnn_gru_shapes_api.py and
tests/test_gpu_cnn_gru_shapes.py.  Shapes, parameters and inputs are tests/cnn_gru_twin.py's on the table's keys.  Nothing here
touches a GPU.

Both LDS images are maxima of two layouts (cnn_gru.hpp).  The act's is max(the plain act's image, 109 568): the GRU image overlays
the convolution's dead operands from a fixed offset.  The update's is max(the plain update's image without its 256-byte tail,
135 680) + 256: below the crossover the chunk ids and row shifts lie behind the recurrent phase, above it behind the activation
image.  The byte counts are literals; tests/test_cnn_gru_shapes_api.py holds them against ``kitchen_shape_cases``' table."""
import functools

import torch

import cnn_gru_twin as twin

N = BC = 33
GRU_ACT_BYTES, GRU_UPDATE_BYTES, TAIL = 109568, 135680, 256
# key: (the recurrent act's LDS image, the recurrent update's)
LDS = {
    "forced_coordination": (109568, 135936),       # the act's image nearest below its crossover (88 672 of the plain act)
    "k15x3p2": (121696, 135936),                   # ... and nearest above
    "k4x4p3": (109568, 135936),
    "k6x5p4": (126224, 135936),                    # the update's image nearest below its crossover (126 224 without the tail)
    "counter_circuit": (137824, 138080),           # ... and nearest above (137 824)
    "multiplayer_schelling/1p": (160512, 160768),
}
# (key, seats) at 33 worlds and nonzero states, and what each is first to run
ACT_CASES = [
    ("forced_coordination", (0, 1)),          # the image just below the act's crossover
    ("k15x3p2", (0, 1)),                      # ... just above it
    ("k4x4p3", (0, 2)),                       # P = 3, two seats with a gap
    ("k6x5p4", (0, 1, 2, 3)),                 # npos 12, P = 4
    ("multiplayer_schelling/1p", (0,)),       # npos 25
]
# (key, L, Bc)
UPDATE_CASES = [
    ("k6x5p4", 2, BC),                        # just below the update's crossover; npos 12, last slab 4 wide
    ("counter_circuit", 2, BC),               # just above it
    ("counter_circuit", 16, BC),              # a long chunk on the conv-bound side
    ("k4x4p3", 2, BC),                        # P = 3, last slab 23 wide
    ("k15x3p2", 2, BC),                       # npos 13
    ("multiplayer_schelling/1p", 2, BC),      # npos 25
]
# (key, chunk): the update's forward sweep against the act's bits on both sides of the update's crossover
UNCHANGED_CASES = [("k6x5p4", 2), ("counter_circuit", 2)]
# A stat's float32 distance from the twin on ONE row bounds nothing (it can cancel to almost 0), so every kitchen pools d over its
# rows above and over these chunk lengths on the CPU alone: same kitchen, same parameters, same Bc
POOL_CHUNKS = (1, 10)


@functools.lru_cache(maxsize=None)
def twin_rows(case):
    """(the float64 twin's row, the float32 CPU row) of one update case"""
    params, batch, ids = twin.update_case(*case)
    cfg = twin.Config()
    return twin.row(params, case[0], batch, ids[0], cfg), twin.row(params, case[0], batch, ids[0], cfg, dtype=torch.float32)


def pool(key):
    return [case for case in UPDATE_CASES if case[0] == key] + [(key, L, BC) for L in POOL_CHUNKS]


@functools.lru_cache(maxsize=None)
def stat_margins(key):
    """d of every scalar stat, pooled over the kitchen's rows"""
    rows = [twin_rows(case) for case in pool(key)]
    return {name: max(abs(single["stats"][name] - exact["stats"][name]) for exact, single in rows) for name in twin.STATS}
