"""CPU oracle (oracle/overcooked_oracle.c) against the reference's own Overcooked sim.cpp, compiled unchanged against the
Madrona stand-in (oracle/_ref/libref_overcooked.so, see oracle/ref.py).  Bit-exact after every step: every viewer's
observation rows, the reward and the done flag; every 10 steps and at the end the players, the objects on all cells and the
timestep as well.  The reference's guard bytes stay untouched throughout.

Every case asserts on the REFERENCE's own outputs and state that it was not vacuous: an episode ended, a pot was used, and --
where a goal-directed "cook" stream drives the worlds -- a soup was delivered.  The type-limit cases sit where the narrow
types of sim.hpp show (int8_t cooking_tick, uint8_t recipe tables and shaping rewards) and assert that the limit was reached.
"""
import zlib

import numpy as np
import pytest

import kitchen_ref as kr
from oracle import ref

GAME = "overcooked"


@pytest.fixture(scope="module", autouse=True)
def _ref_built():
    ref.require()


def _random(params, n, steps, p_interact, seed, layout=None):
    rng = np.random.default_rng(seed)
    return (lambda t, r: kr.layout_actions(rng, layout, params["num_players"], n, p_interact, t)), steps


def _seed(*key):
    return zlib.crc32("-".join(str(k) for k in key).encode())


@pytest.mark.parametrize("layout,horizon,cap,n,steps,p_interact", [
    ("cramped_room", 37, None, 300, 200, 0.35),
    ("asymmetric_advantages", 60, None, 150, 200, 0.45),
    ("coordination_ring", 50, None, 150, 200, 0.4),
    ("forced_coordination", 50, None, 150, 200, 0.5),
    ("counter_circuit", 50, None, 150, 200, 0.6),
    ("multiplayer_schelling", 45, None, 100, 150, 0.35),
    ("multiplayer_schelling", 40, 3, 100, 150, 0.4),
    ("asymmetric_advantages_tomato", 80, None, 150, 250, 0.45),
    ("many_player_layout", 30, 2, 100, 150, 0.35),
    ("many_player_layout", 20, 5, 60, 150, 0.4),
    ("many_player_layout", 30, 8, 50, 150, 0.35),
    ("many_player_layout", 25, 40, 50, 150, 0.35),
    ("cramped_room", 30, 1, 200, 200, 0.4),
])
def test_layouts(layout, horizon, cap, n, steps, p_interact):
    params = kr.layout_params(GAME, layout, horizon, cap)
    cov = kr.lockstep(GAME, params, n, _random(params, n, steps, p_interact, _seed(layout, cap, n), layout), tag=layout)
    print(f"{layout} cap {cap}: {n} worlds x {steps} steps, {cov}")
    assert cov.episodes >= 1 and cov.pot_steps >= 1, cov


@pytest.mark.parametrize("seed", range(24))
def test_random_kitchens(seed):
    """The 24 kitchens of tests/test_gpu_overcooked.py:test_random_layouts_against_oracle (1..6 players, up to 6 pots, drawn
    recipe tables).  Random play, except that in every second world player 0 runs errands to a pot (kitchen_ref.Fetcher): a
    pot must have been used wherever player 0 can walk to a source and to a pot."""
    from test_gpu_overcooked import _random_layout
    params = _random_layout(np.random.default_rng(1000 + seed))
    n, steps, P = 60, 150, params["num_players"]
    rng = np.random.default_rng(3000 + seed)
    fetcher = kr.Fetcher(GAME, params)

    def actions(t, r):
        acts = kr.random_actions(rng, P, n, 0.4)
        fetcher.steer(r.players, acts)
        return acts

    cov = kr.lockstep(GAME, params, n, (actions, steps), tag=f"kitchen {seed}")
    print(f"kitchen {seed} ({params['height']}x{params['width']}, {P} players, horizon {params['horizon']}): {cov}")
    assert cov.episodes >= 1, cov
    if fetcher.can_cook(params["start_player_y"][0] * params["width"] + params["start_player_x"][0]):
        assert cov.pot_steps >= 1, cov


@pytest.mark.parametrize("fixture", ["cramped_room_cook", "coordination_ring_cook", "tomato_mix_cook", "multiplayer_schelling_cook"])
def test_cook_streams(fixture):
    """The goal-directed streams of tests/golden/make_overcooked_golden.py: whole soup cycles, on the layouts where random
    play earns next to nothing."""
    params, stream = kr.cook_stream(GAME, fixture)
    n = 50
    cov = kr.lockstep(GAME, params, n, kr.cook_actions(stream, n, _seed(fixture)), tag=fixture)
    print(f"{fixture}: {n} worlds x {len(stream)} steps, {cov}")
    assert cov.episodes >= 1 and cov.pot_steps >= 1 and cov.deliveries >= 1, cov


LIMITS = [("time", 0), ("time", 127), ("time", 128), ("time", 255), ("value", 255), ("value", 300),
          ("rewards", 200), ("rewards", 242), ("rewards", 257), ("rewards", 287),
          ("horizon", 0), ("horizon", 1), ("horizon", 39), ("horizon", 40), ("horizon", 41)]


@pytest.mark.parametrize("kind,value", LIMITS)
def test_type_limits(kind, value):
    """`cramped_room` where sim.hpp's narrow types show.  From a recipe time of 128 on the int8_t tick wraps at 127 and no
    soup is ever ready; recipe values and shaping rewards are paid & 255; the horizon cases sit around the 40 steps of the
    "about to end" flag (sim.cpp:79) and at the degenerate 0 and 1."""
    params = kr.limit_params(GAME, kind, value)
    n, steps = 150, 600 if kind == "time" else 200
    stream = kr.cook_stream(GAME, "cramped_room_cook")[1]
    rng = np.random.default_rng(_seed(kind, value))
    cook = kr.cook_actions(stream[:steps], 50, _seed(kind, value))

    def actions(t, r):  # a third of the worlds cook (the soups that reach the limits), the others play at random
        a = kr.random_actions(rng, 2, n, 0.45)
        if t < len(cook):
            a[:, :50] = cook[t]
        return a

    cov = kr.lockstep(GAME, params, n, (actions, steps), tag=f"{kind} {value}")
    print(f"{kind} {value}: {cov}")
    kr.assert_limit_covered(kind, value, params, cov)


@pytest.mark.parametrize("layout,horizon,cap,n,steps", [("cramped_room", 37, None, 100, 150), ("multiplayer_schelling", 40, None, 60, 120),
                                                         ("asymmetric_advantages_tomato", 60, None, 60, 150),
                                                         ("many_player_layout", 25, 8, 20, 80), ("cramped_room", 30, 1, 60, 100)])
def test_independent_of_what_madrona_leaves_open(layout, horizon, cap, n, steps):
    """Fresh component memory 0x00 or 0xA5, default member initialisers run or not, two topological orders of the task graph,
    entities visited in ascending or descending order: the same bytes all four ways, and no guard byte written."""
    params = kr.layout_params(GAME, layout, horizon, cap)
    cov = kr.lockstep(GAME, params, n, _random(params, n, steps, 0.5, _seed("open", layout), layout), variants=kr.FOUR_WAYS, tag=layout)
    assert cov.episodes >= 1 and cov.pot_steps >= 1, cov


def test_second_graph_order_is_the_documented_one():
    """setupTasks (sim.cpp:498-537) adds 19 nodes: 0-6 the interact chain, 7-9 move / collision / unset, 10 handle collisions
    (after 9 and 6), 11 pots (after 6), 12 check_reset_system (no dependency), 13-16 the reset systems, 17 observations, 18 post.
    Order 1 takes, of the nodes that are ready, the one added last: check_reset_system first, the move chain before the
    interact chain."""
    r = ref.RefOvercooked(kr.layout_params(GAME, "cramped_room", 30), 1, graph_order=1)
    assert r.node_order(0) == list(range(19))
    assert r.node_order(1) == [12, 7, 8, 9, 0, 1, 2, 3, 4, 5, 6, 11, 14, 10, 15, 16, 13, 17, 18]
    r.close()


def test_refuses_what_the_cpp_cannot_hold():
    """256 cells: WorldState.size (uint8_t) would be 0 and the observation system divide by it.  65 players: MAX_NUM_PLAYERS."""
    big = kr.layout_params(GAME, "cramped_room", 30)
    big.update(height=16, width=16, terrain=[2] * 256)
    with pytest.raises(ValueError):
        ref.RefOvercooked(big, 2)
    many = kr.layout_params(GAME, "cramped_room", 30)
    many.update(num_players=65, start_player_x=[1] * 65, start_player_y=[1] * 65)
    with pytest.raises(ValueError):
        ref.RefOvercooked(many, 2)
    ref.RefOvercooked(kr.layout_params(GAME, "many_player_layout", 30, 2), 1).close()  # 255 cells are held
