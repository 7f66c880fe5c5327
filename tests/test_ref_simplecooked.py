"""CPU oracle (oracle/simplecooked_oracle.c) against the reference's own Simplecooked (overcooked2_env) sim.cpp, compiled
unchanged against the Madrona stand-in (oracle/_ref/libref_simplecooked.so, see oracle/ref.py).  Bit-exact after every step:
both viewers' observation rows, the reward and the done flag; every 10 steps and at the end the players, the objects on all
cells, the timestep and num_dishes_out as well.  The reference's guard bytes stay untouched throughout.

Two players only: with one player the C++ reads the PlayerState of an agent that was never created (is_dish_pickup_useful
loops p < 2), so the driver refuses it, and this project's one-player Simplecooked stays pinned by the numpy twin alone
(tests/test_oracle_simplecooked.py).

Every case asserts on the REFERENCE's own outputs and state that it was not vacuous; see tests/test_ref_overcooked.py.
"""
import zlib

import numpy as np
import pytest

import kitchen_ref as kr
from oracle import ref

GAME = "simplecooked"


@pytest.fixture(scope="module", autouse=True)
def _ref_built():
    ref.require()


def _random(n, steps, p_interact, seed):
    rng = np.random.default_rng(seed)
    return (lambda t, r: kr.random_actions(rng, 2, n, p_interact)), steps


def _seed(*key):
    return zlib.crc32("-".join(str(k) for k in key).encode())


@pytest.mark.parametrize("layout,horizon,n,steps,p_interact", [
    ("simple", 37, 300, 200, 0.5),
    ("unident_s", 60, 150, 200, 0.35),
    ("random0", 50, 150, 200, 0.35),
    ("random1", 50, 150, 200, 0.45),
    ("random3", 50, 150, 200, 0.6),
    ("simple_tomato", 80, 150, 250, 0.45),
])
def test_layouts(layout, horizon, n, steps, p_interact):
    params = kr.layout_params(GAME, layout, horizon)
    cov = kr.lockstep(GAME, params, n, _random(n, steps, p_interact, _seed(layout, n)), tag=layout)
    print(f"{layout}: {n} worlds x {steps} steps, {cov}")
    assert cov.episodes >= 1 and cov.pot_steps >= 1, cov


def _two_player_kitchens():
    from test_gpu_simplecooked import _random_kitchen
    kitchens = [(seed, _random_kitchen(np.random.default_rng(2000 + seed))) for seed in range(16)]
    return [(seed, k) for seed, k in kitchens if k["num_players"] == 2]


@pytest.mark.parametrize("seed,params", _two_player_kitchens(), ids=lambda v: str(v) if isinstance(v, int) else "")
def test_random_kitchens(seed, params):
    """Those of the 16 kitchens of tests/test_gpu_simplecooked.py:test_random_kitchens_against_oracle that have two players.
    Random play, except that in every second world player 0 runs errands to a pot (kitchen_ref.Fetcher): a pot must have
    been used wherever player 0 can walk to a source and to a pot."""
    n, steps = 60, 150
    rng = np.random.default_rng(4000 + seed)
    fetcher = kr.Fetcher(GAME, params)

    def actions(t, r):
        acts = kr.random_actions(rng, 2, n, 0.45)
        fetcher.steer(r.players, acts)
        return acts

    cov = kr.lockstep(GAME, params, n, (actions, steps), tag=f"kitchen {seed}")
    print(f"kitchen {seed} ({params['height']}x{params['width']}, horizon {params['horizon']}): {cov}")
    assert cov.episodes >= 1, cov
    if fetcher.can_cook(params["start_player_y"][0] * params["width"] + params["start_player_x"][0]):
        assert cov.pot_steps >= 1, cov


@pytest.mark.parametrize("fixture", ["simple_cook", "random1_cook", "unident_s_cook"])
def test_cook_streams(fixture):
    """The goal-directed streams of tests/golden/make_simplecooked_golden.py: whole soup cycles."""
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
    """`simple` where sim.hpp's narrow types show.  From a recipe time of 128 on the int8_t tick wraps at 127 and no soup is
    ever ready; recipe values and the three shaping rewards are paid & 255; horizons 0, 1 and around 40 as for Overcooked
    (this world has no "about to end" flag, the cases cost nothing)."""
    params = kr.limit_params(GAME, kind, value)
    n, steps = 150, 600 if kind == "time" else 200
    stream = kr.cook_stream(GAME, "simple_cook")[1]
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
    if kind == "rewards":
        assert (params["dish_pickup_rew"] & 255) in cov.rewards, f"dish pickup reward never paid alone ({cov})"


@pytest.mark.parametrize("layout,horizon,n,steps", [("simple", 37, 100, 150), ("simple_tomato", 60, 60, 150), ("random3", 40, 60, 120)])
def test_independent_of_what_madrona_leaves_open(layout, horizon, n, steps):
    """Fresh component memory 0x00 or 0xA5, default member initialisers run or not, two topological orders of the task graph,
    entities visited in ascending or descending order: the same bytes all four ways, and no guard byte written."""
    params = kr.layout_params(GAME, layout, horizon)
    cov = kr.lockstep(GAME, params, n, _random(n, steps, 0.5, _seed("open", layout)), variants=kr.FOUR_WAYS, tag=layout)
    assert cov.episodes >= 1 and cov.pot_steps >= 1, cov


def test_refuses_what_the_cpp_cannot_hold():
    """One player: undefined in the C++ (see the module docstring); it must be refused, not crash.  More than MAX_SIZE = 100
    cells and more than two players do not fit Config."""
    with pytest.raises(ValueError):
        ref.RefSimplecooked(kr.layout_params(GAME, "simple", 30, 1), 2)
    big = kr.layout_params(GAME, "simple", 30)
    big.update(height=10, width=11, terrain=[2] * 110)
    with pytest.raises(ValueError):
        ref.RefSimplecooked(big, 2)
    three = kr.layout_params(GAME, "simple", 30)
    three.update(num_players=3, start_player_x=[1, 2, 3], start_player_y=[1, 1, 1])
    with pytest.raises(ValueError):
        ref.RefSimplecooked(three, 2)
