"""CPU: the Overcooked oracle (oracle/overcooked_oracle.c) against the golden
vectors produced by the reference's numpy implementation
(tests/golden/make_overcooked_golden.py).  This is what pins the oracle."""
import glob
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

FIXTURES = sorted(f for f in glob.glob(os.path.join(GOLDEN, "overcooked_*.npz")) if "_ref_" not in os.path.basename(f))


def test_fixtures_present():
    assert len(FIXTURES) >= 13


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[11:-4])
def test_oracle_reproduces_reference(path, oracle_lib):
    z = np.load(path)
    params = json.loads(str(z["params"]))
    acts, obs, rew, done = z["actions"], z["obs"], z["reward"], z["done"]
    n = 3
    orc = oracle_lib.OvercookedOracle(params, n, num_threads=2)
    assert np.array_equal(orc.obs, np.broadcast_to(obs[0], orc.obs.shape))
    P = params["num_players"]
    for t in range(len(acts)):
        orc.step(np.repeat(acts[t].astype(np.int32)[:, None], n, axis=1))
        assert np.array_equal(orc.obs, np.broadcast_to(obs[t + 1], orc.obs.shape)), f"obs, step {t}"
        assert (orc.reward == rew[t]).all() and orc.reward.shape == (P, n), f"reward, step {t}"
        assert (orc.done == done[t]).all(), f"done, step {t}"


def test_thread_count_does_not_change_results(oracle_lib):
    from madrona_rl_envs_playground_amd import layouts
    params = layouts.get_base_layout_params("coordination_ring", 40)
    n = 257
    a, b = oracle_lib.OvercookedOracle(params, n, 1), oracle_lib.OvercookedOracle(params, n, 8)
    rng = np.random.default_rng(3)
    for _ in range(100):
        acts = rng.integers(0, 6, size=(2, n)).astype(np.int32)
        a.step(acts)
        b.step(acts)
        assert np.array_equal(a.obs, b.obs) and np.array_equal(a.reward, b.reward) and np.array_equal(a.done, b.done)


def test_observation_is_a_function_of_state(oracle_lib):
    """The reference updates rows in place (player channels are cleared through
    past_player only); the HIP kernel recomputes them.  Property that makes the
    two agree: equal dumped states imply equal observations, across worlds
    whatever their histories."""
    from madrona_rl_envs_playground_amd import layouts
    params = layouts.get_base_layout_params("cramped_room", 1000)
    n = 4000
    orc = oracle_lib.OvercookedOracle(params, n, 4)
    rng = np.random.default_rng(11)
    seen = {}
    for t in range(40):
        orc.step(rng.integers(0, 6, size=(2, n)).astype(np.int32))
        pl, ob, ts = orc.dump()
        urgent = (1000 - ts) < 40
        for w in range(0, n, 7):
            key = (pl[w].tobytes(), ob[w].tobytes(), bool(urgent[w]))
            if key in seen:
                assert np.array_equal(seen[key], orc.obs[w])
            else:
                seen[key] = orc.obs[w].copy()
    assert len(seen) > 50
