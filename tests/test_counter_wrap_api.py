"""No GPU: the oracles that start at a chosen episode (orc_cartpole_create_at, orc_balance_create_at), and the case tables
of wrap_cases.py asserted from the tables alone -- every placement's conditions, Hanabi's committed k re-derived by the
oracle walk, the planted steps finishing exactly the worlds the tables say, and the spread of the cases."""
import ctypes

import numpy as np
import pytest

import hanabi_configs
import wrap_cases as wc
from conftest import load_golden
from wrap_cases import GROUP, HANABI_GROUP, LARGE, PLACEMENTS, SMALL, TWO32

NEAR = TWO32 - 5


def _raw(oracle_lib, game, handle, n):
    """every array of an oracle created through the C functions themselves, as bytes"""
    L = oracle_lib.lib()
    if game == "cartpole":
        parts = [(L.orc_cartpole_state, 4 * n, ctypes.c_float), (L.orc_cartpole_reward, n, ctypes.c_float), (L.orc_cartpole_done, n, ctypes.c_int32)]
    else:
        parts = [(L.orc_balance_obs, 14 * n, ctypes.c_int32), (L.orc_balance_loc, 2 * n, ctypes.c_int32), (L.orc_balance_time, n, ctypes.c_int32),
                 (L.orc_balance_reward, 2 * n, ctypes.c_float), (L.orc_balance_done, n, ctypes.c_int32)]
    return b"".join(ctypes.string_at(fn(handle), count * ctypes.sizeof(kind)) for fn, count, kind in parts)


@pytest.mark.parametrize("game", ["cartpole", "balance"])
def test_create_at_zero_is_create(game, oracle_lib):
    L = oracle_lib.lib()
    n = 1500
    create, create_at = getattr(L, f"orc_{game}_create"), getattr(L, f"orc_{game}_create_at")
    destroy, episodes = getattr(L, f"orc_{game}_destroy"), getattr(L, f"orc_{game}_episodes")
    a, b = create(n), create_at(n, 0)
    assert _raw(oracle_lib, game, a, n) == _raw(oracle_lib, game, b, n)
    assert episodes(a) == episodes(b) == n
    acts = (np.arange(2 * n) % 2).astype(np.int32)
    for _ in range(3):  # and they go on alike
        for h in (a, b):
            if game == "cartpole":
                L.orc_cartpole_step(h, acts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1)
            else:
                L.orc_balance_step(h, acts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert _raw(oracle_lib, game, a, n) == _raw(oracle_lib, game, b, n) and episodes(a) == episodes(b)
    destroy(a)
    destroy(b)
    # the Python constructors: the default is episode 0
    if game == "cartpole":
        plain, at_zero = oracle_lib.CartpoleOracle(n), oracle_lib.CartpoleOracle(n, first_episode=0)
        assert plain.state.tobytes() == at_zero.state.tobytes() and plain.episodes == at_zero.episodes == n
    else:
        plain, at_zero = oracle_lib.BalanceOracle(n), oracle_lib.BalanceOracle(n, first_episode=0)
        assert plain.obs.tobytes() == at_zero.obs.tobytes() and plain.episodes == at_zero.episodes == n


def test_cartpole_world_j_starts_episode_first_plus_j(oracle_lib):
    many = oracle_lib.CartpoleOracle(10, first_episode=NEAR)
    for j in range(10):
        e = (NEAR + j) % TWO32
        one = oracle_lib.CartpoleOracle(1, first_episode=e)
        assert one.state[0].tobytes() == many.state[j].tobytes(), f"world {j}"
        want = (np.float32(-0.05) + oracle_lib.rng_stream(e, 4) * np.float32(0.1)).astype(np.float32)
        assert want.tobytes() == many.state[j].tobytes(), f"world {j}: the reset formula"
    zero = oracle_lib.CartpoleOracle(1)
    assert many.state[5].tobytes() == zero.state[0].tobytes()  # world 5 is episode 0
    assert many.episodes == 5  # the counter wrapped


def test_balance_world_j_starts_episode_first_plus_j(oracle_lib):
    many = oracle_lib.BalanceOracle(10, first_episode=NEAR)
    for j in range(10):
        one = oracle_lib.BalanceOracle(1, first_episode=(NEAR + j) % TWO32)
        assert one.obs[:, 0].tobytes() == many.obs[:, j].tobytes(), f"world {j}: observation rows"
        assert one.loc[:, 0].tobytes() == many.loc[:, j].tobytes() and one.time[0] == many.time[j], f"world {j}: positions, time"
    zero = oracle_lib.BalanceOracle(1)
    assert many.obs[:, 5].tobytes() == zero.obs[:, 0].tobytes()
    assert many.episodes == 5


@pytest.mark.parametrize("game", ["cartpole", "balance"])
def test_episodes_wraps_while_stepping(game, oracle_lib):
    """planted steps from 3 below 2^32: the counter goes 2^32 - 3 -> 4 -> 11, and the finished worlds take 2^32 - 3, 2^32 - 2, 2^32 - 1, 0, ..."""
    n = 40
    first = TWO32 - 3 - n
    hit = np.zeros(n, bool)
    hit[[1, 5, 8, 13, 21, 34, 39]] = True
    if game == "cartpole":
        orc = oracle_lib.CartpoleOracle(n, first_episode=first)
        assert orc.episodes == TWO32 - 3
        state, acts = wc.cartpole_plant(orc.state, hit, 0)
        orc.state[:] = state
        orc.step(acts)
        assert np.array_equal(orc.done[:, 0] != 0, hit) and orc.episodes == 4
        assert orc.state[hit].tobytes() == wc.cartpole_fresh(oracle_lib, TWO32 - 3, 7).tobytes()
    else:
        orc = oracle_lib.BalanceOracle(n, first_episode=first)
        assert orc.episodes == TWO32 - 3
        obs, acts = wc.balance_plant(hit, 0)
        orc.plant(obs)
        orc.step(acts)
        assert np.array_equal(orc.done != 0, hit) and orc.episodes == 4
        assert orc.obs[:, hit].tobytes() == wc.balance_fresh(oracle_lib, TWO32 - 3, 7).tobytes()


def test_compiled_reference_starts_at_the_same_episode(oracle_lib):
    """oracle/_ref's RefCartpole / RefBalance with the same first_episode, through the crossing, as test_ref_cartpole.py and
    test_ref_balance.py compare them from episode 0"""
    from oracle import ref
    ref.require()
    n = 3000
    first = TWO32 - n - 2000
    orc, r = oracle_lib.CartpoleOracle(n, first_episode=first), ref.RefCartpole(n, first_episode=first)
    for t in range(61):
        assert np.array_equal(r.state.view(np.uint32), orc.state.view(np.uint32)), f"cartpole step {t}: state"
        assert np.array_equal(r.done, orc.done) and r.episodes == orc.episodes, f"cartpole step {t}"
        a = np.ones(n, np.int32)  # every world ends on about the same step: batches of resets in world order
        orc.step(a)
        r.step(a)
    assert 2000 < orc.episodes < first and not len(r.guards())  # it wrapped and went on
    first = TWO32 - n - 4000
    orc, r = oracle_lib.BalanceOracle(n, first_episode=first), ref.RefBalance(n, first_episode=first)
    rng = np.random.default_rng(3)
    for t in range(9):
        for k in ("obs", "loc", "time", "reward", "done"):
            assert np.array_equal(getattr(r, k), getattr(orc, k)), f"balance step {t}: {k}"
        assert r.episodes == orc.episodes, f"balance step {t}"
        a = rng.integers(0, 4, size=(2, n)).astype(np.int32)
        orc.step(a)
        r.step(a)
    assert 2000 < orc.episodes < first and not len(r.guards())


# ---------------------------------------------------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------------------------------------------------
CASES = [(game, n, placement) for (game, n), table in wc.PLANTED.items() for placement in table]


@pytest.mark.parametrize("game,n,placement", CASES, ids=[f"{g}_{n}_{p}" for g, n, p in CASES])
def test_planted_placement_conditions(game, n, placement):
    k, first, second = wc.PLANTED[(game, n)][placement]
    groups = (n + GROUP - 1) // GROUP
    assert len(first) == len(second) == groups and 0 < k < TWO32
    low, counts = wc.before(first), np.asarray(first)
    if placement == "inside_workgroup":
        b = wc.crossing_workgroup(k, first)
        assert b > 0 and low[b] > 0, "a lower workgroup must have finished worlds"
        assert low[b] < k < low[b] + counts[b], "finished worlds of b on both sides of 2^32"
        if n == LARGE:
            assert b >= wc.LOOKBACK_GROUP and low[wc.LOOKBACK_GROUP] > 0, "the crossing lies in the second look-back group"
    elif placement == "between_workgroups":
        b = wc.crossing_workgroup(k, first)
        assert counts[b] > 0 and low[b] + counts[b] == k and counts[b + 1] > 0
        if n == LARGE:
            assert b + 1 == wc.LOOKBACK_GROUP, "the boundary is the one between the look-back groups"
    else:
        assert int(counts.sum()) == k and sum(second) > 0, "the step leaves the counter at 0 and the next one finishes worlds"
    assert wc.placement_holds(placement, k, first)
    assert sum(second) > 0 and sum(first) >= k, "the crossing is in step 1, step 2 numbers from beyond it"
    if game == "acrobot":
        assert k <= wc.ACROBOT_LAST
    # the worlds: per workgroup as the table says, and the episode numbers around the crossing
    for counts_of_step in (first, second):
        hit = wc.finished_worlds(n, counts_of_step)
        assert wc.counts_of(hit) == tuple(counts_of_step)
    hit = wc.finished_worlds(n, first)
    e = wc.episodes_of(TWO32 - k, hit)
    worlds = np.flatnonzero(hit)
    last_below, first_above = worlds[k - 1], (worlds[k] if k < len(worlds) else None)
    assert e[last_below] == TWO32 - 1
    if placement == "inside_workgroup":
        assert last_below // GROUP == first_above // GROUP == wc.crossing_workgroup(k, first) and e[first_above] == 0
    elif placement == "between_workgroups":
        assert first_above // GROUP == last_below // GROUP + 1 and e[first_above] == 0
    else:
        assert first_above is None


def test_planted_steps_finish_exactly_the_tables_worlds(oracle_lib):
    """the planting helpers on the CPU: the oracles (Cartpole, balance beam) and the fixture's own done flags (Acrobot) end
    the planted worlds and no others, in both steps of every case"""
    gold = load_golden("acrobot_ref.npz")
    base = {n: wc.cartpole_fresh(oracle_lib, 0, n) for n in (SMALL, LARGE)}
    for (game, n), table in wc.PLANTED.items():
        for placement in table:
            k, hits = wc.planted_case(game, n, placement)
            for step, hit in enumerate(hits):
                if game == "cartpole":
                    orc = oracle_lib.CartpoleOracle(n, num_threads=8)
                    state, acts = wc.cartpole_plant(base[n], hit, step)
                    orc.state[:] = state
                    orc.step(acts)
                    done = orc.done[:, 0] != 0
                elif game == "balance":
                    orc = oracle_lib.BalanceOracle(n)
                    obs, acts = wc.balance_plant(hit, step)
                    orc.plant(obs)
                    orc.step(acts)
                    done = orc.done != 0
                else:
                    # which transition of the fixture each world was given, found again by its state and action
                    state, acts = wc.acrobot_plant(gold, hit, step)
                    key = {(s.tobytes(), int(a)): int(d) for s, a, d in zip(gold["swing_state"], gold["swing_action"], gold["swing_done"])}
                    done = np.array([key[(s.tobytes(), int(a))] for s, a in zip(state, acts)]) != 0
                assert np.array_equal(done, hit), f"{game} {n} {placement} step {step}"
    # two steps from fresh Cartpole states end nothing: the unplanted worlds of step 2 are as the table says
    orc = oracle_lib.CartpoleOracle(SMALL)
    for acts in ((0, 0), (0, 1), (1, 0), (1, 1)):
        orc.state[:] = base[SMALL]
        for a in acts:
            orc.step(np.full(SMALL, a, np.int32))
            assert not orc.done.any()


def test_hanabi_k_gives_the_crossing_inside_a_workgroup(oracle_lib):
    walk = wc.hanabi_walk(oracle_lib, wc.HANABI_K)
    assert wc.HANABI_K > wc.HANABI_N and wc.HANABI_STEP < wc.HANABI_WALK_STEPS == len(walk)
    distance, counts = walk[wc.HANABI_STEP]
    assert distance is not None and len(counts) == 3
    b = wc.crossing_workgroup(distance, counts)
    low = wc.before(counts)
    assert b > 0 and low[b] > 0 and low[b] < distance < low[b] + counts[b]
    assert wc.placement_holds("inside_workgroup", distance, counts)
    assert all(d is not None and sum(c) < d for d, c in walk[:wc.HANABI_STEP]) and all(d is None for d, _ in walk[wc.HANABI_STEP + 1:])
    assert sum(sum(c) for _, c in walk[:wc.HANABI_STEP]) > 0 and sum(sum(c) for _, c in walk[wc.HANABI_STEP + 1:]) > 0
    for placement, (k, counts) in wc.HANABI_MASKS.items():
        assert len(counts) == 3 and wc.placement_holds(placement, k, counts), placement
        assert wc.counts_of(wc.finished_worlds(wc.HANABI_N, counts, HANABI_GROUP), HANABI_GROUP) == counts


def test_lockstep_walks_end_episodes_on_both_sides_of_the_crossing(oracle_lib):
    for game, (k, steps) in wc.LOCKSTEP.items():
        n = wc.LOCKSTEP_WORLDS[game]
        distance = k - n
        assert distance > 0
        if game == "hanabi":
            totals = [sum(c) for _, c in wc.hanabi_walk(oracle_lib, k, steps)]
        else:
            orc = (oracle_lib.CartpoleOracle if game == "cartpole" else oracle_lib.BalanceOracle)(n, first_episode=TWO32 - k)
            assert orc.episodes == TWO32 - distance
            rng = np.random.default_rng(wc.LOCKSTEP_SEED)
            totals = []
            for _ in range(steps):
                at = orc.episodes
                orc.step(wc.lockstep_actions(game, rng, n))
                totals.append((orc.episodes - at) % TWO32)
        below, above = wc.numbers_handed_out(distance, totals)
        assert below == distance and above > 100, f"{game}: {below} episodes below 2^32, {above} from 0 on"
        cum = np.cumsum(totals)
        crossing = int(np.flatnonzero(cum >= distance)[0])
        assert steps // 4 <= crossing < 3 * steps // 4 and cum[crossing - 1] > 0, f"{game}: the crossing falls in step {crossing}"


def test_case_tables_keep_their_spread():
    """all four games, all three placements, both sizes for Cartpole: an edit cannot lose a case"""
    assert set(wc.PLANTED) == {("cartpole", SMALL), ("cartpole", LARGE), ("balance", SMALL), ("acrobot", SMALL)}
    for table in list(wc.PLANTED.values()) + [wc.HANABI_MASKS]:
        assert tuple(table) == PLACEMENTS
    assert SMALL == 3 * 1024 + 5 and LARGE == 262144 + 1024 + 5 and (LARGE + GROUP - 1) // GROUP == 258
    assert {g for g, _ in wc.PLANTED} | {"hanabi"} == set(wc.GAMES) and set(wc.LOCKSTEP) == {"cartpole", "balance", "hanabi"}
    assert wc.HANABI_N == 700 and hanabi_configs.BY_ID[wc.HANABI_CONFIG]["ranks"] == 2
    firsts = [wc.PLANTED[key][p][1] for key in wc.PLANTED for p in PLACEMENTS]
    assert any(GROUP in c for c in firsts), "a workgroup whose every world finishes"
    assert any(0 in c[:-1] for c in firsts), "a workgroup with none"
    assert any(c[-1] == 5 for c in firsts), "the whole ragged tail"
    ks = [wc.PLANTED[key][p][0] for key in wc.PLANTED for p in PLACEMENTS]
    assert min(ks) <= 8 and max(ks) > 2000
