"""The episode counter across 2^32: case tables, planting helpers and expected values, shared by test_counter_wrap_api.py
(no GPU: the tables' own conditions, the oracles) and test_gpu_counter_wrap.py (the kernels).

Hanabi, Cartpole, the balance beam and Acrobot seed every new episode from one uint32 counter; a finished world of rank r
(ascending world order) starts episode (c + r) mod 2^32.  Where the crossing falls is chosen here, not left to chance: the
three lane-per-world games are PLANTED so that the set of worlds that finishes in the next step is known on the host, and
the counter is set to c = 2^32 - k.  Per game three placements:

  inside_workgroup    the crossing is strictly inside the finished worlds of a workgroup b > 0 of the single-launch step
                      (finished worlds below and above 2^32 in b), and a lower workgroup has finished worlds
  between_workgroups  the last finished world of workgroup b takes 2^32 - 1, the first of workgroup b + 1 takes 0
  between_steps       the step's total is exactly k: it leaves the counter at 0 and the next step starts from base 0

A workgroup of the single-launch step owns 1024 consecutive worlds in the three lane-per-world games (GROUP) and 256 in
Hanabi (HANABI_GROUP); the two-launch step's workgroups own 256 (512 at LARGE), so a boundary between the former is
one of the latter too.  SMALL is three full workgroups and a ragged fourth; LARGE (Cartpole) is 258 workgroups, so that
workgroups from 256 on lie in the second group of the two-level look-back (kGroup = 256 in csrc/episode_scan.hpp) and the
totals of lower groups are not zero.  Acrobot's fixture holds the last eight episodes below 2^32, so its k <= 8.

Expected values never come from the device: fresh states from the CPU oracles started at the episode (Cartpole also from
the reset formula on the episode's generator), Acrobot's from its fixture.  Nothing here imports torch or needs a GPU.
"""
import numpy as np

import hanabi_configs

TWO32 = 1 << 32
GROUP = 1024
HANABI_GROUP = 256
LOOKBACK_GROUP = 256
SMALL = 3 * GROUP + 5
LARGE = 262144 + GROUP + 5
PLACEMENTS = ("inside_workgroup", "between_workgroups", "between_steps")
PLANTED_GAMES = ("cartpole", "balance", "acrobot")
GAMES = PLANTED_GAMES + ("hanabi",)
ACROBOT_LAST = 8  # GOLD["fresh_last"]: episodes 2^32 - 8 .. 2^32 - 1


def _large(counts, **at):
    """258 per-workgroup counts from a pattern, single workgroups overwritten"""
    c = np.asarray(counts, np.int64).copy()
    for j, v in at.items():
        c[int(j[1:])] = v
    return tuple(int(v) for v in c)


_J = np.arange(258)
_L_INSIDE = _large(_J * 7 % 13, j257=3)
_L_BETWEEN = _large(_J * 3 % 7, j255=6, j256=2, j257=5)
_L_TOTAL = _large(_J * 11 % 17, j257=5)
# (game, worlds) -> placement -> (k, finished worlds per workgroup in step 1, ... in step 2)
PLANTED = {
    ("acrobot", SMALL): {
        "inside_workgroup": (5, (3, 6, 2, 1), (2, 0, 4, 5)),
        "between_workgroups": (8, (4, 4, 3, 1), (0, 5, 1, 2)),
        "between_steps": (8, (3, 0, 4, 1), (2, 3, 0, 5)),
    },
    ("balance", SMALL): {
        "inside_workgroup": (300 + 217, (300, 500, 1024, 5), (1024, 17, 0, 3)),
        "between_workgroups": (64 + 1024, (64, 1024, 1, 2), (5, 0, 1024, 0)),
        "between_steps": (1 + 333 + 1024 + 5, (1, 333, 1024, 5), (7, 1024, 64, 1)),
    },
    ("cartpole", SMALL): {
        "inside_workgroup": (1024 + 0 + 1, (1024, 0, 3, 5), (3, 1024, 65, 0)),  # workgroup 1 has none: b = 2 looks past it
        "between_workgroups": (129 + 63, (129, 63, 64, 4), (0, 0, 0, 5)),
        "between_steps": (2 + 1024 + 511, (2, 1024, 511, 0), (1024, 1, 0, 2)),
    },
    ("cartpole", LARGE): {
        # the crossing inside workgroup 256, the first of the second look-back group (below it: 256 status words as one total)
        "inside_workgroup": (sum(_L_INSIDE[:256]) + 4, _L_INSIDE, _large(_J * 5 % 11, j0=1024, j257=0)),
        # ... on the boundary between the two look-back groups
        "between_workgroups": (sum(_L_BETWEEN[:256]), _L_BETWEEN, _large(_J * 0, j100=9, j257=1)),
        "between_steps": (sum(_L_TOTAL), _L_TOTAL, _large(_J * 2 % 3, j256=1024, j257=2)),
    },
}
# reset_worlds masks for Hanabi (256-world workgroups: 256 + 256 + 188): placement -> (k, masked worlds per workgroup)
HANABI_N = hanabi_configs.WALK_WORLDS
HANABI_CONFIG = "k3r2i1l1"  # two ranks, one token of each kind: a game is a few moves, 50 to 400 of 700 worlds finish per step
HANABI_MASKS = {
    "inside_workgroup": (5, (3, 6, 2)),
    "between_workgroups": (8, (4, 4, 3)),
    "between_steps": (8, (3, 2, 3)),
}
# Hanabi cannot be planted but is exact: HanabiOracle(first_episode = 2^32 - HANABI_K) walked with hanabi_configs.walk gives
# placement inside_workgroup in step HANABI_STEP (test_counter_wrap_api.py re-derives both)
HANABI_K = 1500
HANABI_STEP = 5
HANABI_WALK_STEPS = 30


def before(counts):
    """finished worlds of the lower workgroups, per workgroup"""
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


def placement_holds(placement, k, counts):
    """Does a step whose workgroups finish `counts` worlds, from the counter 2^32 - k, cross as `placement` says?"""
    counts = np.asarray(counts, np.int64)
    low = before(counts)
    if placement == "inside_workgroup":
        b = np.flatnonzero((low < k) & (k < low + counts))
        return len(b) == 1 and b[0] > 0 and low[b[0]] > 0
    if placement == "between_workgroups":
        b = np.flatnonzero((low + counts == k) & (counts > 0))
        return len(b) > 0 and b[-1] + 1 < len(counts) and counts[b[-1] + 1] > 0
    return int(counts.sum()) == k and k > 0


def crossing_workgroup(k, counts):
    """the workgroup whose finished worlds take 2^32 - 1 (its last one at least)"""
    counts = np.asarray(counts, np.int64)
    low = before(counts)
    return int(np.flatnonzero((low < k) & (k <= low + counts))[0])


def finished_worlds(n, counts, group=GROUP):
    """The worlds (bool, n) that finish: counts[j] of workgroup j, spread evenly over it; even workgroups include their
    first world, odd ones their last (so the ragged tail's last world takes part when its workgroup is odd)."""
    hit = np.zeros(n, bool)
    assert len(counts) == (n + group - 1) // group
    for j, c in enumerate(counts):
        first, size = j * group, min(group, n - j * group)
        assert 0 <= c <= size
        i = np.arange(c)
        if c:
            hit[first + ((i * size) // c if j % 2 == 0 else (i * size + size - 1) // c)] = True
        assert int(hit[first:first + size].sum()) == c
    return hit


def counts_of(hit, group=GROUP):
    n = len(hit)
    return tuple(int(hit[j:j + group].sum()) for j in range(0, n, group))


def episodes_of(c, hit):
    """(n,) int64: the episode each finished world starts, (c + rank) mod 2^32 in ascending world order; -1 elsewhere"""
    rank = np.cumsum(hit) - 1
    return np.where(hit, (int(c) + rank) % TWO32, -1)


def planted_case(game, n, placement):
    k, first, second = PLANTED[(game, n)][placement]
    return k, [finished_worlds(n, first), finished_worlds(n, second)]


# ---------------------------------------------------------------------------------------------------------------------
# planting: the state every world is given before a step, and the step's actions
# ---------------------------------------------------------------------------------------------------------------------
def cartpole_plant(base, hit, step):
    """base: CartpoleOracle(n).state (fresh episodes 0 .. n - 1: two steps of any actions end none of them); a hit world's
    cart stands beyond X_THRESHOLD, on either side: done whatever the action.  -> (state (n, 4), actions (n,))"""
    n = len(hit)
    state = np.array(base, np.float32, copy=True)
    w = np.arange(n)
    state[hit, 0] = np.where(w[hit] % 2 == 0, 3.0, -3.0)
    return state, ((w + step) % 2).astype(np.int32)


def balance_plant(hit, step):
    """Both players between 1 and 3 with moves of +-1 stay on the beam; a hit world is at its last time step (time 1), the
    others have two to go.  -> (obs (2, n, 7), actions (2, n))"""
    n = len(hit)
    w = np.arange(n)
    loc = np.stack([1 + w % 3, 1 + (w // 3 + step) % 3])
    obs = np.zeros((2, n, 7), np.int32)
    for p in range(2):
        obs[p, :, 0] = loc[p] + 2
        obs[p, :, 3] = loc[1 - p] + 2
        obs[p, :, 1] = 2 + (w + p) % 5  # a history, so that a fresh row (zeros) differs from a stale one
        obs[p, :, 6] = np.where(hit, 1, 2)
    actions = np.stack([1 + (w + step) % 2, 1 + (w // 2 + step) % 2]).astype(np.int32)
    return obs, actions


def acrobot_plant(gold, hit, step):
    """swing transitions of the fixture: one that the reference ended for a hit world, one it did not end for the others
    -> (state (n, 4), actions (n,))"""
    n = len(hit)
    ended, alive = np.flatnonzero(gold["swing_done"] != 0), np.flatnonzero(gold["swing_done"] == 0)
    w = np.arange(n) + 31 * step
    idx = np.where(hit, ended[w % len(ended)], alive[w % len(alive)])
    return gold["swing_state"][idx], gold["swing_action"][idx].astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# expected fresh states
# ---------------------------------------------------------------------------------------------------------------------
def cartpole_fresh(oracle_lib, first, m):
    """(m, 4): episodes first, first + 1, ... mod 2^32, from the oracle; its first, middle and last also from the reset
    formula on the episode's generator (sim.cpp:48-66)"""
    orc = oracle_lib.CartpoleOracle(m, first_episode=first)
    out = orc.state.copy()
    orc.close()
    for j in sorted({0, m // 2, m - 1}):
        want = (np.float32(-0.05) + oracle_lib.rng_stream((first + j) % TWO32, 4) * np.float32(0.1)).astype(np.float32)
        assert want.tobytes() == out[j].tobytes()
    return out


def balance_fresh(oracle_lib, first, m):
    """(2, m, 7)"""
    orc = oracle_lib.BalanceOracle(m, first_episode=first)
    out = orc.obs.copy()
    orc.close()
    return out


def acrobot_fresh(gold, first, m):
    """(m, 4) from the fixture: fresh_last are the episodes 2^32 - 8 .. 2^32 - 1, fresh the episodes 0, 1, ..."""
    table = np.concatenate([gold["fresh_last"], gold["fresh"]])
    idx = (np.arange(m) + int(first) + ACROBOT_LAST) % TWO32
    assert idx.max() < len(table), "episode outside the fixture"
    return table[idx]


# ---------------------------------------------------------------------------------------------------------------------
# Hanabi: the walk
# ---------------------------------------------------------------------------------------------------------------------
def hanabi_walk(oracle_lib, k, steps=HANABI_WALK_STEPS, n=HANABI_N):
    """HanabiOracle(first_episode = 2^32 - k) walked alone -> per step (distance of the counter below 2^32 before the step,
    or None once it has wrapped; finished worlds per workgroup)"""
    cfg = hanabi_configs.BY_ID[HANABI_CONFIG]
    orc = oracle_lib.HanabiOracle(cfg, n, first_episode=TWO32 - k)
    out = []
    wrapped = k <= n
    for _ in hanabi_configs.walk(orc, cfg, steps):
        after = orc.episodes
        counts = counts_of(orc.done != 0, HANABI_GROUP)
        start = (after - sum(counts)) % TWO32
        out.append((None if wrapped else TWO32 - start, counts))
        wrapped = wrapped or after < start or after == 0
    orc.close()
    return out



# ---------------------------------------------------------------------------------------------------------------------
# lock-step through the crossing on natural endings: game -> (k, steps); world j starts as episode 2^32 - k + j, so the
# counter starts k - n below 2^32 and the crossing falls near the middle of the steps (test_counter_wrap_api.py walks the
# oracles to assert that)
# ---------------------------------------------------------------------------------------------------------------------
LOCKSTEP = {"cartpole": (SMALL + 1000, 24), "balance": (SMALL + 20000, 20), "hanabi": (HANABI_K, 20)}
LOCKSTEP_SEED = 7
LOCKSTEP_WORLDS = {"cartpole": SMALL, "balance": SMALL, "hanabi": HANABI_N}


def lockstep_actions(game, rng, n):
    """Cartpole (n,), balance beam (2, n): uniform draws (Hanabi's moves are hanabi_configs.walk's)"""
    if game == "cartpole":
        return rng.integers(0, 2, n).astype(np.int32)
    return rng.integers(0, 4, (2, n)).astype(np.int32)


def numbers_handed_out(distance, totals):
    """`totals` worlds finished step by step from a counter `distance` below 2^32 -> (episodes numbered below 2^32, from 0 on)"""
    all_of_them = int(sum(totals))
    return min(all_of_them, distance), max(all_of_them - distance, 0)
