"""CPU oracle (oracle/hanabi_oracle.c) against the reference's own Hanabi sim.cpp, compiled unchanged against the Madrona
stand-in (oracle/_ref/libref_hanabi.so, see oracle/ref.py).  Bit-exact after every step: both agents' observation, state,
mask, active flag and reward, the world's done flag and the episode counter.

Thousands of worlds play hundreds of steps with moves drawn from the reference's own mask, under policies that force the
rare paths; each path's count is asserted to be at least one.  Two reference instances run side by side: components
start as 0x00 without constructors, and as 0xA5 with default-initialisation (LastMove's member initialisers run).  They
must agree with each other -- nothing the reference reads is memory it never wrote, and whether constructors run does
not matter -- and their guard bytes may hold only the documented overflow: with nine information tokens the full
configuration writes one byte past the 658-byte observation and the 783-byte state per token above the maximum
(sim.cpp:119-125 with the unconditional token of :676-678).
"""
import numpy as np
import pytest

from madrona_rl_envs_playground_amd import hanabi_spec
from oracle import ref
from oracle.oracle import HanabiOracle

import hanabi_configs
import hanabi_illegal_cases
from hanabi_configs import choose, count_paths, reachable, tokens_after_move  # noqa: F401  (choose: test_gpu_hanabi.py imports it from here)

CONFIGS = {
    "full": dict(colors=5, ranks=5, players=2, max_information_tokens=8, max_life_tokens=3),
    "small": dict(colors=2, ranks=5, players=2, max_information_tokens=3, max_life_tokens=1),
    "very_small": dict(colors=1, ranks=5, players=2, max_information_tokens=3, max_life_tokens=1),
}
# very_small deals its 10 cards into the two hands: the deck is empty from the start and a game is two moves (sim.cpp:598-600,
# 842), the first with the information pool full (no discard, :400).  Three paths cannot occur there, nor in any other game
# without a deck: hanabi_configs.UNREACHABLE_WITHOUT_A_DECK.


@pytest.fixture(scope="module", autouse=True)
def _ref_built():
    ref.require()


def _assert_same(name, step, orc, refs, ob_n, st_n):
    where = f"{name}, step {step}"
    for r in refs:
        assert np.array_equal(r.obs[:, :, :ob_n], orc.obs[:, :, :ob_n]), f"{where}: observation"
        assert np.array_equal(r.state[:, :, :st_n], orc.state[:, :, :st_n]), f"{where}: state"
        for k in ("mask", "active", "reward", "done"):
            assert np.array_equal(getattr(r, k), getattr(orc, k)), f"{where}: {k}"
        assert r.episodes == orc.episodes, f"{where}: episode counter"


def _check_guards(name, cfg, ob_n, st_n, r, info_after):
    """Only the documented overflow: in a world holding `max + e` information tokens the first e bytes past the observation
    and past the state (every later section moves up by e), and only where the rows are exactly as long as their arrays
    (full config)."""
    g = r.guards()
    if not len(g):
        return 0
    assert ob_n == ref.HANABI_OBS and st_n == ref.HANABI_STATE, f"{name}: guard bytes written {g[:4].tolist()}"
    assert set(g[:, 2].tolist()) <= {ref.GUARD_OBSERVATION, ref.GUARD_STATE}, g[:4].tolist()
    excess = info_after[g[:, 0]] - cfg["max_information_tokens"]
    assert ((g[:, 3] >= 0) & (g[:, 3] < excess)).all(), f"{name}: a write other than the {excess} bytes past a row: {g[:4].tolist()}"
    assert set(g[:, 4].tolist()) <= {0, 1}
    return len(g)


@pytest.mark.parametrize("name,n,steps", [("full", 2000, 300), ("small", 1500, 250), ("very_small", 1000, 200)] +
                         [(cid, 600, 200) for cid in hanabi_configs.IDS])
def test_oracle_matches_compiled_reference(name, n, steps):
    cfg = CONFIGS.get(name) or hanabi_configs.BY_ID[name]
    ob_n, st_n = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg)
    orc = HanabiOracle(cfg, n)
    refs = [ref.RefHanabi(cfg, n, fill=0x00, construct=False), ref.RefHanabi(cfg, n, fill=0xA5, construct=True)]
    _assert_same(name, -1, orc, refs, ob_n, st_n)
    # what the reference never writes stays what the stand-in filled it with: the tail of a shorter configuration's rows
    assert (refs[1].obs[:, :, ob_n:] == 0xA5).all() and (refs[1].state[:, :, st_n:] == 0xA5).all()
    rng = np.random.default_rng(20261016)
    counts, compared, guard_bytes = {}, 0, 0
    for t in range(steps):
        rec = orc.dump()
        acts = choose(rng, cfg, refs[0].mask, rec)
        orc.step(acts)
        for r in refs:
            r.step(acts)
        _assert_same(name, t, orc, refs, ob_n, st_n)
        for k, v in count_paths(cfg, rec, acts, orc.done).items():
            counts[k] = counts.get(k, 0) + v
        info_after = tokens_after_move(cfg, rec, acts)
        for r in refs:
            guard_bytes += _check_guards(name, cfg, ob_n, st_n, r, info_after)
        compared += n
    print(f"hanabi {name}: {compared} world-steps compared bit-exact, {orc.episodes} episodes, "
          f"{guard_bytes} overflow guard bytes; forced paths: {counts}")
    for k, v in counts.items():
        if not reachable(cfg, k):
            continue
        assert v >= 1, f"{name}: the policies never took the path '{k}' ({counts})"
    if name == "full":
        assert guard_bytes >= 1, "the full configuration's documented one-byte overflow never happened"
    else:
        assert name in CONFIGS or guard_bytes == 0, f"{name}: {guard_bytes} guard bytes written"


@pytest.mark.parametrize("name", hanabi_illegal_cases.WALK_CONFIGS)
def test_oracle_matches_compiled_reference_on_moves_the_mask_forbids(name):
    """hanabi_illegal_cases.walk -- empty hints (A), discards at a full pool (B) and actions past the move table or negative
    (E: the reference's rank hint, at the mover's own hand when u / R is odd) side by side with legal moves -- on four times
    the device tests' worlds: every tensor of both agents after every step, in both reference instances, and the guard bytes,
    which may hold only the documented overflow of `max + e` tokens.  (The reference exports no game record; its hands and
    their knowledge are compared through the state rows.)"""
    ic = hanabi_illegal_cases
    cfg, n = ic.config_of(name), 4 * ic.WORLDS
    ob_n, st_n = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg)
    orc = HanabiOracle(cfg, n)
    refs = [ref.RefHanabi(cfg, n, fill=0x00, construct=False), ref.RefHanabi(cfg, n, fill=0xA5, construct=True)]
    _assert_same(name, -1, orc, refs, ob_n, st_n)
    total, guard_bytes = {}, 0
    for t, rec, acts, cls in ic.walk(orc, cfg, reference_contract=True):
        assert np.array_equal(refs[0].mask, refs[1].mask)
        for r in refs:
            r.step(acts)
        _assert_same(name, t, orc, refs, ob_n, st_n)
        info_after = ic.tokens_after(cfg, rec, acts)
        assert (info_after <= cfg["max_information_tokens"] + ic.MAX_EXCESS).all() and (info_after >= 0).all()
        for r in refs:
            guard_bytes += _check_guards(name, cfg, ob_n, st_n, r, info_after)
        for k, v in ic.count_classes(cfg, rec, acts, cls, orc.done).items():
            total[k] = total.get(k, 0) + v
    print(f"hanabi {name}: {n * ic.STEPS} world-steps with illegal moves compared bit-exact, {guard_bytes} overflow guard bytes; {total}")
    for k in ("A", "B", "E", "E at the partner", "E at the mover's own hand", "episodes ended"):
        assert total[k] >= 100, f"{name}: {k} occurred {total[k]} times"
    assert name != "full" or guard_bytes >= 1


def test_episode_index_wraps():
    """The episode counter starts 30 short of 2^32: resets hand out 2^32 - 30 .. 2^32 - 1, then 0, 1, ... (uint32),
    in ascending world order, on both sides."""
    cfg, n = CONFIGS["full"], 400
    first = (1 << 32) - 30
    orc = HanabiOracle(cfg, n, first_episode=first)
    r = ref.RefHanabi(cfg, n, first_episode=first)
    ob_n, st_n = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg)
    _assert_same("wrap", -1, orc, [r], ob_n, st_n)
    assert orc.episodes == (first + n) % (1 << 32)
    rng = np.random.default_rng(5)
    for t in range(150):
        acts = choose(rng, cfg, r.mask, orc.dump())
        orc.step(acts)
        r.step(acts)
        _assert_same("wrap", t, orc, [r], ob_n, st_n)
    assert orc.episodes > (first + n) % (1 << 32)  # games ended after the wrap too
