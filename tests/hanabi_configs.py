"""Hanabi games beyond the three the reference names (full, small, very_small), and the move policies that force the rare
paths: shared by the CPU tests against the compiled reference (test_ref_hanabi.py), the oracle's own tests
(test_oracle_hanabi.py) and the device tests (test_gpu_hanabi_configs.py).

The library accepts 1..5 colours (K), 2..5 ranks (R), 1..8 information tokens and 1..3 life tokens, and refuses the
four (K, R) pairs whose deck (4 + 2 (R - 2)) K - 10 would be negative after dealing two hands of five (DECKLESS).
CONFIGS is a spread over what is left: every R, K on both sides of R, decks of 0, 2 and 40, token pools at both ends.
test_oracle_hanabi.py:test_config_list_keeps_its_spread asserts the spread, so an edit cannot lose it.

Nothing here imports torch or needs a GPU.
"""
import numpy as np

MV_DISCARD, MV_PLAY, MV_INVALID = 0, 1, 4
HAND = 5
POLICIES = 5  # world w follows policy w % 5: random, hints first, burn, run out the deck, complete at full tokens


def config(colors, ranks, information, life):
    return dict(colors=colors, ranks=ranks, players=2, max_information_tokens=information, max_life_tokens=life)


def config_id(cfg):
    return "k%dr%di%dl%d" % (cfg["colors"], cfg["ranks"], cfg["max_information_tokens"], cfg["max_life_tokens"])


CONFIGS = [config(*t) for t in [(3, 5, 8, 3), (4, 5, 5, 2), (5, 4, 8, 3), (5, 3, 8, 3), (5, 2, 8, 3), (3, 3, 4, 2), (2, 4, 1, 1),
                                (4, 2, 2, 3), (3, 2, 1, 1), (2, 3, 8, 3), (1, 5, 1, 1), (4, 4, 7, 2), (5, 5, 1, 3), (2, 3, 3, 1)]]
IDS = [config_id(c) for c in CONFIGS]
BY_ID = dict(zip(IDS, CONFIGS))
DECKLESS = [(1, 2), (1, 3), (1, 4), (2, 2)]  # (K, R) with K * R < 5: ten cards do not exist


def deck_size(cfg):
    """Cards left once both hands are dealt: per colour three of the lowest rank, one of the highest, two of the others."""
    return (4 + 2 * (cfg["ranks"] - 2)) * cfg["colors"] - 2 * HAND


def variant(cfg):
    """The code variant the library picks at creation: 2 the full game, 1 five ranks, 0 any configuration."""
    if (cfg["colors"], cfg["ranks"], cfg["max_information_tokens"], cfg["max_life_tokens"]) == (5, 5, 8, 3):
        return 2
    return 1 if cfg["ranks"] == 5 else 0


# With an empty deck from the start a game is two moves (sim.cpp:598-600, 842), the first with the information pool full
# (no discard, :400).  These paths cannot occur there.
UNREACHABLE_WITHOUT_A_DECK = ("hint after a discard", "firework completed at full tokens", "moves seen with tokens above the maximum")


def reachable(cfg, path):
    return deck_size(cfg) > 0 or path not in UNREACHABLE_WITHOUT_A_DECK


def _pick(rng, allowed):
    """One uniformly drawn True column per row of `allowed` (N, 20); -1 where a row has none."""
    score = rng.random(allowed.shape) * allowed
    return np.where(allowed.any(-1), score.argmax(-1), -1)


def choose(rng, cfg, mask, rec):
    """The movers' actions (2, N) for the five policies, from the reference's mask and the game records."""
    K, R, max_info = cfg["colors"], cfg["ranks"], cfg["max_information_tokens"]
    n = rec.shape[0]
    w = np.arange(n)
    mover = rec[:, 83].astype(np.int64)
    legal = mask[mover, w] != 0                                         # (N, 20)
    uid = np.arange(20)
    is_discard, is_play, is_hint = uid < HAND, (uid >= HAND) & (uid < 2 * HAND), (uid >= 2 * HAND) & (uid < 2 * HAND + K + R)
    hand = rec[w[:, None], 100 + 36 * mover[:, None] + np.arange(HAND)].astype(np.int64)
    size = rec[w, 105 + 36 * mover].astype(np.int64)
    fw = rec[:, 76:81].astype(np.int64)
    playable = (np.arange(HAND) < size[:, None]) & (fw[w[:, None], np.minimum(hand // R, 4)] == hand % R)
    info = rec[:, 81].astype(np.int64)

    a_random = _pick(rng, legal)
    a_hint = _pick(rng, legal & is_hint)
    a_discard = _pick(rng, legal & is_discard)
    a_play_ok = _pick(rng, np.pad(playable, ((0, 0), (HAND, 20 - 2 * HAND))))
    a_useless_discard = _pick(rng, legal & np.pad(~playable, ((0, 0), (0, 20 - HAND))))

    pol = w % POLICIES
    act = a_random.copy()
    act = np.where((pol == 1) & (a_hint >= 0), a_hint, act)                        # hints whenever legal
    act = np.where(pol == 2, HAND, act)                                            # play card 0: burns the life tokens
    run = np.where(a_discard >= 0, a_discard, np.where(a_hint >= 0, a_hint, HAND))  # discard / hint: runs the deck out
    act = np.where(pol == 3, run, act)
    # play a playable card only with the information pool full, so that a completed firework brings the ninth token
    full = info >= max_info
    complete = np.where(full & (a_play_ok >= 0), a_play_ok,
                        np.where(~full & (a_useless_discard >= 0), a_useless_discard,
                                 np.where(~full & (a_discard >= 0), a_discard,
                                          np.where(a_hint >= 0, a_hint, a_random))))
    act = np.where(pol == 4, complete, act)
    acts = np.zeros((2, n), np.int32)
    acts[mover, w] = act
    return acts


def tokens_after_move(cfg, rec, acts):
    """Information tokens once the move of `acts` is made, before checkDone may reset the world (sim.cpp:646, 676-678,
    700, 749): a discard and a completed firework add one, a hint spends one."""
    R = cfg["ranks"]
    n = rec.shape[0]
    w = np.arange(n)
    mover = rec[:, 83].astype(np.int64)
    uid = acts[mover, w].astype(np.int64)
    card = rec[w, 100 + 36 * mover + np.clip(uid - HAND, 0, HAND - 1)].astype(np.int64)
    play = (uid >= HAND) & (uid < 2 * HAND)
    completes = play & (rec[w, 76 + np.minimum(card // R, 4)] == card % R) & (card % R == R - 1)
    return rec[:, 81].astype(np.int64) + (uid < HAND) + completes - (uid >= 2 * HAND)


def count_paths(cfg, rec, acts, done):
    """Which rare paths the step from records `rec` with actions `acts` took, as counts."""
    K, R, max_info = cfg["colors"], cfg["ranks"], cfg["max_information_tokens"]
    n = rec.shape[0]
    w = np.arange(n)
    mover = rec[:, 83].astype(np.int64)
    uid = acts[mover, w].astype(np.int64)
    hint = uid >= 2 * HAND
    play = (uid >= HAND) & (uid < 2 * HAND)
    card = rec[w, 100 + 36 * mover + np.clip(uid - HAND, 0, HAND - 1)].astype(np.int64)
    fw = rec[w, 76 + np.minimum(card // R, 4)].astype(np.int64)
    scores = play & (fw == card % R)
    last_move, last_player = rec[:, 87], rec[:, 88]
    return {
        "hint as an episode's first move": int((hint & (last_player == 0xFF)).sum()),
        "hint after a play": int((hint & (last_move == MV_PLAY)).sum()),
        "hint after a discard": int((hint & (last_move == MV_DISCARD)).sum()),
        "last life token burnt": int((play & ~scores & (rec[:, 82] == 1) & (done != 0)).sum()),
        "deck out, last round played": int(((rec[:, 50] == 0) & (rec[:, 84] == 1) & (done != 0)).sum()),
        "firework completed at full tokens": int((scores & (card % R == R - 1) & (rec[:, 81] == max_info)).sum()),
        "moves seen with tokens above the maximum": int((rec[:, 81] > max_info).sum()),
    }


# ---------------------------------------------------------------------------------------------------------------------
# The walk the device lock-step follows (test_gpu_hanabi_configs.py) and its CPU twin checks for coverage
# (test_oracle_hanabi.py:test_lockstep_walk_reaches_every_path): the oracle alone, moves from `choose` on the oracle's own
# mask and records.  A Hanabi workgroup owns 256 worlds; 700 are three workgroups with a ragged last one.
# ---------------------------------------------------------------------------------------------------------------------
WALK_WORLDS = 700
WALK_SEED = 20261018
WALK_STEPS = {cid: 120 for cid in IDS}  # raised per configuration where 120 steps leave a reachable path at zero


def walk(orc, cfg, steps, seed=WALK_SEED):
    """Steps `orc` (a HanabiOracle of this configuration) `steps` times; yields (t, records before the step, actions)
    after each oracle step, so that a simulator fed the same actions can be compared with `orc` there."""
    rng = np.random.default_rng(seed)
    for t in range(steps):
        rec = orc.dump()
        acts = choose(rng, cfg, orc.mask, rec)
        orc.step(acts)
        yield t, rec, acts
