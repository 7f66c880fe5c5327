"""Moves that the legal-move mask forbids, for the Hanabi step: the case tables and the generator shared by the oracle's CPU
tests (test_hanabi_illegal_api.py, test_ref_hanabi.py, test_oracle_hanabi.py) and the device tests
(test_gpu_hanabi_illegal.py).  The reference applies whatever integer arrives (sim.cpp:604 "move is already valid by
definition").  The library's contract (include/mrl_envs.h, ACTION) is the reference's result for every move of the table,
allowed or not, and for a value outside the table the in-table rank hint `mapped_action` names, at the partner: a
departure from the reference where it would hint the mover's own hand (class E below).  So the device tests feed the oracle
the MAPPED action (walk's default), while the tests that pin the oracle to the reference itself feed both the raw one
(walk(..., reference_contract=True)).

Classes of a world's move in one step:
    L  legal: hanabi_configs.choose, its five policies
    A  empty hint: an in-table colour / rank hint that the mask forbids although tokens > 0 -- the target holds no such card
    B  discard at a full pool: a held slot discarded while information_tokens >= max (tokens then exceed the maximum)
    E  out of table: an action at or past 10 + K + R, or negative; only with tokens > 0, so the pool never underflows.  The
       reference falls into its rank-hint branch (sim.cpp:742-754): rank u % R at player (actor + 1 + u / R) % 2 with
       u = uint32(action) - 10 - K -- the mover's OWN hand when u / R is odd
    Z  a hint at zero tokens: the pool wraps to 255 and the reference writes far past its rows.  Outside the reference's
       defined behaviour: never fed to the oracle or the reference (z_hint is for the device's memory-safety test alone)

Slots at or past the hand size are not built: in the two-player game each player moves once in the last round and still
holds five cards then, so a mover's hand is never short.

Nothing here imports torch or needs a GPU.
"""
import numpy as np

from hanabi_configs import HAND, MV_DISCARD, MV_PLAY, _pick, choose, tokens_after_move

L, A, B, E, Z = 0, 1, 2, 3, 4
CLASS_NAMES = {L: "L", A: "A", B: "B", E: "E", Z: "Z"}
ILLEGAL_SHARE = 1.0 / 8  # of the worlds, per class A, B, E and step; the rest (5/8, and where a class cannot be built) is L

# Tokens above the maximum.  The reference advances a running offset, so `max + e` tokens move every later section up by e
# entries and, in the full game, write e bytes past the observation and the state (test_ref_hanabi.py:_check_guards; the
# stand-in's guard zones are 64 bytes).  The library's encoders follow the shift up to e = 5 (csrc/hanabi.hip: info_now =
# min(info, max + 5); legal play alone reaches at most max + K <= max + 5): that is the domain.  Class B is only built while
# it leaves tokens <= max + B_EXCESS; completed fireworks (sim.cpp:676-678, one token each, unconditionally) may add to that,
# and choose_with_illegal replaces the play that would cross the bound.
MAX_EXCESS = 5
B_EXCESS = 3

WORLDS, STEPS, SEED = 300, 64, 20261021  # the device lock-step's own size: one 256-world workgroup and a ragged second one

FULL = dict(colors=5, ranks=5, players=2, max_information_tokens=8, max_life_tokens=3)
SMALL = dict(colors=2, ranks=5, players=2, max_information_tokens=3, max_life_tokens=1)
VERY_SMALL = dict(colors=1, ranks=5, players=2, max_information_tokens=3, max_life_tokens=1)
# one configuration per code variant (2, 1, 0), token pools at both ends, and games without a deck (very_small, k1r5i1l1)
WALK_CONFIGS = ["full", "small", "very_small", "k5r3i8l3", "k2r4i1l1", "k4r5i5l2", "k1r5i1l1"]


def table_size(cfg):
    return 2 * HAND + cfg["colors"] + cfg["ranks"]


def out_of_table(cfg):
    """The fixed list class E draws from: the first value past the table and the next, both parities of u / R right behind
    the table (2 R values; 20..24 and 25..29 in the full game), powers of two and their neighbours, both ends of int32."""
    T, R = table_size(cfg), cfg["ranks"]
    vals = list(range(T, T + 2 * R)) + [63, 64, 127, 128, 255, 256, 1000, 2 ** 31 - 1, -1, -2, -5, -2 ** 31]
    assert all(v >= T or v < 0 for v in vals)
    return np.array(sorted(set(vals)), np.int64)


def reference_hint(cfg, uid):
    """What the reference makes of action `uid` (int32 array) at or past 10 + K, per sim.cpp:742-754: (rank, self) with
    self = 1 where the hinted hand is the mover's own."""
    u = (np.asarray(uid, np.int64) - 2 * HAND - cfg["colors"]) % (1 << 32)
    return u % cfg["ranks"], (u // cfg["ranks"]) & 1


def mapped_action(cfg, acts):
    """The library's contract for actions outside the move table, as one pure function: int32 array -> int32 array.  A value
    at or past 10 + K + R, or negative, becomes the in-table rank hint 10 + K + (u mod R), u = uint32(action) - 10 - K; every
    in-table value stays.  The reference agrees on the rank and, when u / R is even, on the target; when it is odd the
    reference hints the mover's own hand and the library the partner (test_hanabi_illegal_api.py shows both)."""
    a = np.asarray(acts).astype(np.int64)
    rank, _ = reference_hint(cfg, a)
    outside = (a < 0) | (a >= table_size(cfg))
    return np.where(outside, 2 * HAND + cfg["colors"] + rank, a).astype(np.int32)


def tokens_after(cfg, rec, acts):
    """hanabi_configs.tokens_after_move for any int32 action: the reference reads it as uint32, so a negative one is a hint."""
    return tokens_after_move(cfg, rec, np.where(acts < 0, 1 << 20, acts.astype(np.int64)))


def choose_with_illegal(rng, cfg, mask, rec):
    """The movers' actions (2, N) int32 and each world's class (N,), from the oracle's mask and the records before the step."""
    K, R, max_info = cfg["colors"], cfg["ranks"], cfg["max_information_tokens"]
    n = rec.shape[0]
    w = np.arange(n)
    acts = choose(rng, cfg, mask, rec)
    mover = rec[:, 83].astype(np.int64)
    legal = mask[mover, w] != 0
    uid = np.arange(20)
    info = rec[:, 81].astype(np.int64)
    size = rec[w, 105 + 36 * mover].astype(np.int64)
    in_table_hint = (uid >= 2 * HAND) & (uid < table_size(cfg))
    a_empty = _pick(rng, in_table_hint & ~legal & (info > 0)[:, None])
    held = np.pad(np.arange(HAND) < size[:, None], ((0, 0), (0, 20 - HAND)))
    a_full = _pick(rng, held & ((info >= max_info) & (info + 1 <= max_info + B_EXCESS))[:, None])
    pool = out_of_table(cfg)
    a_out = np.where(info > 0, pool[rng.integers(0, len(pool), n)], -1 << 40)
    roll = rng.random(n)
    cls = np.full(n, L)
    act = acts[mover, w].astype(np.int64)
    for k, (code, cand, ok) in enumerate(((A, a_empty, a_empty >= 0), (B, a_full, a_full >= 0), (E, a_out, info > 0))):
        take = (roll >= k * ILLEGAL_SHARE) & (roll < (k + 1) * ILLEGAL_SHARE) & ok
        act = np.where(take, cand, act)
        cls = np.where(take, code, cls)
    out = np.zeros((2, n), np.int32)
    out[mover, w] = act.astype(np.int32)
    # the domain, enforced: a play that would complete a firework at max + MAX_EXCESS tokens gives way to a legal hint
    # (tokens > 0 there and the partner holds cards, so one exists)
    over = tokens_after(cfg, rec, out) > max_info + MAX_EXCESS
    if over.any():
        a_hint = _pick(rng, legal & in_table_hint)
        assert (a_hint[over] >= 0).all()
        out[mover[over], w[over]] = a_hint[over]
        cls = np.where(over, L, cls)
    return out, cls


def z_hint(rec, worlds):
    """Class Z for `worlds` whose pool is empty: the colour hint 10, the mover's entry; (2, len(worlds)) int32."""
    assert (rec[worlds, 81] == 0).all()
    return np.full((2, len(worlds)), 2 * HAND, np.int32)


def count_classes(cfg, rec, acts, cls, done):
    """Counts of one step, keyed as test_hanabi_illegal_api.py asserts them and the device tests print them."""
    n = rec.shape[0]
    w = np.arange(n)
    mover = rec[:, 83].astype(np.int64)
    uid = acts[mover, w]
    _, to_self = reference_hint(cfg, uid)
    last_move, last_player = rec[:, 87], rec[:, 88]
    is_a, is_e = cls == A, cls == E
    return {
        "L": int((cls == L).sum()), "A": int(is_a.sum()), "B": int((cls == B).sum()), "E": int(is_e.sum()),
        "E at the partner": int((is_e & (to_self == 0)).sum()), "E at the mover's own hand": int((is_e & (to_self == 1)).sum()),
        "A as an episode's first move": int((is_a & (last_player == 0xFF)).sum()),
        "A after a play": int((is_a & (last_player != 0xFF) & (last_move == MV_PLAY)).sum()),
        "A after a discard": int((is_a & (last_player != 0xFF) & (last_move == MV_DISCARD)).sum()),
        "episodes ended": int((done != 0).sum()),
        "episodes ended by an illegal move's step": int(((done != 0) & (cls != L)).sum()),
        "episodes ended by the last-round rule": int(((rec[:, 50] == 0) & (rec[:, 84] == 1) & (done != 0)).sum()),
    }


# (configuration, count) pairs that cannot occur, with the reason, as hanabi_configs.UNREACHABLE_WITHOUT_A_DECK is for the
# legal paths.  None: a game without a deck is two moves, but class B makes its first move a discard (at the full pool) and
# class A or E its second, so every count is reachable there too; test_hanabi_illegal_api.py asserts all of them everywhere.
UNREACHABLE = {}


def reachable(name, key):
    return (name, key) not in UNREACHABLE


def walk(orc, cfg, steps=STEPS, seed=SEED, reference_contract=False):
    """Steps `orc` with choose_with_illegal on its own mask and records; yields (t, records before, actions, classes)
    after each oracle step.  The yielded actions are the raw ones, for the device; the oracle is stepped on mapped_action of
    them (the library's contract), or on the raw ones too with `reference_contract` (the reference's own behaviour, for the
    tests that compare the oracle with the reference)."""
    rng = np.random.default_rng(seed)
    for t in range(steps):
        rec = orc.dump()
        acts, cls = choose_with_illegal(rng, cfg, orc.mask, rec)
        orc.step(acts if reference_contract else mapped_action(cfg, acts))
        yield t, rec, acts, cls


def config_of(name):
    import hanabi_configs
    return {"full": FULL, "small": SMALL, "very_small": VERY_SMALL}.get(name) or hanabi_configs.BY_ID[name]
