"""The illegal-move walk of tests/hanabi_illegal_cases.py on the oracle alone: that the inputs the device tests
(test_gpu_hanabi_illegal.py) feed really contain every class, in every configuration, within those tests' own world and
step counts, and that they stay inside the domain in which the reference's behaviour is defined.  No GPU."""
import numpy as np
import pytest

import hanabi_configs
import hanabi_illegal_cases as ic

MIN_COUNT = 100
AT_LEAST_100 = ("A", "B", "E")
AT_LEAST_1 = ("E at the partner", "E at the mover's own hand", "A as an episode's first move", "A after a play", "A after a discard",
              "episodes ended", "episodes ended by the last-round rule")


def test_walk_configurations_cover_every_code_variant_and_both_ends_of_the_pools():
    cfgs = {name: ic.config_of(name) for name in ic.WALK_CONFIGS}
    assert {hanabi_configs.variant(c) for c in cfgs.values()} == {0, 1, 2}
    assert {"full", "small", "very_small", "k5r3i8l3", "k2r4i1l1", "k4r5i5l2"} <= set(cfgs)
    assert any(hanabi_configs.deck_size(c) == 0 for n, c in cfgs.items() if n in hanabi_configs.BY_ID)
    pools = {c["max_information_tokens"] for c in cfgs.values()}
    assert 1 in pools and 8 in pools


@pytest.mark.parametrize("name", ic.WALK_CONFIGS)
def test_out_of_table_list(name):
    """The fixed list: the first value past the table and the next, both parities of u / R right behind it (20..24 and
    25..29 in the full game), the named large values and the named negative ones; and reference_hint on them by hand."""
    cfg = ic.config_of(name)
    K, R, T = cfg["colors"], cfg["ranks"], ic.table_size(cfg)
    vals = ic.out_of_table(cfg).tolist()
    assert {T, T + 1} <= set(vals) and set(range(T, T + 2 * R)) <= set(vals)
    assert {63, 64, 127, 128, 255, 256, 1000, 2 ** 31 - 1, -1, -2, -5, -2 ** 31} <= set(vals)
    assert all(-2 ** 31 <= v < 2 ** 31 and (v < 0 or v >= T) for v in vals)
    rank, to_self = ic.reference_hint(cfg, np.arange(T, T + 2 * R))
    assert rank.tolist() == list(range(R)) * 2 and to_self.tolist() == [1] * R + [0] * R  # u / R = 1, then 2
    rank, to_self = ic.reference_hint(cfg, np.array([-1]))
    u = 2 ** 32 - 1 - 10 - K
    assert (int(rank[0]), int(to_self[0])) == (u % R, (u // R) % 2)
    if name == "full":
        assert sorted(v for v in vals if 20 <= v < 30) == list(range(20, 30))


@pytest.mark.parametrize("name", ic.WALK_CONFIGS)
def test_walk_reaches_every_class_inside_the_domain(name, oracle_lib):
    cfg = ic.config_of(name)
    max_info = cfg["max_information_tokens"]
    orc = oracle_lib.HanabiOracle(cfg, ic.WORLDS, num_threads=4)
    w = np.arange(ic.WORLDS)
    total = {}
    for t, rec, acts, cls in ic.walk(orc, cfg):
        mover = rec[:, 83].astype(np.int64)
        uid = acts[mover, w].astype(np.int64)
        info, size = rec[:, 81].astype(np.int64), rec[w, 105 + 36 * mover]
        # the domain before every step: tokens in [0, max + e], hands of 4..5 cards, the mover's hand full
        assert ((info >= 0) & (info <= max_info + ic.MAX_EXCESS)).all(), f"step {t}: tokens {info.max()}"
        assert np.isin(rec[:, 105], (4, 5)).all() and np.isin(rec[:, 141], (4, 5)).all() and (size == 5).all()
        # each class is what it says
        a, b, e = cls == ic.A, cls == ic.B, cls == ic.E
        assert ((uid[a] >= 10) & (uid[a] < ic.table_size(cfg)) & (info[a] > 0)).all()
        assert ((uid[b] >= 0) & (uid[b] < 5) & (info[b] >= max_info) & (info[b] + 1 <= max_info + ic.B_EXCESS)).all()
        assert (((uid[e] >= ic.table_size(cfg)) | (uid[e] < 0)) & (info[e] > 0)).all()
        assert not (cls == ic.Z).any()
        assert ((uid < 10) | (info > 0)).all(), "a hint at zero tokens (class Z) must never reach the oracle"
        for k, v in ic.count_classes(cfg, rec, acts, cls, orc.done).items():
            total[k] = total.get(k, 0) + v
    after = orc.dump()[:, 81].astype(np.int64)
    assert (after <= max_info + ic.MAX_EXCESS).all()
    print(f"hanabi {name}: {ic.WORLDS} worlds x {ic.STEPS} steps: {total}")
    for k in AT_LEAST_100:
        assert not ic.reachable(name, k) or total[k] >= MIN_COUNT, f"{name}: class {k} occurred {total[k]} times"
    for k in AT_LEAST_1:
        assert not ic.reachable(name, k) or total[k] >= 1, f"{name}: '{k}' never occurred ({total})"
    assert ic.B_EXCESS <= ic.MAX_EXCESS <= 64  # inside the reference stand-in's 64-byte guard zones and the encoders' shift


@pytest.mark.parametrize("name", ic.WALK_CONFIGS)
def test_illegal_classes_are_forbidden_by_the_mask(name, oracle_lib):
    """A and B are in-table moves whose mask entry is 0; L moves have it set."""
    cfg = ic.config_of(name)
    orc = oracle_lib.HanabiOracle(cfg, ic.WORLDS, num_threads=4)
    w = np.arange(ic.WORLDS)
    rng = np.random.default_rng(7)
    for _ in range(20):
        rec, mask = orc.dump(), orc.mask.copy()
        acts, cls = ic.choose_with_illegal(rng, cfg, mask, rec)
        mover = rec[:, 83].astype(np.int64)
        uid = acts[mover, w].astype(np.int64)
        inside = (cls != ic.E)
        allowed = mask[mover[inside], w[inside], uid[inside]] != 0
        assert (allowed == (cls[inside] == ic.L)).all()
        orc.step(acts)


@pytest.mark.parametrize("name", ic.WALK_CONFIGS)
def test_mapped_action_against_the_reference_behaviour(name, oracle_lib):
    """The library's departure from the reference, made visible: the oracle (pinned to the reference on these values by
    test_ref_hanabi.py and the fixtures) fed an out-of-table action and fed mapped_action of it.  With u / R even the two
    are the same step, bit for bit; with u / R odd the reference hints the mover's own hand, the mapped action the partner:
    same rank, same token spent, another target byte in the record (and other knowledge)."""
    cfg = ic.config_of(name)
    K, R, T = cfg["colors"], cfg["ranks"], ic.table_size(cfg)
    pool = ic.out_of_table(cfg)
    n = len(pool)
    mapped = ic.mapped_action(cfg, pool)
    rank, to_self = ic.reference_hint(cfg, pool)
    assert ((mapped >= 10 + K) & (mapped < T)).all() and np.array_equal(mapped - 10 - K, rank)
    assert set(to_self.tolist()) == {0, 1}
    inside = np.arange(-3, T + 3)
    keep = (inside >= 0) & (inside < T)
    assert np.array_equal(ic.mapped_action(cfg, inside)[keep], inside[keep])            # every in-table value stays
    by_hand = [10 + K + ((v - 10 - K) % (1 << 32)) % R for v in pool.tolist()]           # Python integers, no numpy
    assert mapped.tolist() == by_hand
    raw, fed = oracle_lib.HanabiOracle(cfg, n), oracle_lib.HanabiOracle(cfg, n)
    raw.step(np.stack([pool, pool]).astype(np.int32))                                    # world i makes move pool[i] first
    fed.step(np.stack([mapped, mapped]))
    a, b = raw.dump(), fed.dump()
    even, odd = to_self == 0, to_self == 1
    assert np.array_equal(a[even], b[even]) and np.array_equal(raw.state[:, even], fed.state[:, even])
    assert (a[odd, 89] == 0).all() and (b[odd, 89] == 1).all()                           # target: the mover (0) / the partner (1)
    assert np.array_equal(a[odd, 81], b[odd, 81]) and np.array_equal(a[odd, 94], b[odd, 94])  # tokens, hinted rank
    assert np.array_equal(raw.mask, fed.mask) and np.array_equal(raw.done, fed.done)
