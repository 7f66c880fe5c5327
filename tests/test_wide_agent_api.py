"""CPU: the public surface of the device-side CleanPPOAgent collection phase (mrl_agent_act, mrl_agent_credit,
mrl_gae_active; WidePolicy; CleanPPOAgent) and the yardsticks tests/test_gpu_wide_agent.py measures against: the float64 twin
against torch float32, the draws of the GPU cases, and the reference's own advantage pass and reward bookkeeping
(tests/golden/cleanppo_gae.npz, recorded from the reference's class by tests/golden/make_cleanppo_golden.py)."""
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from conftest import load_golden

import hanabi_configs
import wide_twin as twin

NEW_SYMBOLS = ["mrl_wide_policy_num_params", "mrl_agent_workspace_bytes", "mrl_agent_act", "mrl_agent_credit", "mrl_gae_active"]


def reference_shaped_network(d, s, a):
    """a network of the reference's CleanRLNetwork shape, built here from torch alone"""
    nn = torch.nn

    def net(inputs, outputs):
        return nn.Sequential(nn.Linear(inputs, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU(), nn.Linear(512, 512), nn.ReLU(),
                             nn.Linear(512, outputs))

    module = nn.Module()
    module.critic = net(s, 1)
    module.actor = net(d, a)
    return module


def test_symbols(hip_lib):
    from madrona_rl_envs_playground_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.mrl_abi_version() == 4


@pytest.mark.parametrize("d,s,a", [(7, 7, 4), (658, 783, 20), (1, 1, 1), (3, 9, 64)])
def test_parameter_count_and_order(d, s, a, hip_lib):
    from madrona_rl_envs_playground_amd.simulators import WidePolicy
    torch.manual_seed(d)
    network = reference_shaped_network(d, s, a)
    vector = torch.nn.utils.parameters_to_vector(network.parameters()).detach()
    assert hip_lib.mrl_wide_policy_num_params(d, s, a) == vector.numel()
    policy = WidePolicy.from_module(network, device="cpu")
    assert policy.num_params == vector.numel() and (policy.obs_dim, policy.state_dim, policy.num_actions) == (d, s, a)
    assert torch.equal(policy.params, vector)
    # the order by name: the critic's first weight leads, the actor's last bias ends
    assert torch.equal(policy.params[:512 * s].view(512, s), network.critic[0].weight.detach())
    assert torch.equal(policy.params[-a:], network.actor[6].bias.detach())
    assert hip_lib.mrl_agent_workspace_bytes(33) >= 33 * (4 + 2 * 2 * 512 * 4 + 64 * 4 + 4)


def test_policy_shape_refusals(hip_lib):
    from madrona_rl_envs_playground_amd.simulators import WidePolicy
    with pytest.raises(ValueError):
        WidePolicy(7, 7, 65, device="cpu")
    with pytest.raises(ValueError):
        WidePolicy(0, 7, 4, device="cpu")
    narrow = reference_shaped_network(7, 7, 4)
    narrow.actor[2] = torch.nn.Linear(512, 256)
    with pytest.raises(ValueError):
        WidePolicy.from_module(narrow, device="cpu")
    assert not hasattr(WidePolicy, "load_")


def test_module_parameters_are_views_of_params(hip_lib):
    from madrona_rl_envs_playground_amd.simulators import WidePolicy
    torch.manual_seed(5)
    policy = WidePolicy.from_module(reference_shaped_network(7, 9, 4), device="cpu")
    module = policy.module()
    assert policy.module() is module
    storage = policy.params.untyped_storage().data_ptr()
    at = policy.params.data_ptr()
    for p in module.parameters():
        assert p.untyped_storage().data_ptr() == storage and p.data_ptr() == at
        at += 4 * p.numel()
    assert at == policy.params.data_ptr() + 4 * policy.params.numel()
    before = policy.params.clone()
    optimizer = torch.optim.Adam(module.parameters(), lr=1e-2, eps=1e-5)
    x = torch.ones(3, 7)
    state = torch.ones(3, 9)
    _, logp, _, value = module.get_action_and_value(x, state, torch.ones(3, 4, dtype=torch.bool), torch.zeros(3, dtype=torch.long))
    (logp.sum() + value.sum()).backward()
    optimizer.step()
    assert not torch.equal(policy.params, before)  # the optimizer's in-place step is what the kernels read next
    assert torch.equal(policy.params, torch.nn.utils.parameters_to_vector(module.parameters()).detach())


def test_draws_lie_on_the_24_bit_grid():
    u = twin.draws(12345, 7, 4096, 1)
    assert np.all(u >= 0) and np.all(u < 1) and np.all(u * 2 ** 24 == np.floor(u * 2 ** 24))
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert not np.array_equal(u, twin.draws(12345, 7, 4096, 0)) and not np.array_equal(u, twin.draws(12345, 8, 4096, 1))


@pytest.mark.parametrize("weights", sorted(twin.WEIGHTS))
@pytest.mark.parametrize("game", ["balance", "hanabi_very_small", "hanabi_full"] + [game for game, _ in twin.CONFIG_CASES])
def test_twin_against_torch_float32(game, weights):
    """The twin and torch's float32 evaluation are the same function: their distance d is a float32 rounding distance (the
    bound: K <= 783 terms of size <= |x w| each rounded to 2^-24 relative, four layers), and away from the boundaries they
    choose the same actions."""
    agent = twin.make_agent(game, weights)
    inputs = twin.case_inputs(game, 65, twin.case_seed(game, 65, weights))
    d_value, d_logp = twin.margins(agent, inputs)
    print(f"{game} {weights}: d_value {d_value:.3e} d_logp {d_logp:.3e}")
    assert 0 < d_value < 1e-4 and 0 < d_logp < 1e-3
    u = twin.draws(1, 0, 65, 0)
    out = twin.act(twin.flat(agent), inputs["obs"], inputs["state"], inputs["mask"], u)
    _, lp32 = twin.torch_forward32(agent, inputs["obs"], inputs["state"], inputs["mask"])
    cdf32 = np.cumsum(np.exp(lp32), axis=1)[:, :-1]
    actions32 = (u[:, None] >= cdf32).sum(axis=1)
    keep = ~twin.near_boundary(out["cdf"], u)
    assert np.array_equal(actions32[keep], out["actions"][keep])
    legal = inputs["mask"] != 0
    assert legal[np.arange(65), out["actions"]].all() and legal[np.arange(65), out["greedy"]].all()
    assert np.isneginf(out["logp"][~legal]).all()


@pytest.mark.parametrize("weights", sorted(twin.WEIGHTS))
@pytest.mark.parametrize("game,n", twin.CASES + twin.CONFIG_CASES)
def test_gpu_cases_draw_away_from_boundaries(game, n, weights):
    """The rows a GPU action comparison may skip: at most 1 % of a case's rows lie within 1e-5 of a boundary -- with the draws of
    the seat the GPU case acts as, n % 2, and for the named games with those of seat 0 as well."""
    seed = twin.case_seed(game, n, weights)
    agent = twin.make_agent(game, weights)
    inputs = twin.case_inputs(game, n, seed)
    for player in sorted({0, n % 2} if (game, n) in twin.CASES else {n % 2}):
        u = twin.draws(seed, 0, n, player)
        near = twin.near_boundary(twin.act(twin.flat(agent), inputs["obs"], inputs["state"], inputs["mask"], u)["cdf"], u)
        assert near.sum() <= 0.01 * n, f"seat {player}: {near.sum()} of {n} rows are near a boundary"


@pytest.mark.parametrize("weights", sorted(twin.WEIGHTS))
@pytest.mark.parametrize("game,n,player,step", twin.LARGE_CASES)
def test_large_gpu_cases_draw_away_from_boundaries(game, n, player, step, weights):
    """The same cap for the cases past 1024 worlds, at the player and the step they run with."""
    seed = twin.case_seed(game, n, weights)
    agent = twin.make_agent(game, weights)
    inputs = twin.case_inputs(game, n, seed)
    u = twin.draws(seed, step, n, player)
    assert not np.array_equal(u, twin.draws(seed, 0, n, player))  # (the step reaches the draw)
    near = twin.near_boundary(twin.act(twin.flat(agent), inputs["obs"], inputs["state"], inputs["mask"], u)["cdf"], u)
    print(f"{game} n={n} {weights}: {near.sum()} of {n} rows are near a boundary")
    assert near.sum() <= 0.01 * n, f"{near.sum()} of {n} rows are near a boundary"


@pytest.mark.parametrize("kind", sorted(twin.EDGE_DRAWS))
def test_edge_draws_sit_at_the_ends_of_the_grid(kind):
    assert len(twin.EDGE_DRAWS[kind]) == 6
    for seed, player, world in twin.EDGE_DRAWS[kind]:
        assert twin.draws(seed, 0, twin.EDGE_N, player)[world] == twin.EDGE_U[kind], (seed, player, world)
    assert twin.EDGE_U["top"] == np.nextafter(np.float32(1.0), np.float32(0.0))  # the largest u there is


def test_edge_rows_are_decided_by_the_ends_of_the_grid():
    """What the GPU's edge-draw test rests on.  Top draws: the twin chooses the last legal action, with a probability far
    above the grid's spacing (so the boundary below it is nowhere near u); the row is one the general comparison skips; and a
    float32 cumulative sum without the fallback runs on into the illegal tail in some of the rows (which ones depends on the
    rounding: evidence that the device takes the branch, not proof).  Zero draws: the three empty boundaries are passed
    (0 >= 0) and the first legal action, 3, is chosen."""
    agent = twin.make_agent(twin.EDGE_GAME, "orthogonal")
    params = twin.flat(agent)
    rows = twin.edge_rows()
    assert [r[0] for r in rows].count("top") == 48 and [r[0] for r in rows].count("zero") == 6
    illegal, lowest = 0, 1.0
    for kind, seed, player, world, variant, want in rows:
        inputs = twin.edge_inputs(kind, seed, world, variant)
        legal = inputs["mask"] != 0
        u = twin.draws(seed, 0, twin.EDGE_N, player)
        out = twin.act(params, inputs["obs"], inputs["state"], inputs["mask"], u)
        assert out["actions"][world] == want and legal[world, want], (kind, seed, variant)
        if kind == "zero":
            assert not legal[world, :3].any()
            continue
        assert want == np.flatnonzero(legal[world]).max() and not legal[world, want + 1:].any() and not legal[world, 0]
        lowest = min(lowest, float(np.exp(out["logp"][world, want])))
        assert twin.near_boundary(out["cdf"], u)[world]
        raw = twin.head32(out["logits"].astype(np.float32)[world:world + 1], inputs["mask"][world:world + 1], u[world:world + 1])[0]
        assert raw >= want
        illegal += not legal[world, raw]
    print(f"top draws: the raw float32 count is illegal in {illegal} of 48 rows; the last legal action's probability >= {lowest:.3f}")
    assert lowest >= 1e-3
    assert illegal >= 1


@pytest.mark.parametrize("game,d,s,a", twin.NARROW_CASES)
def test_narrow_integer_policies_are_exact_in_float32(game, d, s, a):
    """The narrow-policy GPU cases compare bit for bit: every sum of absolute terms stays below 2^24, the logits are not all
    alike, and in the tied case the tie is there and is the largest logit of some worlds."""
    full = twin.dims(game)
    assert d < full[0] and s < full[1] and a <= full[2]
    tie = twin.TIE if a == 15 else None
    layers = twin.integer_layers(d, s, a, tie=tie)
    inputs = twin.narrow_inputs(twin.case_inputs(game, twin.NARROW_N, 4242), d, s, a)
    values, logits, bound = twin.integer_forward(layers, inputs["obs"], inputs["state"])
    assert bound < 2 ** 24
    assert len(np.unique(logits)) > 1 and len(np.unique(values)) > 1
    reference = twin.forward(twin.integer_params(layers), inputs["obs"], inputs["state"], a)
    assert np.array_equal(reference[0], values) and np.array_equal(reference[1], logits)  # the flat order is the twin's
    if tie:
        lo, hi = tie
        assert np.array_equal(logits[:, lo], logits[:, hi])
        assert ((logits <= logits[:, [lo]]).sum(axis=1) > 2).any()


# ---------------------------------------------------------------- every Hanabi configuration of tests/hanabi_configs.py

# id: (D, S, A, code variant, deck); D = 21 K R + 11 K + 11 R + 12 + information + life, S = D + 5 K R, A = 10 + K + R
CONFIG_TABLE = {
    "k3r5i8l3": (426, 501, 18, 1, 20), "k4r5i5l2": (538, 638, 19, 1, 30), "k5r4i8l3": (542, 642, 19, 0, 30), "k5r3i8l3": (426, 501, 18, 0, 20),
    "k5r2i8l3": (310, 360, 17, 0, 10), "k3r3i4l2": (273, 318, 16, 0, 8), "k2r4i1l1": (248, 288, 16, 0, 6), "k4r2i2l3": (251, 291, 16, 0, 6),
    "k3r2i1l1": (195, 225, 15, 0, 2), "k2r3i8l3": (204, 234, 15, 0, 2), "k1r5i1l1": (185, 210, 16, 1, 0), "k4r4i7l2": (445, 525, 18, 0, 22),
    "k5r5i1l3": (651, 776, 20, 1, 40), "k2r3i3l1": (197, 227, 15, 0, 2),
}


def test_config_table_and_its_spread():
    """(D, S, A), variant and deck of every configuration as literals, and what the list brings to the act kernels -- asserted so
    that an edit of ``hanabi_configs.CONFIGS`` cannot lose it."""
    from madrona_rl_envs_playground_amd import hanabi_spec
    assert list(CONFIG_TABLE) == hanabi_configs.IDS == [game[len("hanabi_"):] for game, _ in twin.CONFIG_CASES]
    assert all(n == 65 for _, n in twin.CONFIG_CASES)
    for cid, (d, s, a, variant, deck) in CONFIG_TABLE.items():
        cfg = hanabi_configs.BY_ID[cid]
        k, r = cfg["colors"], cfg["ranks"]
        assert (hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg), hanabi_spec.num_moves(cfg)) == (d, s, a) == twin.dims("hanabi_" + cid)
        assert d == 21 * k * r + 11 * k + 11 * r + 12 + cfg["max_information_tokens"] + cfg["max_life_tokens"]
        assert s == d + 5 * k * r and a == 10 + k + r
        assert hanabi_configs.variant(cfg) == variant and hanabi_configs.deck_size(cfg) == deck
    rows = list(CONFIG_TABLE.values())
    assert {a for _, _, a, _, _ in rows} == set(range(15, 21))
    assert [cid for cid, row in CONFIG_TABLE.items() if row[2] == 20] == ["k5r5i1l3"]  # A = 20 on a game that is not the full one
    assert {variant for _, _, _, variant, _ in rows} == {0, 1}
    tails = {w % 64 for d, s, _, _, _ in rows for w in (d, s)}  # the last k-chunk of a first layer
    assert {2, 3, 5, 32, 62} <= tails
    assert any(w % 2 for d, s, _, _, _ in rows for w in (d, s)) and any(d % 4 for d, _, _, _, _ in rows) and any(s % 4 for _, s, _, _, _ in rows)
    assert {0, 2} <= {deck for _, _, _, _, deck in rows}
    # the named games keep their seeds, the configurations get their own
    assert [twin.case_seed(g, 65, "orthogonal") for g in ("balance", "hanabi_very_small", "hanabi_full")] == [514736, 514737, 514738]
    assert twin.case_seed("hanabi_k3r5i8l3", 65, "orthogonal") == 7919 * 65 + 10
    assert twin.case_seed("hanabi_k2r3i3l1", 65, "peaked") == 7919 * 65 + 104729 + 10 + 13


@pytest.mark.parametrize("game,n", twin.CONFIG_CASES)
def test_config_margins_pool_three_input_sets(game, n):
    """d of a configuration is the largest of three sets' distances, each a float32 rounding distance of the size the named
    games have."""
    for weights in sorted(twin.WEIGHTS):
        agent, seed = twin.make_agent(game, weights), twin.case_seed(game, n, weights)
        per_set = [twin.margins(agent, twin.case_inputs(game, n, seed + 1000003 * k)) for k in range(3)]
        d_value, d_logp = twin.config_margins(game, weights)
        print(f"{game} {weights}: d_value {d_value:.3e} d_logp {d_logp:.3e}; per set {per_set}")
        assert d_value == max(m[0] for m in per_set) and d_logp == max(m[1] for m in per_set)
        assert 1e-9 < d_value < 5e-8 and 1e-7 < d_logp < 1e-5


@pytest.mark.parametrize("game,n", twin.CONFIG_CASES)
def test_integer_policies_of_every_configuration_are_exact_in_float32(game, n):
    """The operand-map GPU cases compare bit for bit: every sum of absolute terms stays below 2^24 and the logits are not all alike."""
    d, s, a = twin.dims(game)
    layers = twin.integer_layers(d, s, a)
    inputs = twin.case_inputs(game, n, twin.INTEGER_SEED)
    values, logits, bound = twin.integer_forward(layers, inputs["obs"], inputs["state"])
    print(f"{game}: the largest sum of absolute terms is {bound:.3e}")
    assert bound < 2 ** 24
    assert len(np.unique(logits)) > n and logits.std(axis=0).min() > 0 and logits.std(axis=1).min() > 0 and len(np.unique(values)) > 1
    reference = twin.forward(twin.integer_params(layers), inputs["obs"], inputs["state"], a)
    assert np.array_equal(reference[0], values) and np.array_equal(reference[1], logits)  # the flat order is the twin's


# episodes ended in the committed walk of each configuration (65 worlds, 24 steps, twin.WALK_SEEDS)
WALK_EPISODES = {"k1r5i1l1": 952, "k3r2i1l1": 407, "k2r4i1l1": 521, "k5r4i8l3": 93, "k4r5i5l2": 118, "k5r5i1l3": 177}


@pytest.mark.parametrize("cid", sorted(twin.WALK_SEEDS))
def test_config_walk_reaches_what_the_gpu_test_relies_on(cid, oracle_lib):
    """Conditions on the closed loop of tests/test_gpu_wide_agent_configs.py, walked here by the oracle and the twin alone."""
    assert sorted(twin.WALK_SEEDS) == sorted(WALK_EPISODES) and (twin.WALK_N, twin.WALK_STEPS) == (65, 24)
    game = "hanabi_" + cid
    d, s, a = twin.dims(game)
    steps = twin.walked(cid)
    assert len(steps) == twin.WALK_STEPS
    near = rows = empty = ended = 0
    chosen = np.zeros(a, np.int64)
    d_value = d_logp = 0.0
    for t, step in enumerate(steps):
        assert not step["before"]["mask"][..., a:].any() and not step["after"]["mask"][..., a:].any(), f"step {t}: a legal move beyond {a}"
        assert ((step["before"]["active"] != 0).sum(axis=0) == 1).all()  # one seat is the one to act
        ended += int(step["after"]["done"].sum())
        for p, seat in enumerate(step["seats"]):
            active = seat["active"]
            assert (step["actions"][p][~active] == 0).all()
            if not active.any():
                empty += 1
                continue
            legal = step["before"]["mask"][p][active, :a] != 0
            assert legal[np.arange(active.sum()), seat["twin"]["actions"]].all()
            assert np.array_equal(step["actions"][p][active], seat["twin"]["actions"])
            rows += int(active.sum())
            near += int(twin.near_boundary(seat["twin"]["cdf"], seat["u"]).sum())
            chosen += np.bincount(seat["twin"]["actions"], minlength=a)
            d_value, d_logp = max(d_value, seat["d"][0]), max(d_logp, seat["d"][1])
    print(f"{cid}: {rows} active rows, {near} near a boundary, {ended} episodes ended, {empty} seat-steps without an active world, "
          f"d_value {d_value:.3e} d_logp {d_logp:.3e}, actions chosen {chosen.tolist()}")
    assert rows == twin.WALK_N * twin.WALK_STEPS
    assert near == 0, f"{near} active rows lie within 1e-5 of a boundary: choose another seed"
    assert (chosen > 0).all(), f"actions never chosen: {np.flatnonzero(chosen == 0).tolist()}"
    assert empty >= 1 and not steps[0]["seats"][1]["active"].any()  # seat 1 at step 0: an act over an empty world list
    assert ended >= max(50, WALK_EPISODES[cid] / 2)
    assert 0 < d_value < 1e-4 and 0 < d_logp < 1e-3


@pytest.mark.parametrize("game,n,seed", twin.LIVE_CASES)
def test_live_walk_reaches_what_the_gpu_test_relies_on(game, n, seed, oracle_lib):
    """Conditions on the closed loop of tests/test_gpu_wide_agent_live.py, walked here by the oracle and the twin alone (the
    device's own walk differs from this one only behind a row it decided otherwise, and asserts the near-boundary cap again):
    few rows near a boundary, episodes that end in several 1024-world blocks of the totals in the same step, world lists whose
    length changes from step to step and lies on either side of one pass of 1024, no tie among a row's largest logits (so the
    first-arg-max rule of GREEDY decides nothing), and an advantage pass that is coupled across its workgroups."""
    assert [(g, m) for g, m, _ in twin.LIVE_CASES] == [(g, 2081) for g in ("hanabi_k1r5i1l1", "hanabi_k5r4i8l3", "hanabi_k2r4i1l1", "balance")]
    assert twin.LIVE_STEPS == 12 and twin.NEAR_CAP == 0.001
    d, s, a = twin.dims(game)
    blocks = range(0, n, 1024)
    near = rows = ended = ties = 0
    together = one_idle = False
    counts, either_side = [[], []], False
    activity = np.zeros((2, twin.LIVE_STEPS, n), bool)
    for t, step in enumerate(twin.twin_walk(game, n, twin.LIVE_STEPS, seed)):
        done = step["after"]["done"] != 0
        per_block = [int(done[b:b + 1024].sum()) for b in blocks]
        ended += int(done.sum())
        together |= sum(c > 0 for c in per_block) >= 2
        one_idle |= min(per_block) == 0 < max(per_block)
        for p, seat in enumerate(step["seats"]):
            active = activity[p, t] = seat["active"]
            assert (step["actions"][p][~active] == 0).all()
            counts[p].append(int(active.sum()))
            if not active.any():
                continue
            either_side |= counts[p][-1] > 1024 and bool(active[:1024].any() and active[1024:].any())
            legal = step["before"]["mask"][p][active, :a] != 0
            assert legal[np.arange(active.sum()), seat["twin"]["actions"]].all()
            rows += counts[p][-1]
            near += int(twin.near_boundary(seat["twin"]["cdf"], seat["u"]).sum())
            top = np.sort(np.where(legal, seat["twin"]["logits"], -np.inf), axis=1)[:, -2:]
            ties += int((top[:, 0] == top[:, 1]).sum())
            assert 0 < seat["d"][0] < 1e-4 and 0 < seat["d"][1] < 1e-3
    coupled = [twin.coupled_across_workgroups(activity[p], step["after"]["active"][p]) for p in range(2)]
    print(f"{game}: {rows} active rows, {near} near a boundary, {ended} episodes ended, list lengths {counts}, coupled advantage pass "
          f"of the seats {coupled}")
    assert near <= twin.NEAR_CAP * rows, f"{near} of {rows} active rows lie within 1e-5 of a boundary: choose another seed"
    assert together, "no step ends episodes in two blocks of the totals at once"
    assert ended >= 50
    assert ties == 0, f"{ties} rows whose two largest legal logits tie"
    if game == "balance":
        assert counts == [[n] * twin.LIVE_STEPS] * 2 and coupled == [False, False]  # every row of both seats: nothing to wait for
        return
    assert any(len(set(c)) >= 3 and max(c) > 1024 > min(c) for c in counts) and either_side
    assert any(coupled), "t* never lies below a workgroup's own least row"
    if game == "hanabi_k5r4i8l3":
        assert one_idle, "no step in which one block ends episodes and another ends none"


FIXTURE_CASES = [(regime, n) for n in (5, 70) for regime in ("coupled", "together")]


def fixture_case(regime, n):
    g = load_golden("cleanppo_gae.npz")
    return {k[len(f"{regime}_{n}_"):]: v for k, v in g.items() if k.startswith(f"{regime}_{n}_")}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("regime,n", FIXTURE_CASES)
def test_advantage_pass_equals_the_reference_bit_for_bit(regime, n):
    f = fixture_case(regime, n)
    num_steps = f["before_active"].shape[0]
    assert num_steps == 8
    adv, ret, active = twin.gae_active(f["before_rewards"], f["before_values"], f["before_dones"], f["before_active"],
                                       f["before_next_done"], f["next_value"], f["activity"][num_steps], float(f["gamma"]),
                                       float(f["gae_lambda"]))
    assert same_bits(adv, f["advantages"]) and same_bits(ret, f["returns"])
    assert np.array_equal(active, f["active_after"])
    # the fixture holds the regime it claims: the coupling acts below T - 1, or not at all
    boot = f["activity"][num_steps]
    first = np.where(boot, num_steps, np.where(f["before_active"].any(axis=0),
                                               num_steps - 1 - f["before_active"][::-1].argmax(axis=0), -1))
    if regime == "coupled":
        assert 0 <= first.min() < num_steps - 1 and boot.any() and not boot.all()
        skipped = f["before_active"] & f["active_after"] & (f["advantages"] == 0) & (np.arange(num_steps)[:, None] >= first.min())
        assert skipped.any()  # an already bootstrapped, active world was left at 0
        assert (f["before_active"] != f["active_after"]).any()
    else:
        assert first.min() == num_steps and np.array_equal(f["before_active"], f["active_after"])
    assert f["dones_in"].any()  # episode ends


@pytest.mark.parametrize("regime,n", FIXTURE_CASES)
def test_credit_step_equals_the_reference(regime, n):
    """The per-world arrays after every update() bit for bit, and the reward buffer in every cell (last_active[w], w).  The other
    cells differ on purpose: the reference's indexed add selects whole rows (include/mrl_envs.h, mrl_agent_credit)."""
    f = fixture_case(regime, n)
    rec = twin.new_record(8, n)
    worlds = np.arange(n)
    for t in range(8):
        twin.book(rec, t, f["activity"][t])
        twin.credit(rec, f["rewards_in"][t], f["dones_in"][t])
        assert same_bits(rec["running_rewards"], f["trace_running_rewards"][t])
        for name in ("next_done", "new_game", "last_active"):
            assert np.array_equal(rec[name].astype(np.int64), f["trace_" + name][t].astype(np.int64)), name
        own = rec["last_active"]
        assert same_bits(rec["rewards"][own, worlds], f["trace_rewards"][t][own, worlds])
    assert same_bits(rec["dones"], f["before_dones"]) and np.array_equal(rec["active"] != 0, f["before_active"])
    if regime == "together":
        assert same_bits(rec["rewards"], f["before_rewards"])
    finished = f["dones_in"].sum()
    assert rec["totals"][:, 0].sum() == finished


def reference_signature():
    """names and defaults of the reference's CleanPPOAgent.__init__ (pantheonrl_extension/vectoragent.py:117-136)"""
    return [("envs", None), ("name", None), ("device", None), ("num_updates", None), ("verbose", True), ("lr", 2.5e-4), ("num_steps", 128),
            ("anneal_lr", True), ("gamma", 0.99), ("gae_lambda", 0.95), ("num_minibatches", 4), ("update_epochs", 4), ("norm_adv", True),
            ("clip_coef", 0.2), ("clip_vloss", True), ("ent_coef", 0.01), ("vf_coef", 0.5), ("max_grad_norm", 0.5), ("target_kl", None)]


def test_agent_signature_and_refusal_of_other_envs(hip_lib):
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent, VectorAgent
    from madrona_rl_envs_playground_amd.pantheonrl_extension.vectorobservation import VectorObservation
    parameters = list(inspect.signature(CleanPPOAgent.__init__).parameters.values())[1:]
    for got, (name, default) in zip(parameters, reference_signature()):
        assert got.name == name
        assert got.default == default if name not in ("envs", "name", "device", "num_updates") else got.default is inspect.Parameter.empty
    assert [p.name for p in parameters[len(reference_signature()):]] == ["seed"]
    assert issubclass(CleanPPOAgent, VectorAgent)
    space = SimpleNamespace(shape=(7,))
    envs = SimpleNamespace(num_envs=3, observation_space=space, share_observation_space=space, action_space=SimpleNamespace(n=4, shape=()),
                           ego_ind=0)
    agent = CleanPPOAgent(envs, "stub", torch.device("cpu"), num_updates=1, verbose=False, num_steps=4)
    assert agent.policy.params.numel() == hip_lib.mrl_wide_policy_num_params(7, 7, 4)
    assert agent.seed == CleanPPOAgent(envs, "stub", torch.device("cpu"), num_updates=1, verbose=False).seed  # derived from the name
    assert CleanPPOAgent(envs, "stub", "cpu", 1, verbose=False, seed=9).seed == 9
    x = torch.zeros(3, 7)
    with pytest.raises(TypeError, match="MadronaEnv"):
        agent.get_action(VectorObservation(torch.ones(3, dtype=torch.bool), x, x, torch.ones(3, 4, dtype=torch.bool)))
    with pytest.raises(TypeError, match="MadronaEnv"):
        agent.update(torch.zeros(3), torch.zeros(3))
