"""GPU: the wide policy's bank -- ``mrl_agent_act_bank``, ``mrl_agent_bank_resample``, ``WidePolicyAgent``,
``WidePopulationAgent`` and ``cross_play`` with a ``WidePolicyBank`` -- on Hanabi ``very_small`` and the balance beam.

Every comparison is exact.  The reference of every bank output is the plain act (``mrl_agent_act``) of this same library under the
world's policy alone, which tests/test_gpu_wide_agent*.py pin to the oracle and the twin; the reference of the resample is
``resample_twin``.  The games are live: a few random steps in, so the movers differ from world to world."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wide_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib, layouts  # noqa: E402
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.envs.hanabi_env import VERY_SMALL_CONFIG, HanabiMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.pantheonrl_extension import WidePolicyAgent, WidePopulationAgent  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (ExecMode, OvercookedSimulator, WideOptimizer, WidePolicy, WidePolicyBank,  # noqa: E402
                                                         agent_act, agent_act_bank, agent_bank_workspace_bytes, cross_play,
                                                         resample_twin, wide_resample)
from test_gpu_wide_agent import DEV, cpu, make_sim, same_bits  # noqa: E402

GAMES = ("hanabi_very_small", "balance")
MARK, ROW_MARK = -7, -9  # what ACTION and ids_row hold in front of a call
K = 5
WARM_STEPS = 9


def up(x, to):
    return (x + to - 1) // to * to


def make_bank(game, k):
    """k policies of the game's shape that play differently: the "peaked" weights of the forward tests under k seeds"""
    return WidePolicyBank.from_policies([WidePolicy.from_module(twin.make_agent(game, "peaked", seed=100 + j), device=DEV) for j in range(k)])


def warm_sim(game, n, seed=5):
    sim = make_sim(game, n)
    sim.rollout_random(WARM_STEPS, seed=seed)
    torch.cuda.synchronize()
    return sim


class Layout:
    """byte offsets of include/mrl_envs.h's workspace of mrl_agent_act_bank"""

    def __init__(self, n, k):
        self.n, self.k = n, k
        self.act_bytes = int(_lib.lib().mrl_agent_workspace_bytes(n))
        self.logits = up(4 * n, 256) + 256 + 2 * (2 * n * 512 * 4)
        self.values = self.logits + n * 64 * 4
        self.eff = self.act_bytes
        self.plan = self.act_bytes + up(4 * n, 256)
        self.kp, self.max_tiles = up(k, 4), (n + 31) // 32 + k
        self.count, self.start, self.table = 4, 4 + self.kp, 4 + 2 * self.kp
        self.lists = self.table + 4 * self.max_tiles
        self.total = agent_bank_workspace_bytes(n, k)

    def floats(self, ws, at, count):
        return ws[at:at + 4 * count].view(np.float32)

    def read(self, ws):
        """the plan's words and the logits and values by list position"""
        words = ws[self.plan:self.total].view(np.uint32)
        tiles, acted, out_of_range = (int(x) for x in words[:3])
        return {"tiles": tiles, "acted": acted, "out_of_range": out_of_range,
                "count": words[self.count:self.count + self.k].astype(np.int64), "start": words[self.start:self.start + self.k].astype(np.int64),
                "table": words[self.table:self.table + 4 * tiles].reshape(tiles, 4).astype(np.int64),
                "lists": words[self.lists:self.lists + acted].astype(np.int64),
                "eff": ws[self.eff:self.eff + 4 * self.n].view(np.int32),
                "logits": self.floats(ws, self.logits, self.n * 64).reshape(self.n, 64)[:acted],
                "values": self.floats(ws, self.values, self.n)[:acted]}


def plain_act(sim, game, player, policy, seed, step, **flags):
    """``agent_act`` without a record on a marked ACTION -> the seat's actions (N), the computed worlds, and their logits (rows, A)
    and values in the order of the world list"""
    n = sim.num_worlds
    a = twin.dims(game)[2]
    ws = torch.zeros(int(_lib.lib().mrl_agent_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    sim.action_tensor().to_torch().fill_(MARK)
    agent_act(sim, player, policy, seed=seed, step=step, workspace=ws, **flags)
    torch.cuda.synchronize()
    host = cpu(ws)
    count = int(host[up(4 * n, 256):up(4 * n, 256) + 4].view(np.uint32)[0])
    worlds = host[:4 * count].view(np.uint32).astype(np.int64)
    lay = Layout(n, 1)
    return {"action": cpu(sim.action_tensor())[player, :, 0], "other": cpu(sim.action_tensor())[1 - player, :, 0], "worlds": worlds,
            "logits": lay.floats(host, lay.logits, n * 64).reshape(n, 64)[:count, :a].copy(), "values": lay.floats(host, lay.values, n)[:count].copy()}


def bank_act(sim, player, bank, ids, seed, step, ids_row=True, workspace=None, **flags):
    """``agent_act_bank`` on a marked ACTION and a zeroed workspace -> ACTION of both seats, ids_row, the workspace's bytes"""
    n = sim.num_worlds
    lay = Layout(n, bank.num_policies)
    ws = torch.zeros(lay.total, dtype=torch.uint8, device=DEV) if workspace is None else workspace
    row = torch.full((n,), ROW_MARK, dtype=torch.int32, device=DEV) if ids_row else None
    sim.action_tensor().to_torch().fill_(MARK)
    agent_act_bank(sim, player, bank, ids, ids_row=row, seed=seed, step=step, workspace=ws, **flags)
    torch.cuda.synchronize()
    actions = cpu(sim.action_tensor())
    return {"action": actions[player, :, 0], "other": actions[1 - player, :, 0], "ids_row": cpu(row) if ids_row else None, "ws": cpu(ws),
            "layout": lay}


# ---------------------------------------------------------------- 1: a bank of one is the plain act

@pytest.mark.parametrize("flags", [{}, {"greedy": True}, {"all_rows": True}, {"greedy": True, "all_rows": True}], ids=lambda f: "+".join(f) or "sampled")
@pytest.mark.parametrize("n", [1, 33, 257])
@pytest.mark.parametrize("game", GAMES)
def test_bank_of_one_equals_the_plain_act(game, n, flags, hip_lib):
    sim = warm_sim(game, n)
    bank = make_bank(game, 1)
    ids = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    active = cpu(sim.active_agent_tensor()).reshape(2, n) != 0
    if game != "balance" and n > 1:
        assert active[0].any() and active[1].any()  # the movers differ from world to world
    for player in (0, 1):
        want = plain_act(sim, game, player, bank.policy(0), 11, 3, **flags)
        got = bank_act(sim, player, bank, ids, 11, 3, **flags)
        same_bits(got["action"], want["action"], f"seat {player}: ACTION")
        assert (got["other"] == MARK).all()
        plan = got["layout"].read(got["ws"])
        computed = np.ones(n, bool) if flags.get("all_rows") else active[player]
        assert np.array_equal(plan["lists"], want["worlds"]) and np.array_equal(want["worlds"], np.flatnonzero(computed))
        same_bits(plan["logits"][:, :want["logits"].shape[1]], want["logits"], f"seat {player}: logits")
        same_bits(plan["values"], want["values"], f"seat {player}: values")
        same_bits(got["ids_row"], np.where(computed, 0, -1).astype(np.int32), f"seat {player}: ids_row")
        assert (got["action"][~computed] == 0).all() and plan["out_of_range"] == 0 and plan["acted"] == computed.sum()
    sim.close()


# ---------------------------------------------------------------- 2 and 3: mixed assignments against K plain acts, the plan

def assignment(name, n):
    w = np.arange(n)
    if name == "robin":
        return w % K
    if name == "one_owner":
        return np.full(n, 3)
    if name == "one_idle":  # policy 4 owns no world
        return w % (K - 1)
    if name == "tile_edges":  # with all_rows: policy 0 exactly 32 worlds, policy 1 exactly 33, policy 2 the rest
        return np.where(w < 32, 0, np.where(w < 65, 1, 2))
    ids = w % K  # "holes": -1 scattered, a few ids beyond the bank
    ids[w % 7 == 3] = -1
    ids[w % 5 == 1] = -(2 + w[w % 5 == 1] % 3)  # any negative value
    ids[w % 11 == 5] = K + w[w % 11 == 5] % 3
    return ids


ASSIGNMENTS = ("robin", "one_owner", "one_idle", "tile_edges", "holes")
MIXED = [("hanabi_very_small", 2081), ("hanabi_very_small", 70), ("balance", 2081), ("balance", 70)]


@functools.lru_cache(maxsize=None)
def mixed_world(game, n):
    """a live simulator, a bank of K and the oracle: the plain act of every member for both seats, with and without all_rows,
    computed once and left unchanged"""
    sim = warm_sim(game, n, seed=6)
    bank = make_bank(game, K)
    plain = {(player, all_rows, k): plain_act(sim, game, player, bank.policy(k), 21, 4, all_rows=all_rows)
             for player in (0, 1) for all_rows in (False, True) for k in range(K)}
    return sim, bank, plain, cpu(sim.active_agent_tensor()).reshape(2, n) != 0


@functools.lru_cache(maxsize=None)
def mixed_case(game, n, name):
    sim, bank, plain, active = mixed_world(game, n)
    all_rows = name == "tile_edges"
    # the two seats' columns differ: seat 1 reads the assignment shifted by one world
    host = np.stack([assignment(name, n), np.roll(assignment(name, n), 1)], axis=1).astype(np.int32)
    ids = torch.from_numpy(host).to(DEV)
    return host, all_rows, [bank_act(sim, player, bank, ids, 21, 4, all_rows=all_rows) for player in (0, 1)]


@pytest.mark.parametrize("name", ASSIGNMENTS)
@pytest.mark.parametrize("game,n", MIXED)
def test_mixed_assignment_equals_plain_acts_selected_by_id(game, n, name, hip_lib):
    _, _, plain, active = mixed_world(game, n)
    host, all_rows, runs = mixed_case(game, n, name)
    for player, got in enumerate(runs):
        ids = host[:, player]
        computed = np.ones(n, bool) if all_rows else active[player]
        valid = (ids >= 0) & (ids < K)
        acted = valid & computed
        want_action = np.full(n, MARK, np.int32)
        want_action[valid & ~computed] = 0
        for k in range(K):
            mine = acted & (ids == k)
            want_action[mine] = plain[player, all_rows, k]["action"][mine]
        same_bits(got["action"], want_action, f"{name}, seat {player}: ACTION")
        assert (got["other"] == MARK).all()
        want_row = np.where(acted, ids, np.where(valid, -1, ROW_MARK)).astype(np.int32)
        same_bits(got["ids_row"], want_row, f"{name}, seat {player}: ids_row")
        plan = got["layout"].read(got["ws"])
        assert plan["acted"] == acted.sum() and plan["out_of_range"] == (ids >= K).sum()
        same_bits(plan["eff"], np.where(computed | ~valid, ids, -1).astype(np.int32), f"{name}, seat {player}: the effective ids")
        # logits and values through the lists: position j is world lists[j] under policy ids[lists[j]]
        worlds = plan["lists"]
        assert np.array_equal(np.sort(worlds), np.flatnonzero(acted))
        for k in range(K):
            mine = np.flatnonzero(ids[worlds] == k)  # list positions of policy k
            if len(mine) == 0:
                continue
            want = plain[player, all_rows, k]
            rows = np.searchsorted(want["worlds"], worlds[mine])  # the plain act's list is ascending
            assert np.array_equal(want["worlds"][rows], worlds[mine])
            same_bits(plan["logits"][mine][:, :want["logits"].shape[1]], want["logits"][rows], f"{name}, seat {player}, policy {k}: logits")
            same_bits(plan["values"][mine], want["values"][rows], f"{name}, seat {player}, policy {k}: values")
    if name == "tile_edges":
        plan = runs[0]["layout"].read(runs[0]["ws"])
        assert plan["count"][:2].tolist() == [32, 33] and np.bincount(plan["table"][:, 0], minlength=K)[:2].tolist() == [1, 2]
    if name == "holes":
        assert (host >= K).any() and (host < 0).any()


@pytest.mark.parametrize("name", ASSIGNMENTS)
@pytest.mark.parametrize("game,n", MIXED)
def test_plan_read_back(game, n, name, hip_lib):
    _, _, _, active = mixed_world(game, n)
    host, all_rows, runs = mixed_case(game, n, name)
    for player, got in enumerate(runs):
        ids = host[:, player]
        plan, lay = got["layout"].read(got["ws"]), got["layout"]
        acted = (ids >= 0) & (ids < K) & (np.ones(n, bool) if all_rows else active[player])
        counts = np.array([(acted & (ids == k)).sum() for k in range(K)])
        assert np.array_equal(plan["count"], counts) and np.array_equal(plan["start"], np.cumsum(counts) - counts)
        assert plan["tiles"] == sum((c + 31) // 32 for c in counts) <= lay.max_tiles
        lists = plan["lists"]
        for k in range(K):  # ascending and disjoint: each list is exactly its policy's worlds in order
            assert np.array_equal(lists[plan["start"][k]:plan["start"][k] + counts[k]], np.flatnonzero(acted & (ids == k)))
        covered = np.zeros(plan["acted"], np.int64)
        for policy, first, rows, zero in plan["table"]:
            assert 1 <= rows <= 32 and zero == 0 and 0 <= policy < K
            assert plan["start"][policy] <= first and first + rows <= plan["start"][policy] + counts[policy]
            assert (ids[lists[first:first + rows]] == policy).all()  # one policy per tile
            covered[first:first + rows] += 1
        assert (covered == 1).all()
        if n > 2048:
            assert counts.sum() > 0  # (the three-launch plan had something to place)


# ---------------------------------------------------------------- 4: determinism and containment

@pytest.mark.parametrize("game,n", [("hanabi_very_small", 33), ("balance", 1025)])
def test_same_bits_again_on_a_side_stream_and_inside_the_workspace(game, n, hip_lib):
    sim = warm_sim(game, n, seed=8)
    bank = make_bank(game, 3)
    ids = torch.from_numpy(np.stack([np.arange(n) % 3, (np.arange(n) + 1) % 4 - 1], axis=1).astype(np.int32)).to(DEV)
    first = bank_act(sim, 1, bank, ids, 31, 2)
    again = bank_act(sim, 1, bank, ids, 31, 2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        aside = bank_act(sim, 1, bank, ids, 31, 2)
    torch.cuda.synchronize()
    guard, size = 4096, first["layout"].total
    block = torch.full((size + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    block[guard:guard + size] = 0
    fenced = bank_act(sim, 1, bank, ids, 31, 2, workspace=block[guard:guard + size])
    for name, other in (("again", again), ("side stream", aside), ("guarded", fenced)):
        same_bits(other["action"], first["action"], f"{name}: ACTION")
        same_bits(other["ids_row"], first["ids_row"], f"{name}: ids_row")
        same_bits(other["ws"], first["ws"], f"{name}: the workspace")
    whole = cpu(block)
    assert (whole[:guard] == 0xA5).all() and (whole[guard + size:] == 0xA5).all()
    assert (first["action"] != MARK).sum() == (cpu(ids)[:, 1] >= 0).sum() > 0
    sim.close()


# ---------------------------------------------------------------- 5: the resample

@pytest.mark.parametrize("players", [0b11, 0b10])
@pytest.mark.parametrize("mode", ["robin", "random"])
def test_resample_against_the_twin(mode, players, hip_lib):
    n = 33
    sim = make_sim("hanabi_very_small", n)
    rng = np.random.default_rng(3)
    first, num = [3, 1], [1, 3]  # seat 1 draws from {1, 2, 3}, seat 0 from {3}: a range of one
    ids_host = np.stack([np.full(n, 3), rng.integers(1, 4, size=n)], axis=1).astype(np.int32)
    ids_host[rng.uniform(size=(n, 2)) < 0.2] = -1
    ids, episodes = torch.from_numpy(ids_host).to(DEV), torch.full((n,), 40, dtype=torch.int32, device=DEV)
    want_ids, want_episodes = ids_host.copy(), np.full(n, 40, np.int32)
    seen = []
    for t in range(12):
        sim.rollout_random(1, seed=9, first_step=t)
        wide_resample(sim, ids, episodes, mode, first, num, players=players, seed=11)
        torch.cuda.synchronize()
        done = cpu(sim.done_tensor()).reshape(-1)
        seen.append(int((done != 0).sum()))
        resample_twin(want_ids, want_episodes, done, mode, first, num, players, seed=11)
        same_bits(cpu(ids), want_ids, f"{mode}, step {t}: ids")
        same_bits(cpu(episodes), want_episodes, f"{mode}, step {t}: episodes")
    assert 0 < sum(seen) and min(seen) < n  # games ended, and not all at once
    assert (want_ids < 0).sum() == (ids_host < 0).sum() and (want_ids[:, 0][want_ids[:, 0] >= 0] == 3).all()
    sim.close()


# ---------------------------------------------------------------- 6 and 7: the two agents under env.step

def test_population_agent_reproduces_the_hand_issued_loop(hip_lib):
    n, k, steps, seed, mode = 33, 3, 12, 17, "random"
    game = "hanabi_very_small"
    bank = make_bank(game, k)
    ego = WidePolicy.from_module(twin.make_agent(game, "orthogonal", seed=55), device=DEV)
    scratch = torch.empty(int(_lib.lib().mrl_agent_workspace_bytes(n)), dtype=torch.uint8, device=DEV)
    env, hand = HanabiMadrona(n, 0, config=VERY_SMALL_CONFIG), HanabiMadrona(n, 0, config=VERY_SMALL_CONFIG)
    partner = WidePopulationAgent(env, bank, members=[1, 2], resample=mode, seed=seed)
    env.add_partner_agent(partner)
    assert partner.seat == 1
    env.reset()
    ids = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
    ids[:, 1] = torch.tensor([1, 2], dtype=torch.int32, device=DEV)[torch.arange(n, device=DEV) % 2]
    episodes = torch.zeros(n, dtype=torch.int32, device=DEV)
    finished = 0
    for t in range(steps):
        agent_act(env.sim, 0, ego, seed=3, step=t, workspace=scratch)
        env.step(env.static_actions[0].clone())
        agent_act(hand.sim, 0, ego, seed=3, step=t, workspace=scratch)
        agent_act_bank(hand.sim, 1, bank, ids, seed=seed, step=t)
        hand.sim.step()
        torch.cuda.synchronize()
        same_bits(cpu(env.static_actions), cpu(hand.static_actions), f"step {t}: actions")
        same_bits(cpu(env.static_dones), cpu(hand.static_dones), f"step {t}: DONE")
        wide_resample(hand.sim, ids, episodes, mode, [0, 1], [1, 2], players=0b10, seed=seed)
        torch.cuda.synchronize()
        same_bits(cpu(partner.ids), cpu(ids), f"step {t}: ids")
        same_bits(cpu(partner.episodes), cpu(episodes), f"step {t}: episodes")
        finished += int((cpu(hand.static_dones) != 0).sum())
    assert finished > 0 and (cpu(ids)[:, 0] == -1).all() and set(cpu(ids)[:, 1].tolist()) <= {1, 2}
    env.close()
    hand.close()
    # defaults on the beam: world n starts with members[n % len(members)], the other seat's column is -1
    env = BalanceMadronaTorch(7, 0)
    beam_bank = make_bank("balance", 3)
    agent = WidePopulationAgent(env, beam_bank, members=[2, 0], resample=None)
    env.add_partner_agent(agent)
    agent.get_action()
    agent.update(None, None)
    assert cpu(agent.ids).tolist() == [[-1, 2], [-1, 0]] * 3 + [[-1, 2]] and not cpu(agent.episodes).any()
    with pytest.raises(ValueError, match="consecutive"):
        WidePopulationAgent(env, beam_bank, members=[2, 0], resample="robin")
    env.close()
    cartpole = CartpoleMadronaTorch(4, 0)
    for build in (lambda: WidePopulationAgent(cartpole, beam_bank), lambda: WidePolicyAgent(cartpole, beam_bank.policy(0))):
        with pytest.raises(TypeError, match="no torch fallback"):
            build()
    cartpole.close()


def test_frozen_partner_acts_as_the_plain_act_without_a_record(hip_lib):
    n, game = 33, "hanabi_very_small"
    policy = WidePolicy.from_module(twin.make_agent(game, "peaked", seed=41), device=DEV)
    env = HanabiMadrona(n, 0, config=VERY_SMALL_CONFIG)
    partner = WidePolicyAgent(env, policy, seed=23)
    env.add_partner_agent(partner)
    assert partner.seat == 1
    before = cpu(policy.params)
    for t in range(4):
        env.static_actions.fill_(MARK)
        got = partner.get_action(None)
        assert got.data_ptr() == env.static_actions[1].data_ptr()
        torch.cuda.synchronize()
        got = cpu(env.static_actions)
        want = plain_act(env.sim, game, 1, policy, 23, t)  # the agent numbers its draws by its calls
        same_bits(got[1, :, 0], want["action"], f"call {t}: the partner's actions")
        assert (got[0] == MARK).all()
        partner.update(None, None)
        env.sim.rollout_random(1, seed=2, first_step=t)
    torch.cuda.synchronize()
    same_bits(cpu(policy.params), before, "a frozen partner's parameters")
    env.close()


# ---------------------------------------------------------------- 8: cross-play

def test_cross_play_matches_the_hand_loop(hip_lib):
    k, n, steps, seed, game = 2, 64, 24, 4, "hanabi_very_small"
    bank = make_bank(game, k)
    env = HanabiMadrona(n, 0, config=VERY_SMALL_CONFIG)
    with pytest.raises(ValueError, match="steps has no default"):
        cross_play(env, bank)
    result = cross_play(env, bank, greedy=False, seed=seed, steps=steps)
    torch.cuda.synchronize()
    mean_return, episodes = cpu(result.mean_return), cpu(result.episodes)
    env.close()
    # by hand on a twin simulator: the same calls, the sums on the host
    sim = make_sim(game, n)
    sim.enable_episode_stats()
    sim.reset_worlds(None)
    pair = np.arange(n) % (k * k)
    ids = torch.from_numpy(np.stack([pair // k, pair % k], axis=1).astype(np.int32)).to(DEV)
    total, finished = np.zeros(n, np.float64), np.zeros(n, np.int64)
    for t in range(steps):
        agent_act_bank(sim, 0, bank, ids, seed=seed, step=t)
        agent_act_bank(sim, 1, bank, ids, seed=seed, step=t)
        sim.step()
        torch.cuda.synchronize()
        over = cpu(sim.done_tensor()).reshape(n) != 0
        last = cpu(sim.last_episode_return_tensor()).reshape(2, n)[0]
        assert last.dtype == np.float32
        total += np.where(over, last.astype(np.float64), 0.0)
        finished += over
    sim.close()
    want_count = np.bincount(pair, weights=finished, minlength=k * k).astype(np.int64).reshape(k, k)
    want_sum = np.array([total[pair == q].sum() for q in range(k * k)]).reshape(k, k)
    assert mean_return.shape == (k, k) and mean_return.dtype == np.float64 and episodes.dtype == np.int64
    same_bits(episodes, want_count, "finished episodes per pair")
    assert (want_count > 0).all()
    same_bits(mean_return, want_sum / want_count, "mean return per pair")
    # the beam has a default, and the members choose the matrix
    env = BalanceMadronaTorch(16, 0)
    small = cross_play(env, make_bank("balance", 3), members_a=[2], members_b=[0, 1])
    assert tuple(small.mean_return.shape) == (1, 2) and (cpu(small.episodes) >= 8 * 6).all()  # eight worlds a pair, twelve steps
    env.close()


# ---------------------------------------------------------------- 9: training a member in place

def test_training_a_member_moves_its_row_only(hip_lib):
    n, game = 33, "balance"
    sim = warm_sim(game, n)
    bank = make_bank(game, 3)
    ids = torch.ones((n, 2), dtype=torch.int32, device=DEV)
    start = cpu(bank.params)
    before = bank_act(sim, 0, bank, ids, 5, 1)
    module = bank.policy(1).module()
    optimizer = torch.optim.SGD(module.parameters(), lr=0.05)
    x = sim.observation_tensor().to_torch()[0, :, :7].float()
    (module.actor(x).square().sum() + module.critic(x).sum()).backward()
    optimizer.step()
    torch.cuda.synchronize()
    after_params = cpu(bank.params)
    same_bits(after_params[0], start[0], "row 0")
    same_bits(after_params[2], start[2], "row 2")
    assert not np.array_equal(after_params[1], start[1])
    same_bits(cpu(bank.policy(1).params), after_params[1], "the member's view")
    assert WideOptimizer(bank.policy(1)).policy is bank.policy(1)
    # the next bank act reads the new row: it is the plain act under the member as it now stands
    after = bank_act(sim, 0, bank, ids, 5, 1)
    want = plain_act(sim, game, 0, bank.policy(1), 5, 1)
    plan = after["layout"].read(after["ws"])
    same_bits(after["action"], want["action"], "ACTION under the trained row")
    same_bits(plan["logits"][:, :4], want["logits"], "logits under the trained row")
    same_bits(plan["values"], want["values"], "values under the trained row")
    old = before["layout"].read(before["ws"])
    assert not np.array_equal(old["logits"][:, :4], plan["logits"][:, :4]) and not np.array_equal(old["values"], plan["values"])
    sim.close()


# ---------------------------------------------------------------- 10: refusals

def test_refusals_enqueue_nothing(hip_lib):
    n, k, game = 33, 3, "hanabi_very_small"
    L = _lib.lib()
    sim = warm_sim(game, n)
    bank = make_bank(game, k)
    d, s, a = twin.dims(game)
    sim.action_tensor().to_torch().fill_(MARK)
    size = agent_bank_workspace_bytes(n, k)
    ws = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    ids = torch.ones((n, 2), dtype=torch.int32, device=DEV)
    ids_row = torch.full((n,), ROW_MARK, dtype=torch.int32, device=DEV)
    episodes = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    sim.done_tensor().to_torch().fill_(1)  # a resample that ran would move every id
    first, num = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(3, 3)
    fine = _lib.CnnResampleDesc(1, first, num, 0)
    rows = {"obs": sim.observation_tensor().shape[2], "state": sim.agent_state_tensor().shape[2], "mask": sim.action_mask_tensor().shape[2]}

    def desc(params=bank.params.data_ptr(), count=k, stride=bank.num_params, obs_dim=d, state_dim=s, num_actions=a):
        return _lib.WideBankDesc(params, count, stride, obs_dim, state_dim, num_actions)

    def act(handle=None, player=0, b=desc(), ids_ptr=None, row_ptr=None, flags=0, workspace=None, wsize=None):
        return L.mrl_agent_act_bank(sim._handle if handle is None else handle, player, ctypes.byref(b) if b is not None else None,
                                    ids.data_ptr() if ids_ptr is None else ids_ptr, ids_row.data_ptr() if row_ptr is None else row_ptr, 1, 0,
                                    flags, ws.data_ptr() if workspace is None else workspace, size if wsize is None else wsize, None)

    def resample(handle=None, players=3, r=fine, ids_ptr=None, episodes_ptr=None):
        return L.mrl_agent_bank_resample(sim._handle if handle is None else handle, players, ctypes.byref(r) if r is not None else None,
                                         ids.data_ptr() if ids_ptr is None else ids_ptr,
                                         episodes.data_ptr() if episodes_ptr is None else episodes_ptr, None)

    kitchen = OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **layouts.get_base_layout_params("cramped_room", 40))
    refused = [
        act(handle=kitchen._handle), resample(handle=kitchen._handle),  # a kitchen simulator
        act(flags=_lib.AGENT_VALUE_ONLY), act(flags=_lib.AGENT_VALUE_ONLY | _lib.AGENT_ALL_ROWS), act(flags=8), act(flags=1 << 31),
        act(b=desc(obs_dim=rows["obs"] + 1)), act(b=desc(state_dim=rows["state"] + 1)), act(b=desc(num_actions=rows["mask"] + 1)),  # wrong dims
        act(b=desc(obs_dim=0)), act(b=desc(state_dim=0)), act(b=desc(num_actions=0)), act(b=desc(num_actions=65)),
        act(b=None), act(b=desc(params=None)), act(b=desc(count=0)), act(b=desc(count=257)), act(b=desc(stride=bank.num_params - 1)),
        act(player=2), act(ids_ptr=0), act(ids_ptr=ids.data_ptr() + 2), act(row_ptr=ids_row.data_ptr() + 2),
        act(workspace=0), act(workspace=ws.data_ptr() + 8), act(wsize=size - 1), act(wsize=0),  # a short or misaligned workspace
        resample(r=None), resample(players=0), resample(players=4), resample(ids_ptr=0), resample(episodes_ptr=0),
    ]
    assert refused == [_lib.MRL_ERR_INVALID] * len(refused), refused
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        agent_act_bank(sim, 0, bank, ids.to(torch.int64))
    with pytest.raises(ValueError):
        agent_act_bank(sim, 0, bank, ids[:-1])
    with pytest.raises(ValueError):
        agent_act_bank(sim, 0, bank.policy(0), ids)
    with pytest.raises(ValueError):
        agent_act_bank(kitchen, 0, bank, ids)
    with pytest.raises(ValueError):
        wide_resample(kitchen, ids, episodes, "robin", 0, 3)
    # a capturing stream: the plain act refuses one on this game, and so does the bank act
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                agent_act(sim, 0, bank.policy(0), workspace=ws[:size])
            with pytest.raises(_lib.MrlError, match="captured"):
                agent_act_bank(sim, 0, bank, ids, ids_row=ids_row, workspace=ws[:size])
            scratch.add_(0)
    torch.cuda.synchronize()
    # nothing was enqueued: ACTION, the workspace, ids_row, the ids and the episodes keep every byte
    assert (cpu(sim.action_tensor()) == MARK).all() and (cpu(ws) == 0xA5).all() and (cpu(ids_row) == ROW_MARK).all()
    assert (cpu(ids) == 1).all() and (cpu(episodes) == 5).all()
    # and the simulator still acts and resamples
    agent_act_bank(sim, 0, bank, ids, ids_row=ids_row, all_rows=True, workspace=ws[:size])
    wide_resample(sim, ids, episodes, "robin", 0, 3)
    torch.cuda.synchronize()
    assert (cpu(sim.action_tensor())[0] >= 0).all() and (cpu(ids_row) == 1).all()
    assert (cpu(ids) == 2).all() and (cpu(episodes) == 6).all()
    kitchen.close()
    sim.close()
