"""GPU: the policy bank -- ``mrl_cnn_act_bank``, ``mrl_cnn_bank_resample``, ``mrl_rollout_cnn_bank``, ``env.act_bank`` /
``env.rollout_bank``, ``CnnPopulationAgent``, ``cross_play`` and ``mappo_advantages(seats=...)``.

The oracle is the plain ``mrl_cnn_act``: a bank act must give every acted cell the bits the plain act gives it under the cell's
own policy, and must leave every other cell alone.  No tolerance appears anywhere except in the advantage test, whose bound is
worked out there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_twin as twin  # noqa: E402
from bank_cases import assert_plan_read_back, cpu, same_bits  # noqa: E402
from madrona_rl_envs_playground_amd import _lib, layouts  # noqa: E402
from madrona_rl_envs_playground_amd.envs import OvercookedMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.pantheonrl_extension import CnnPopulationAgent  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CartpoleSimulator, CnnActorCritic, CnnPolicy, CnnPolicyBank, CnnRecord,  # noqa: E402
                                                         CnnResample, ExecMode, MappoOptimizer, OvercookedSimulator,
                                                         SimplecookedSimulator, ValueNorm, cnn_act, cnn_act_bank, cnn_resample,
                                                         cross_play, gae, mappo_advantages, mappo_update, minibatch_indices,
                                                         resample_twin)

DEV = torch.device("cuda", 0)
RECORDED = ("actions", "logprobs", "values", "rewards", "dones", "next_done", "logits")
MARK, ACTION_MARK = -77, -7


def record_arrays(record):
    return {name: cpu(getattr(record, name)) for name in RECORDED if getattr(record, name) is not None}


def marked_record(num_steps, n, p, logits=True):
    """a record whose every cell holds a value no act writes"""
    record = CnnRecord(num_steps, n, p, DEV, logits=logits)
    for name in RECORDED:
        t = getattr(record, name)
        if t is not None:
            t.fill_(MARK)
    return record


def make_sim(game, layout, n, horizon=twin.HORIZON):
    if game == "simplecooked":  # one seat: F = 5 + 10
        return SimplecookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n,
                                     **layouts.get_simplecooked_layout_params(layout, horizon, max_num_players=1))
    return OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **layouts.get_base_layout_params(layout, horizon))


def trained_module(w, h, f, seed):
    """``cnn_twin.make_module``'s "trained" weights at any shape"""
    torch.manual_seed(seed)
    module = CnnActorCritic(w, h, f)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith("bias"):
                p.normal_(0.0, 0.1)
            elif "action_out" in name or "v_out" in name:
                p.normal_(0.0, 0.3)
            else:
                p.normal_(0.0, (2.0 / p[0].numel()) ** 0.5)
    return module


def make_bank(sim, k, first_seed=101):
    _, _, h, w, f = sim.observation_world_major_tensor().shape
    return CnnPolicyBank.from_policies([CnnPolicy.from_module(trained_module(w, h, f, first_seed + i), device=DEV) for i in range(k)])


def synthetic(sim, seed):
    """cnn_twin.synthetic_observations at the simulator's shape, written into its own tensor"""
    shape = tuple(sim.observation_world_major_tensor().shape)
    rng = np.random.default_rng(seed)
    obs = (rng.uniform(size=shape) < 0.25).astype(np.int8)
    obs = np.where(rng.uniform(size=shape) < 1.0 / 16, rng.integers(0, 21, size=shape).astype(np.int8), obs)
    obs = np.where(rng.uniform(size=shape) < 1.0 / 64, rng.integers(-3, 0, size=shape).astype(np.int8), obs).astype(np.int8)
    sim.observation_world_major_tensor().to_torch().copy_(torch.from_numpy(obs).to(DEV))


def one_act(sim, act, n, p):
    """``act(record)`` into row 1 of a marked record over a marked ACTION tensor -> the arrays"""
    record = marked_record(2, n, p)
    sim.action_tensor().to_torch().fill_(ACTION_MARK)
    act(record)
    torch.cuda.synchronize()
    out = record_arrays(record)
    out["action_tensor"] = cpu(sim.action_tensor())
    return out


# ---------------------------------------------------------------- 1: a bank of one is the plain act

@pytest.mark.parametrize("n", [1, 33, 257])
def test_bank_of_one_equals_the_plain_act(n, hip_lib):
    sim = make_sim("overcooked", "cramped_room", n)
    synthetic(sim, 1000 + n)
    bank = make_bank(sim, 1)
    ids = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    ids_row = torch.full((n, 2), 9, dtype=torch.int32, device=DEV)
    for kwargs in ({}, {"greedy": True}):
        want = one_act(sim, lambda r: cnn_act(sim, bank.policy(0), None, r, row=1, seed=5 + n, step=3, **kwargs), n, 2)
        got = one_act(sim, lambda r: cnn_act_bank(sim, bank, ids, None, r, ids_row, row=1, seed=5 + n, step=3, **kwargs), n, 2)
        for name in want:
            same_bits(got[name], want[name], f"K = 1, n = {n}, {kwargs}: {name}")
        assert (want["actions"][1] >= 0).all() and not (cpu(ids_row) != 0).any()
    sim.close()


# ---------------------------------------------------------------- 2 and 3: a mixed assignment, and the plan read back

def mixed_ids(n, p, k, players, counts, seed):
    """(N, P) int32: policy j acted in exactly counts[j] cells of the masked seats (None: every cell left over), one masked cell at
    k + 2 (outside the bank), a few at -1, the cells of other seats random valid ids (which must not be acted)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, k, size=(n, p)).astype(np.int32)
    seats = [s for s in range(p) if (players >> s) & 1]
    cells = rng.permutation(np.array([(w, s) for w in range(n) for s in seats]))
    at = 0
    for j, c in enumerate(counts):
        if c is None:
            continue
        for w, s in cells[at:at + c]:
            ids[w, s] = j
        at += c
    w, s = cells[at]
    ids[w, s] = k + 2
    at += 1
    rest = cells[at:]
    spare = min(5, len(rest)) if any(c is None for c in counts) else len(rest)
    for w, s in rest[:spare]:
        ids[w, s] = -1 - (int(w) % 2) * 6  # -1 and -7: every negative value is "not acted"
    for w, s in rest[spare:]:
        ids[w, s] = counts.index(None)
    return ids


# (game, layout, worlds, players, counts per policy; policy 2 of the four is assigned nowhere)
MIXED = {
    "n65": ("overcooked", "cramped_room", 65, 0b11, (1, 31, 0, 32)),
    "n513": ("overcooked", "cramped_room", 513, 0b11, (33, None, 0, 32)),        # 1026 cells: the plan's second chunk of 1024
    "n1024": ("overcooked", "cramped_room", 1024, 0b11, (33, None, 0, 32)),      # 2048 cells: the last size one workgroup plans
    "n1025": ("overcooked", "cramped_room", 1025, 0b11, (33, None, 0, 32)),      # 2050 cells: the first size of count, scan, place
    "n65_seat1": ("overcooked", "cramped_room", 65, 0b10, (1, 31, 0, 30)),
    "n513_seat1": ("overcooked", "cramped_room", 513, 0b10, (33, None, 0, 32)),
    "simple_1p": ("simplecooked", "simple", 130, 0b1, (31, 33, 0, 32)),
    "asymmetric": ("overcooked", "asymmetric_advantages", 33, 0b11, (1, 32, 0, 31)),
}


@functools.lru_cache(maxsize=None)
def mixed_case(key):
    game, layout, n, players, counts = MIXED[key]
    k = 4
    sim = make_sim(game, layout, n)
    p, f = sim.observation_world_major_tensor().shape[1], sim.observation_world_major_tensor().shape[4]
    synthetic(sim, 77 + n)
    bank = make_bank(sim, k)
    ids_host = mixed_ids(n, p, k, players, counts, seed=n + players)
    ids = torch.from_numpy(ids_host).to(DEV)
    seed, step = 4242 + n, 9
    plain = [one_act(sim, lambda r, j=j: cnn_act(sim, bank.policy(j), players, r, row=1, seed=seed, step=step), n, p) for j in range(k)]
    size = int(sim._L.mrl_cnn_bank_workspace_bytes(n, p, k))
    block = torch.full((size + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ids_row = torch.full((n, p), 9, dtype=torch.int32, device=DEV)
    got = one_act(sim, lambda r: cnn_act_bank(sim, bank, ids, players, r, ids_row, row=1, seed=seed, step=step, workspace=block[256:256 + size]), n, p)
    again = one_act(sim, lambda r: cnn_act_bank(sim, bank, ids, players, r, None, row=1, seed=seed, step=step, workspace=block[256:256 + size]), n, p)
    out = {"n": n, "p": p, "f": f, "k": k, "players": players, "ids": ids_host, "plain": plain, "got": got, "again": again,
           "ids_row": cpu(ids_row), "block": cpu(block), "size": size, "ids_after": cpu(ids)}
    sim.close()
    return out


def acted_mask(c):
    seat_in_mask = np.array([(c["players"] >> s) & 1 for s in range(c["p"])], dtype=bool)[None, :]
    return seat_in_mask & (c["ids"] >= 0) & (c["ids"] < c["k"])


@pytest.mark.parametrize("key", sorted(MIXED))
def test_mixed_assignment_equals_plain_acts_selected_by_id(key, hip_lib):
    c = mixed_case(key)
    n, p, k, ids = c["n"], c["p"], c["k"], c["ids"]
    if key == "simple_1p":
        assert p == 1 and c["f"] == 15
    acted = acted_mask(c)
    counts = [int((acted & (ids == j)).sum()) for j in range(k)]
    want_counts = MIXED[key][4]
    assert all(w is None or w == g for w, g in zip(want_counts, counts)) and counts[2] == 0, counts
    assert (~acted).sum() > 0 and (ids[~acted] < 0).any() and (ids >= k).sum() == 1
    for name in RECORDED:
        for row in range(c["got"][name].shape[0]) if name != "next_done" else [None]:
            got = c["got"][name] if row is None else c["got"][name][row]
            want = np.full_like(got, MARK)
            for j in range(k):
                plain = c["plain"][j][name] if row is None else c["plain"][j][name][row]
                pick = acted & (ids == j)
                want[pick] = plain[pick]
            same_bits(got, want, f"{key}: {name} row {row}")
    # what an act at row 1 writes at all: the plain acts wrote it for their whole mask, so the selection above is not all marks
    assert (c["got"]["actions"][1][acted] >= 0).all() and (c["got"]["values"][1][acted] != MARK).all()
    assert (c["got"]["rewards"][0][acted] != MARK).all() and (c["got"]["logits"][1][acted] != MARK).all()
    assert (c["got"]["actions"][1][~acted] == MARK).all() and (c["got"]["values"][1][~acted] == MARK).all()
    # ACTION (P, N, 1): the acted cells' actions, every other entry untouched
    action = c["got"]["action_tensor"][:, :, 0].T
    same_bits(action[acted], c["got"]["actions"][1][acted], f"{key}: ACTION of acted cells")
    assert (action[~acted] == ACTION_MARK).all()
    # the members do differ: somewhere two policies give a cell different logits
    assert any(not np.array_equal(c["plain"][0]["logits"][1][0], c["plain"][j]["logits"][1][0]) for j in (1, 3))
    # ids as the act used them; the caller's ids are read only; the same bits on a second run
    same_bits(c["ids_row"], np.where(acted, ids, -1).astype(np.int32), f"{key}: ids_row")
    same_bits(c["ids_after"], ids, f"{key}: ids")
    for name in c["got"]:
        same_bits(c["again"][name], c["got"][name], f"{key}: second run, {name}")


@pytest.mark.parametrize("key", sorted(MIXED))
def test_plan_read_back(key, hip_lib):
    c = mixed_case(key)
    assert_plan_read_back(c["block"], c["size"], c["n"], c["p"], c["k"], c["ids"], acted_mask(c), out_of_range=1)


# ---------------------------------------------------------------- 4: the resample against its twin

@pytest.mark.parametrize("players", [0b11, 0b01])
@pytest.mark.parametrize("mode", ["robin", "random"])
def test_resample_against_the_twin(mode, players, hip_lib):
    n, horizon = 33, 5
    sim = make_sim("overcooked", "cramped_room", n, horizon)
    rng = np.random.default_rng(3)
    first, num = [1, 3], [3, 1]  # seat 0 draws from {1, 2, 3}, seat 1 from {3}: a range of one
    ids_host = np.stack([rng.integers(1, 4, size=n), np.full(n, 3)], axis=1).astype(np.int32)
    ids_host[rng.uniform(size=(n, 2)) < 0.2] = -1
    ids, episodes = torch.from_numpy(ids_host).to(DEV), torch.full((n,), 40, dtype=torch.int32, device=DEV)
    want_ids, want_episodes = ids_host.copy(), np.full(n, 40, np.int32)
    late = torch.arange(n, device=DEV) % 3 == 0  # these worlds restart after step 2: their episodes end three steps later
    seen = []
    for t in range(8):
        sim.action_tensor().to_torch().copy_(torch.from_numpy(rng.integers(0, 6, size=(2, n, 1)).astype(np.int32)).to(DEV))
        sim.step()
        if t == 1:
            sim.reset_worlds(late)
        cnn_resample(sim, ids, episodes, mode, first, num, players=players, seed=11)
        torch.cuda.synchronize()
        done = cpu(sim.done_tensor()).reshape(-1)
        seen.append(int((done != 0).sum()))
        before = want_ids.copy()
        resample_twin(want_ids, want_episodes, done, mode, first, num, players, seed=11)
        same_bits(cpu(ids), want_ids, f"{mode}, step {t}: ids")
        same_bits(cpu(episodes), want_episodes, f"{mode}, step {t}: episodes")
        # the twin itself moves only finished worlds, masked seats and non-negative cells, inside the ranges
        moved = want_ids != before
        assert not moved[done == 0].any() and not moved[before < 0].any()
        assert not moved[:, 1].any()  # a range of one, or a seat outside the mask
        if mode == "robin":  # three ids: the next one is another one
            assert (moved[:, 0] == ((done != 0) & (before[:, 0] >= 0))).all()
        live = want_ids[:, 0] >= 0
        assert ((want_ids[live, 0] >= 1) & (want_ids[live, 0] <= 3)).all()
    assert 0 in seen and 0 < max(seen) < n and (want_episodes > 40).all()  # some, not all, worlds finish at a time
    assert (want_ids < 0).sum() == (ids_host < 0).sum()
    sim.close()


# ---------------------------------------------------------------- 5: the rollout against the hand-issued loop

ROLLOUT = dict(layout="cramped_room", n=33, t=12, horizon=5, k=3, seed=21, first_step=100)


def rollout_ids(n):
    """seat 0 of world n starts under n mod 3, seat 1 under (n + 1) mod 3; two cells are never acted"""
    ids = torch.stack([torch.arange(n) % 3, (torch.arange(n) + 1) % 3], dim=1).to(torch.int32)
    ids[4, 0] = ids[9, 1] = -1
    return ids.to(DEV).contiguous()


def final_state(env):
    return {"obs_own": cpu(env.static_world_major_observations), "players": cpu(env.sim.state_players_tensor()),
            "objects": cpu(env.sim.state_objects_tensor()), "timestep": cpu(env.sim.state_timestep_tensor()),
            "action_tensor": cpu(env.static_actions)}


@functools.lru_cache(maxsize=None)
def rollout_case(mode, pieces=1):
    """one rollout of T, or ``pieces`` chained ones of T / pieces with their records put together"""
    r = ROLLOUT
    env = OvercookedMadrona(r["layout"], r["n"], 0, horizon=r["horizon"])
    bank = make_bank(env.sim, r["k"])
    ids, episodes = rollout_ids(r["n"]), torch.zeros(r["n"], dtype=torch.int32, device=DEV)
    resample = CnnResample(mode, [0, 1], [3, 2], 2, seed=r["seed"]) if mode else None
    t = r["t"] // pieces
    parts = []
    for piece in range(pieces):
        record, ring, ids_record = env.rollout_bank(bank, ids, t, episodes=episodes, resample=resample, seed=r["seed"],
                                                    first_step=r["first_step"] + piece * t, record=CnnRecord(t, r["n"], 2, DEV, logits=True))
        torch.cuda.synchronize()
        parts.append((record_arrays(record), cpu(ring), cpu(ids_record)))
    out = {name: np.concatenate([part[0][name][:t] for part in parts]) for name in ("actions", "logprobs", "rewards", "dones", "logits")}
    out["values"] = np.concatenate([part[0]["values"][:t] for part in parts] + [parts[-1][0]["values"][t:]])
    out["next_done"] = parts[-1][0]["next_done"]
    out["ring"] = np.concatenate([part[1][:t] for part in parts] + [parts[-1][1][t:]])
    out["ids_record"] = np.concatenate([part[2][:t] for part in parts] + [parts[-1][2][t:]])
    out["ids"], out["episodes"] = cpu(ids), cpu(episodes)
    out["final"] = final_state(env)
    env.close()
    return out


@functools.lru_cache(maxsize=None)
def hand_case(mode):
    """the same as calls: act_bank, step, resample, T times; the closing value-only act"""
    r = ROLLOUT
    n, t = r["n"], r["t"]
    env = OvercookedMadrona(r["layout"], n, 0, horizon=r["horizon"])
    bank = make_bank(env.sim, r["k"])
    ids, episodes = rollout_ids(n), torch.zeros(n, dtype=torch.int32, device=DEV)
    record = CnnRecord(t, n, 2, DEV, logits=True)
    ring = torch.empty((t + 1,) + tuple(env.static_world_major_observations.shape), dtype=torch.int8, device=DEV)
    ids_record = torch.empty((t + 1, n, 2), dtype=torch.int32, device=DEV)
    ring[0].copy_(env.static_world_major_observations)
    for k in range(t):
        actions = env.act_bank(bank, ids, record=record, ids_row=ids_record[k], row=k, seed=r["seed"], step=r["first_step"] + k)
        env.n_step(actions.clone(), out=ring[k + 1])
        if mode:
            cnn_resample(env.sim, ids, episodes, mode, [0, 1], [3, 2], seed=r["seed"])
    cnn_act_bank(env.sim, bank, ids, None, record, ids_record[t], row=t, value_only=True)
    torch.cuda.synchronize()
    out = record_arrays(record)
    out.update(ring=cpu(ring), ids_record=cpu(ids_record), ids=cpu(ids), episodes=cpu(episodes), final=final_state(env))
    env.close()
    return out


def assert_same_rollout(got, want, what, final=("players", "objects", "timestep", "action_tensor")):
    for name in RECORDED + ("ring", "ids_record", "ids", "episodes"):
        same_bits(got[name], want[name], f"{what}: {name}")
    for name in final:
        same_bits(got["final"][name], want["final"][name], f"{what}: the simulator's {name}")


@pytest.mark.parametrize("mode", ["robin", "random"])
def test_rollout_bank_equals_the_hand_issued_loop(mode, hip_lib):
    got, want = rollout_case(mode), hand_case(mode)
    assert_same_rollout(got, want, f"rollout against calls, {mode}")
    same_bits(got["final"]["obs_own"], got["ring"][ROLLOUT["t"]], "the simulator's own tensor after the rollout")
    # it is a test of something: episodes end (twice per world), ids move, acted cells only are recorded
    assert (got["episodes"] == 2).all() and not np.array_equal(got["ids_record"][0], got["ids_record"][ROLLOUT["t"]])
    assert (got["ids_record"][:, 4, 0] == -1).all() and (got["ids_record"][:, 9, 1] == -1).all() and (got["ids_record"] >= 0).sum() > 0
    assert ((got["ids_record"][:, :, 0] <= 2) & (got["ids_record"][:, :, 1] <= 2)).all()
    assert (got["ids_record"][6:, [0, 1, 2], 1] >= 1).all()  # seat 1 draws from {1, 2} once its first episode is over
    assert not got["values"][:, 4, 0].any() and not got["actions"][:, 9, 1].any()  # the record started at zero and stays there
    # each act ran under the ids of its row: row k of the record equals a plain act of policy j wherever ids_record[k] == j is
    # what test_mixed_assignment pins; here the rows' ids are the resample twin's
    ids, episodes = cpu(rollout_ids(ROLLOUT["n"])), np.zeros(ROLLOUT["n"], np.int32)
    for k in range(ROLLOUT["t"]):
        same_bits(got["ids_record"][k], ids, f"ids_record[{k}] against the twin")
        done = got["dones"][k + 1] if k + 1 < ROLLOUT["t"] else got["next_done"]  # DONE behind step k, in the columns of acted cells
        resample_twin(ids, episodes, done.max(axis=1), mode, [0, 1], [3, 2], 0b11, seed=ROLLOUT["seed"])
    same_bits(got["ids"], ids, "ids after the rollout against the twin")


@pytest.mark.parametrize("mode", ["robin", "random"])
def test_two_chained_bank_rollouts_equal_one(mode, hip_lib):
    assert_same_rollout(rollout_case(mode, pieces=2), rollout_case(mode), f"two rollouts of 6 against one of 12, {mode}")


def test_bank_of_one_rollout_equals_the_plain_rollout(hip_lib):
    r = ROLLOUT
    n, t = r["n"], r["t"]
    runs = []
    for banked in (False, True):
        env = OvercookedMadrona(r["layout"], n, 0, horizon=r["horizon"])
        bank = make_bank(env.sim, 1)
        record = CnnRecord(t, n, 2, DEV, logits=True)
        if banked:
            ids = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
            _, ring, ids_record = env.rollout_bank(bank, ids, t, seed=r["seed"], first_step=r["first_step"], record=record)
            assert not cpu(ids_record).any() and not cpu(ids).any()
        else:
            _, ring = env.rollout(bank.policy(0), t, seed=r["seed"], first_step=r["first_step"], record=record)
        torch.cuda.synchronize()
        runs.append(dict(record_arrays(record), ring=cpu(ring), final=final_state(env)))
        env.close()
    for name in RECORDED + ("ring",):
        same_bits(runs[1][name], runs[0][name], f"K = 1 rollout against mrl_rollout_cnn: {name}")
    for name in runs[0]["final"]:
        same_bits(runs[1]["final"][name], runs[0]["final"][name], f"K = 1 rollout against mrl_rollout_cnn: the simulator's {name}")


# ---------------------------------------------------------------- 6: the population agent

def test_population_agent_reproduces_the_rollout(hip_lib):
    """seat 1 is a CnnPopulationAgent inside VectorMultiAgentEnv.step, seat 0 the same calls by hand: test 5's ids and actions"""
    r = ROLLOUT
    n, t, mode = r["n"], r["t"], "random"
    want = rollout_case(mode)
    env = OvercookedMadrona(r["layout"], n, 0, horizon=r["horizon"])
    bank = make_bank(env.sim, r["k"])
    partner = CnnPopulationAgent(env, bank, members=[1, 2], resample=mode, seed=r["seed"])
    env.add_partner_agent(partner)
    assert partner.seat == 1
    partner._draws = r["first_step"]  # the rollout numbered its draws from first_step
    partner._attach()
    partner.ids.copy_(rollout_ids(n))  # seat 1 of world n starts under (n + 1) mod 3 there, a member outside the agent's range too
    partner.ids[:, 0] = -1
    ego_ids, ego_episodes = rollout_ids(n), torch.zeros(n, dtype=torch.int32, device=DEV)
    ego_ids[:, 1] = -1
    env.reset()
    for k in range(t):
        same_bits(cpu(ego_ids)[:, 0], want["ids_record"][k][:, 0], f"step {k}: the ego's ids")
        same_bits(cpu(partner.ids)[:, 1], want["ids_record"][k][:, 1], f"step {k}: the partner's ids")
        cnn_act_bank(env.sim, bank, ego_ids, 0b01, seed=r["seed"], step=r["first_step"] + k)
        env.step(env.static_actions[0])
        torch.cuda.synchronize()
        acted = want["ids_record"][k] >= 0
        same_bits(cpu(env.static_actions)[:, :, 0].T[acted], want["actions"][k][acted], f"step {k}: actions")
        cnn_resample(env.sim, ego_ids, ego_episodes, mode, [0, 1], [3, 2], players=0b01, seed=r["seed"])
    same_bits(cpu(partner.ids)[:, 1], want["ids"][:, 1], "the partner's ids at the end")
    same_bits(cpu(partner.episodes), want["episodes"], "the partner's episode counts")
    assert (cpu(partner.ids)[:, 0] == -1).all()
    env.close()
    # defaults: world n starts with members[n % len(members)], the other seat's column is -1
    env = OvercookedMadrona(r["layout"], 7, 0, horizon=r["horizon"])
    agent = CnnPopulationAgent(env, bank, members=[2, 0], resample=None)
    env.add_partner_agent(agent)
    agent.get_action()
    agent.update(None, None)
    assert cpu(agent.ids).tolist() == [[-1, 2], [-1, 0]] * 3 + [[-1, 2]] and not cpu(agent.episodes).any()
    with pytest.raises(ValueError, match="consecutive"):
        CnnPopulationAgent(env, bank, members=[2, 0], resample="robin")
    with pytest.raises(TypeError, match="no torch fallback"):
        CnnPopulationAgent(object(), bank)
    env.close()


# ---------------------------------------------------------------- 7: cross-play

CROSS_SEEDS = (101, 102)  # make_bank's first two members


def test_cross_play_matches_one_world_runs(hip_lib):
    layout, n, horizon = "cramped_room", 8, 20
    env = OvercookedMadrona(layout, n, 0, horizon=horizon)
    bank = make_bank(env.sim, 2, CROSS_SEEDS[0])
    trace, step = [], env.sim.step

    def recording_step():
        trace.append(env.static_actions.clone())
        step()

    env.sim.step = recording_step
    result = cross_play(env, bank, greedy=True, seed=3)
    torch.cuda.synchronize()
    del env.sim.step
    assert len(trace) == horizon
    trace = np.stack([cpu(a)[:, :, 0] for a in trace])  # (horizon, P, N)
    mean_return, episodes = cpu(result.mean_return), cpu(result.episodes)
    assert mean_return.shape == (2, 2) and episodes.tolist() == [[2, 2], [2, 2]]
    env.close()
    singles = {}
    for a in range(2):
        for b in range(2):
            sim = make_sim("overcooked", layout, 1, horizon)
            sim.enable_episode_stats()
            sim.reset_worlds(None)
            taken = []
            for t in range(horizon):
                cnn_act(sim, bank.policy(a), 0b01, seed=3, step=t, greedy=True)
                cnn_act(sim, bank.policy(b), 0b10, seed=3, step=t, greedy=True)
                taken.append(sim.action_tensor().to_torch().clone())
                sim.step()
            torch.cuda.synchronize()
            singles[a, b] = (np.stack([cpu(x)[:, 0, 0] for x in taken]), float(cpu(sim.last_episode_return_tensor()).reshape(2, 1)[0, 0]))
            sim.close()
    for world in range(n):
        pair = world % 4
        same_bits(trace[:, :, world], singles[pair // 2, pair % 2][0], f"world {world}: the action trace")
    for a in range(2):
        for b in range(2):
            assert mean_return[a, b] == singles[a, b][1]
    traces = [singles[a, b][0] for a in range(2) for b in range(2)]
    assert sum(not np.array_equal(traces[i], traces[j]) for i in range(4) for j in range(i)) >= 1  # at least two pairs differ
    small = OvercookedMadrona(layout, 3, 0, horizon=horizon)
    with pytest.raises(ValueError, match="cannot play"):
        cross_play(small, bank)
    small.close()


# ---------------------------------------------------------------- 8 and 9: training a member, the ego's advantages

@functools.lru_cache(maxsize=None)
def training_record():
    """a rollout of bank member 1 (seat 0) against members 0 and 2 (seat 1): record, ring, the bank's parameters at that time"""
    n, t = 33, 6
    env = OvercookedMadrona("cramped_room", n, 0, horizon=5)
    bank = make_bank(env.sim, 3)
    ids = torch.stack([torch.ones(n), (torch.arange(n) % 2) * 2], dim=1).to(torch.int32).to(DEV).contiguous()
    record, ring, _ = env.rollout_bank(bank, ids, t, seed=8)
    torch.cuda.synchronize()
    env.close()
    return record, ring, bank.params.clone()


def test_update_through_a_view_moves_its_row_only(hip_lib):
    record, ring, start = training_record()
    n, t = record.num_worlds, record.num_steps
    w, h, _, f = twin.shape("cramped_room")
    bank = CnnPolicyBank(w, h, f, 3, device=DEV)
    bank.params.copy_(start)
    alone = CnnPolicy(w, h, f, device=DEV)
    alone.params.copy_(start[1])
    ego = torch.arange(t * n, device=DEV, dtype=torch.int32) * 2  # the samples of seat 0: (t N + n) P + 0
    stats = []
    for policy in (bank.policy(1), alone):
        value_norm = ValueNorm(DEV)
        advantages, returns = mappo_advantages(record, value_norm, seats=[0])
        optimizer = MappoOptimizer(policy)
        shuffles = torch.Generator(device=DEV).manual_seed(5)
        for _ in range(2):
            indices = ego[minibatch_indices(t * n, 2, 1, generator=shuffles, device=DEV).long()].contiguous()
            stats.append(cpu(mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm).stats))
    torch.cuda.synchronize()
    after = cpu(bank.params)
    same_bits(after[0], cpu(start)[0], "row 0")
    same_bits(after[2], cpu(start)[2], "row 2")
    same_bits(after[1], cpu(alone.params), "row 1 against the same update on a stand-alone copy")
    assert not np.array_equal(after[1], cpu(start)[1])
    same_bits(stats[0], stats[2], "stats of the first update")
    same_bits(stats[1], stats[3], "stats of the second update")


def test_advantages_over_the_ego_seat(hip_lib):
    record, _, _ = training_record()
    raw, raw_returns = gae(record.rollout(), 0.99, 0.95)
    shape = (record.num_steps, record.num_worlds, record.num_players)
    raw = raw.view(shape)
    got, returns = mappo_advantages(record, None, seats=[0])
    want = raw.clone()
    want[:, :, 0] = (raw[:, :, 0] - raw[:, :, 0].mean()) / (raw[:, :, 0].std() + 1e-5)
    # the same torch expressions on the same device: the reductions may be grouped differently from one slicing to the next,
    # so the bound is a few float32 roundings of a normalised advantage of O(1), not bits
    assert float((got - want).abs().max()) <= 1e-5
    same_bits(cpu(got[:, :, 1]), cpu(raw[:, :, 1]), "the partner's column keeps its raw advantages")
    same_bits(cpu(returns), cpu(raw_returns.view(shape)), "returns")
    ego = got[:, :, 0]
    assert abs(float(ego.mean())) <= 1e-5 and abs(float(ego.std()) - 1.0) <= 1e-3
    # the default is what it was
    whole, _ = mappo_advantages(record, None)
    assert float((whole - (raw - raw.mean()) / (raw.std() + 1e-5)).abs().max()) <= 1e-5
    assert float((whole[:, :, 0] - ego).abs().max()) > 1e-4  # and differs: the partner's critics are other nets


# ---------------------------------------------------------------- 10: refusals

def test_refusals_enqueue_nothing(hip_lib):
    n, t, k = 33, 2, 3
    L = _lib.lib()
    sim = make_sim("overcooked", "cramped_room", n)
    p = 2
    bank = make_bank(sim, k)
    record = marked_record(t, n, p)
    sim.action_tensor().to_torch().fill_(ACTION_MARK)
    size = int(L.mrl_cnn_bank_workspace_bytes(n, p, k))
    ws = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    ring = torch.zeros((t + 1,) + tuple(sim.observation_world_major_tensor().shape), dtype=torch.int8, device=DEV)
    ids = torch.ones((n, p), dtype=torch.int32, device=DEV)
    episodes = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    ids_record = torch.full((t + 1, n, p), 9, dtype=torch.int32, device=DEV)
    sim.done_tensor().to_torch().fill_(1)  # a resample that ran would move every id
    good, rec = bank.desc(), record.struct
    first, num = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(3, 3)
    fine = _lib.CnnResampleDesc(1, first, num, 0)

    def desc(params=bank.params.data_ptr(), count=k, stride=bank.num_params, hidden=64, flags=0):
        return _lib.CnnBankDesc(params, count, stride, hidden, flags)

    def act(handle=None, players=3, d=good, ids_ptr=None, r=rec, row=0, flags=0, workspace=None, wsize=None):
        return L.mrl_cnn_act_bank(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                  ids.data_ptr() if ids_ptr is None else ids_ptr, ctypes.byref(r) if r is not None else None, None, row, 1, 0,
                                  flags, ws.data_ptr() if workspace is None else workspace, size if wsize is None else wsize, None)

    def resample(handle=None, players=3, d=fine, ids_ptr=None, episodes_ptr=None):
        return L.mrl_cnn_bank_resample(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                       ids.data_ptr() if ids_ptr is None else ids_ptr,
                                       episodes.data_ptr() if episodes_ptr is None else episodes_ptr, None)

    def rollout(handle=None, players=3, d=good, ids_ptr=None, episodes_ptr=None, again=fine, r=rec, ring_ptr=None, wsize=None):
        return L.mrl_rollout_cnn_bank(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                      ids.data_ptr() if ids_ptr is None else ids_ptr,
                                      episodes.data_ptr() if episodes_ptr is None else episodes_ptr,
                                      ctypes.byref(again) if again is not None else None, ctypes.byref(r) if r is not None else None,
                                      ids_record.data_ptr(), ring.data_ptr() if ring_ptr is None else ring_ptr, 1, 0, ws.data_ptr(),
                                      size if wsize is None else wsize, None)

    def sampler(mode=1, first_id=(0, 0), num_ids=(3, 3), null=False):
        f, m = (ctypes.c_uint32 * 2)(*first_id), (ctypes.c_uint32 * 2)(*num_ids)
        keep.append((f, m))
        return _lib.CnnResampleDesc(mode, None if null else f, m, 0)

    keep = []
    other = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    holes = _lib.CnnRecordDesc(*[None if name == "values" else getattr(record, name).data_ptr() for name in _lib.CNN_RECORD_BUFFERS], t)
    refused = [
        act(handle=other._handle), rollout(handle=other._handle), resample(handle=other._handle),  # not a kitchen
        act(d=None), rollout(d=None), act(d=desc(params=None)), act(d=desc(hidden=128)), act(d=desc(flags=2)),
        act(d=desc(count=0)), act(d=desc(count=257)), rollout(d=desc(count=0)), rollout(d=desc(count=257)),
        act(d=desc(stride=bank.num_params - 1)), rollout(d=desc(stride=0)),
        act(ids_ptr=0), rollout(ids_ptr=0), resample(ids_ptr=0), resample(episodes_ptr=0), rollout(episodes_ptr=0),
        act(players=0), act(players=4), rollout(players=0), resample(players=0), resample(players=4),
        act(r=holes), rollout(r=holes), rollout(r=None), rollout(ring_ptr=0),
        act(row=t), act(row=t - 1, flags=_lib.CNN_VALUE_ONLY), act(r=None, row=t, flags=_lib.CNN_VALUE_ONLY), act(flags=8),
        act(workspace=0), act(workspace=ws.data_ptr() + 8), act(wsize=size - 1), rollout(wsize=size - 1),
        resample(d=None), resample(d=sampler(mode=0)), resample(d=sampler(mode=3)), resample(d=sampler(null=True)),
        resample(d=sampler(num_ids=(3, 0))), resample(d=sampler(first_id=(0, 255), num_ids=(3, 2))), resample(d=sampler(num_ids=(257, 1))),
        rollout(again=sampler(num_ids=(0, 3))), rollout(again=sampler(mode=7)),
    ]
    assert refused == [_lib.MRL_ERR_INVALID] * len(refused), refused
    # a seat outside `players` may carry any range: it is not read
    nobody = torch.full((n, p), -1, dtype=torch.int32, device=DEV)
    assert resample(players=1, d=sampler(num_ids=(3, 0)), ids_ptr=nobody.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (cpu(nobody) == -1).all() and (cpu(episodes) == 6).all()
    episodes.fill_(5)
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        cnn_act_bank(sim, bank, ids.to(torch.int64))
    with pytest.raises(ValueError):
        cnn_act_bank(sim, bank, ids[:-1])
    with pytest.raises(ValueError):
        cnn_act_bank(sim, bank.policy(0), ids)
    with pytest.raises(ValueError):
        cnn_resample(sim, ids, episodes.to(torch.int64), "robin", 0, 3)
    with pytest.raises(ValueError):
        sim.rollout_cnn_bank(bank, ids, record, ring, resample=CnnResample("robin", 0, 3, 2))  # no episodes
    # a capturing stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                cnn_act_bank(sim, bank, ids, None, record, row=0, workspace=ws[:size])
            scratch.add_(0)
    torch.cuda.synchronize()
    # nothing was enqueued
    for name, value in record_arrays(record).items():
        assert (value == MARK).all(), name
    assert (cpu(sim.action_tensor()) == ACTION_MARK).all() and not cpu(ring).any() and (cpu(ws) == 0xA5).all()
    assert (cpu(ids) == 1).all() and (cpu(episodes) == 5).all() and (cpu(ids_record) == 9).all()
    # and the simulator still acts, steps and resamples
    cnn_act_bank(sim, bank, ids, None, record, row=0, workspace=ws[:size])
    sim.step()
    sim.done_tensor().to_torch().fill_(1)
    cnn_resample(sim, ids, episodes, "robin", 0, 3)
    torch.cuda.synchronize()
    assert (cpu(record.actions)[0] >= 0).all() and (cpu(ids) == 2).all() and (cpu(episodes) == 6).all()
    other.close()
    sim.close()
