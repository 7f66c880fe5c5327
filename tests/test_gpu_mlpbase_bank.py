"""GPU: the balance beam's policy bank -- ``mrl_mlpbase_act_bank``, ``mrl_mlpbase_bank_resample``, ``mrl_rollout_mlpbase_bank``,
``env.act_bank`` / ``env.rollout_bank``, ``MlpBasePopulationAgent``, ``cross_play`` on an ``MlpBasePolicyBank`` and
``mappo_advantages(seats=...)`` on a bank rollout.

The oracle is the plain ``mrl_mlpbase_act``, which tests/test_gpu_balance_mappo.py checks against its twin: a bank act must give
every acted cell the bits the plain act gives it under the cell's own policy, and must leave every other cell alone.  Where a
comparison needs a second run, a second, identically created simulator is fed the same actions (the beam numbers its episodes
deterministically).  No tolerance appears anywhere except in the advantage test, whose bound is worked out there."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bank_cases import assert_plan_read_back, cpu, same_bits  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.pantheonrl_extension import MlpBasePopulationAgent  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (BalanceBeamSimulator, BankResample, CartpoleSimulator, CnnResample, ExecMode,  # noqa: E402
                                                         MappoOptimizer, MlpBaseActorCritic, MlpBasePolicy, MlpBasePolicyBank,
                                                         MlpBaseRecord, ValueNorm, cross_play, gae, mappo_advantages, mappo_update,
                                                         minibatch_indices, mlpbase_act, mlpbase_act_bank, mlpbase_resample,
                                                         resample_twin, wide_resample)

DEV = torch.device("cuda", 0)
RECORDED = _lib.MLPBASE_RECORD_BUFFERS  # actions, logprobs, values, rewards, dones, next_done, logits, obs
MARK, ACTION_MARK = -77, -7
P = 2


def record_arrays(record):
    return {name: cpu(getattr(record, name)) for name in RECORDED if getattr(record, name) is not None}


def mark(record):
    """every cell of the record holds a value no act writes"""
    for name in RECORDED:
        t = getattr(record, name)
        if t is not None:
            t.fill_(MARK)
    return record


def make_sim(n):
    return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)


@functools.lru_cache(maxsize=None)
def member_params(layer_N, seed):
    """a member that has left its initialisation: no LayerNorm weight at 1, no bias at 0, heads of ordinary size"""
    torch.manual_seed(seed)
    module = MlpBaseActorCritic(layer_N=layer_N)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in module.named_parameters():
            noise = torch.randn(p.shape, generator=gen)
            p.add_((0.3 if name.endswith("action_out.linear.weight") else 0.05 if p.dim() == 2 else 0.2) * noise)
    return torch.nn.utils.parameters_to_vector(module.parameters()).detach().clone()


def make_bank(k, layer_N=2, first_seed=101):
    bank = MlpBasePolicyBank(k, layer_N, device=DEV)
    for i in range(k):
        bank.params[i].copy_(member_params(layer_N, first_seed + 2 * i))
    return bank


def synthetic(sim, seed):
    """positions 0..8 and 0..2 steps left in every cell of OBSERVATION (the observation is the beam's whole state)"""
    p, n, _ = sim.observation_tensor().shape
    rng = np.random.default_rng(seed)
    obs = rng.integers(0, 9, size=(p, n, 7)).astype(np.int32)
    obs[:, :, 6] = rng.integers(0, 3, size=(p, n))
    sim.observation_tensor().to_torch().copy_(torch.from_numpy(obs).to(DEV))


def one_act(sim, act, record):
    """``act(record)`` over a marked record and a marked ACTION tensor -> the arrays (``record`` None: ACTION alone)"""
    if record is not None:
        mark(record)
    sim.action_tensor().to_torch().fill_(ACTION_MARK)
    act(record)
    torch.cuda.synchronize()
    out = record_arrays(record) if record is not None else {}
    out["action_tensor"] = cpu(sim.action_tensor())
    return out


# ---------------------------------------------------------------- 1: a bank of one is the plain act

@pytest.mark.parametrize("layer_N", [1, 2])
@pytest.mark.parametrize("n", [1, 17, 257])  # 17 worlds are 34 cells, one past a tile
def test_bank_of_one_equals_the_plain_act(n, layer_N, hip_lib):
    t = 2
    sim = make_sim(n)
    synthetic(sim, 1000 + n)
    bank = make_bank(1, layer_N)
    ids = torch.zeros((n, P), dtype=torch.int32, device=DEV)
    ids_row = torch.full((n, P), 9, dtype=torch.int32, device=DEV)
    record = MlpBaseRecord(t, n, P, DEV, logits=True)
    assert record.obs is not None and record.logits is not None
    common = dict(seed=5 + n, step=3)
    for players in (0b11, 0b01, 0b10):
        for kwargs in ({}, {"greedy": True}):
            for r in (record, None):
                want = one_act(sim, lambda r: mlpbase_act(sim, bank.policy(0), players, r, row=1, **common, **kwargs), r)
                got = one_act(sim, lambda r: mlpbase_act_bank(sim, bank, ids, players, r, ids_row, row=1, **common, **kwargs), r)
                for name in want:
                    same_bits(got[name], want[name], f"K = 1, n = {n}, players {players}, {kwargs}, record {r is not None}: {name}")
                seats = np.array([(players >> s) & 1 for s in range(P)], dtype=bool)
                assert (got["action_tensor"][seats] >= 0).all() and (got["action_tensor"][~seats] == ACTION_MARK).all()
                same_bits(cpu(ids_row), np.where(seats[None, :], 0, -1).astype(np.int32).repeat(n, 0), "ids_row")
        # the closing value-only act at row T
        want = one_act(sim, lambda r: mlpbase_act(sim, bank.policy(0), players, r, row=t, value_only=True), record)
        got = one_act(sim, lambda r: mlpbase_act_bank(sim, bank, ids, players, r, None, row=t, value_only=True), record)
        for name in want:
            same_bits(got[name], want[name], f"K = 1, n = {n}, players {players}, closing: {name}")
        assert (got["action_tensor"] == ACTION_MARK).all() and (got["values"][t][:, seats] != MARK).all()
        assert (got["obs"][t][:, seats] != MARK).all() and (got["next_done"][:, seats] != MARK).all()
    sim.close()


# ---------------------------------------------------------------- 2 to 5: mixed assignments and the plan read back

def mixed_ids(n, k, players, counts, seed, beyond=True):
    """(N, P) int32: policy j acted in exactly counts[j] cells of the masked seats (None: every cell left over), one masked cell at
    k + 2 (outside the bank), a few at -1 and -7, the cells of other seats random valid ids (which must not be acted)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, k, size=(n, P)).astype(np.int32)
    seats = [s for s in range(P) if (players >> s) & 1]
    cells = rng.permutation(np.array([(w, s) for w in range(n) for s in seats]))
    at = 0
    for j, c in enumerate(counts):
        if c is None:
            continue
        for w, s in cells[at:at + c]:
            ids[w, s] = j
        at += c
    if beyond:
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


def spread_ids(n, k, seed):
    """every policy of a large bank somewhere: cell s under policy s mod k, shuffled, a few cells at -1"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(n * P) % k).astype(np.int32).reshape(n, P)
    ids[rng.uniform(size=(n, P)) < 0.02] = -1
    return ids


# key: (worlds, K, layer_N, players, ids, ids beyond the bank)
MIXED = {
    # 140 cells: policy 2 has no cell, policy 0 exactly a tile, policy 1 one more, cells at -1 and -7, one id beyond the bank
    "n70": (70, 5, 2, 0b11, lambda: mixed_ids(70, 5, 0b11, (32, 33, 0, None, 20), seed=70), 1),
    "n70_seat1": (70, 5, 1, 0b10, lambda: mixed_ids(70, 5, 0b10, (32, 1, 0, None, 3), seed=71), 1),
    # 600 cells over 256 policies, two or three each: nearly every tile is ragged
    "k256": (300, 256, 2, 0b11, lambda: spread_ids(300, 256, seed=300), 0),
    # 2050 cells: the first size of count, scan, place
    "n1025": (1025, 3, 2, 0b11, lambda: mixed_ids(1025, 3, 0b11, (33, None, 32), seed=1025), 1),
    # 2048 cells: the last size one workgroup plans
    "n1024": (1024, 3, 1, 0b11, lambda: mixed_ids(1024, 3, 0b11, (33, None, 32), seed=1024), 1),
}


@functools.lru_cache(maxsize=None)
def mixed_case(key):
    n, k, layer_N, players, make_ids, _ = MIXED[key]
    sim = make_sim(n)
    synthetic(sim, 77 + n)
    bank = make_bank(k, layer_N)
    ids_host = make_ids()
    ids = torch.from_numpy(ids_host).to(DEV)
    seed, step = 4242 + n, 9
    record = MlpBaseRecord(2, n, P, DEV, logits=True)
    used = sorted(set(int(j) for j in ids_host.reshape(-1) if 0 <= j < k))
    plain = {j: one_act(sim, lambda r, j=j: mlpbase_act(sim, bank.policy(j), players, r, row=1, seed=seed, step=step), record) for j in used}
    size = int(sim._L.mrl_cnn_bank_workspace_bytes(n, P, k))
    assert size == int(sim._L.mrl_mlpbase_bank_workspace_bytes(n, k))
    block = torch.full((size + 512,), 0xA5, dtype=torch.uint8, device=DEV)
    ids_row = torch.full((n, P), 9, dtype=torch.int32, device=DEV)
    got = one_act(sim, lambda r: mlpbase_act_bank(sim, bank, ids, players, r, ids_row, row=1, seed=seed, step=step,
                                                  workspace=block[256:256 + size]), record)
    again = one_act(sim, lambda r: mlpbase_act_bank(sim, bank, ids, players, r, None, row=1, seed=seed, step=step,
                                                    workspace=block[256:256 + size]), record)
    out = {"n": n, "k": k, "players": players, "ids": ids_host, "plain": plain, "got": got, "again": again, "ids_row": cpu(ids_row),
           "block": cpu(block), "size": size, "ids_after": cpu(ids)}
    sim.close()
    return out


def acted_mask(c):
    seat_in_mask = np.array([(c["players"] >> s) & 1 for s in range(P)], dtype=bool)[None, :]
    return seat_in_mask & (c["ids"] >= 0) & (c["ids"] < c["k"])


@pytest.mark.parametrize("key", sorted(MIXED))
def test_mixed_assignment_equals_plain_acts_selected_by_id(key, hip_lib):
    c = mixed_case(key)
    k, ids, beyond = c["k"], c["ids"], MIXED[key][5]
    acted = acted_mask(c)
    counts = np.bincount(ids[acted], minlength=k)
    if key == "n70":
        assert counts[0] == 32 and counts[1] == 33 and counts[2] == 0 and counts[3] > 0 and counts[4] == 20
    if key == "k256":
        assert (counts > 0).all() and counts.max() <= 3  # every tile but a few holds two or three rows
    assert (~acted).sum() > 0 and (ids[~acted] < 0).any() and (ids >= k).sum() == beyond
    for name in RECORDED:
        for row in range(c["got"][name].shape[0]) if name != "next_done" else [None]:
            got = c["got"][name] if row is None else c["got"][name][row]
            want = np.full_like(got, MARK)
            for j, plain in c["plain"].items():
                pick = acted & (ids == j)
                want[pick] = (plain[name] if row is None else plain[name][row])[pick]
            same_bits(got, want, f"{key}: {name} row {row}")
    # what an act at row 1 writes at all: the plain acts wrote it for their whole mask, so the selection above is not all marks
    g = c["got"]
    assert (g["actions"][1][acted] >= 0).all() and (g["values"][1][acted] != MARK).all() and (g["obs"][1][acted] != MARK).all()
    assert (g["rewards"][0][acted] != MARK).all() and (g["logits"][1][acted] != MARK).all() and (g["dones"][1][acted] != MARK).all()
    # un-acted cells keep every byte, the observation rows included
    for name in ("actions", "logprobs", "values", "dones", "logits", "obs"):
        assert (g[name][1][~acted] == MARK).all(), name
    # ACTION (P, N, 1): the acted cells' actions, every other entry untouched
    action = g["action_tensor"][:, :, 0].T
    same_bits(action[acted], g["actions"][1][acted], f"{key}: ACTION of acted cells")
    assert (action[~acted] == ACTION_MARK).all()
    # the members do differ: somewhere two policies give a cell different logits
    first, *others = sorted(c["plain"])
    assert any(not np.array_equal(c["plain"][first]["logits"][1], c["plain"][j]["logits"][1]) for j in others)
    # ids as the act used them; the caller's ids are read only; the same bits on a second run
    same_bits(c["ids_row"], np.where(acted, ids, -1).astype(np.int32), f"{key}: ids_row")
    same_bits(c["ids_after"], ids, f"{key}: ids")
    for name in g:
        same_bits(c["again"][name], g[name], f"{key}: second run, {name}")


@pytest.mark.parametrize("key", sorted(MIXED))
def test_plan_read_back(key, hip_lib):
    c = mixed_case(key)
    assert_plan_read_back(c["block"], c["size"], c["n"], P, c["k"], c["ids"], acted_mask(c), out_of_range=MIXED[key][5])


# ---------------------------------------------------------------- 6: the resample against its twin

def resample_start(n):
    """what both resample tests start from -> (rng, first, num, ids (N, 2) with a fifth of the cells at -1)"""
    rng = np.random.default_rng(3)
    first, num = [1, 3], [3, 1]  # seat 0 draws from {1, 2, 3}, seat 1 from {3}: a range of one
    ids_host = np.stack([rng.integers(1, 4, size=n), np.full(n, 3)], axis=1).astype(np.int32)
    ids_host[rng.uniform(size=(n, 2)) < 0.2] = -1
    return rng, first, num, ids_host


def resample_schedule(sim, n, rng):
    """The steps both resample tests run: eight times random actions and a step, yielding t behind each for the caller's resample."""
    late = torch.arange(n, device=DEV) % 3 == 0  # these worlds restart after step 2: their episodes are out of step with the others'
    for t in range(8):
        sim.action_tensor().to_torch().copy_(torch.from_numpy(rng.integers(0, 4, size=(2, n, 1)).astype(np.int32)).to(DEV))
        sim.step()
        if t == 1:
            sim.reset_worlds(late)
        yield t


def assert_mixed_done(seen, n, want_episodes):
    """``seen``: the worlds with DONE set behind each step"""
    assert 0 < min(x for x in seen if x) < n and (want_episodes > 40).all()  # DONE is a mix: some, not all, worlds finish at a time


@pytest.mark.parametrize("players", [0b11, 0b01])
@pytest.mark.parametrize("mode", ["robin", "random"])
def test_resample_against_the_twin(mode, players, hip_lib):
    n = 33
    sim = make_sim(n)
    rng, first, num, ids_host = resample_start(n)
    ids, episodes = torch.from_numpy(ids_host).to(DEV), torch.full((n,), 40, dtype=torch.int32, device=DEV)
    want_ids, want_episodes = ids_host.copy(), np.full(n, 40, np.int32)
    seen = []
    for t in resample_schedule(sim, n, rng):
        mlpbase_resample(sim, ids, episodes, mode, first, num, players=players, seed=11)
        torch.cuda.synchronize()
        done = cpu(sim.done_tensor()).reshape(-1)
        seen.append(int((done != 0).sum()))
        before = want_ids.copy()
        resample_twin(want_ids, want_episodes, done, mode, first, num, players, seed=11)
        same_bits(cpu(ids), want_ids, f"{mode}, step {t}: ids")
        same_bits(cpu(episodes), want_episodes, f"{mode}, step {t}: episodes")
        moved = want_ids != before
        assert not moved[done == 0].any() and not moved[before < 0].any()
        assert not moved[:, 1].any()  # a range of one, or a seat outside the mask
        if mode == "robin":  # three ids: the next one is another one
            assert (moved[:, 0] == ((done != 0) & (before[:, 0] >= 0))).all()
        live = want_ids[:, 0] >= 0
        assert ((want_ids[live, 0] >= 1) & (want_ids[live, 0] <= 3)).all()
    assert_mixed_done(seen, n, want_episodes)
    assert (want_ids < 0).sum() == (ids_host < 0).sum()
    # the descriptor may carry everything, under either name
    assert BankResample is CnnResample
    mlpbase_resample(sim, ids, episodes, BankResample(mode, first, num, 2, seed=11), players=players)
    torch.cuda.synchronize()
    resample_twin(want_ids, want_episodes, cpu(sim.done_tensor()).reshape(-1), mode, first, num, players, seed=11)
    same_bits(cpu(ids), want_ids, "through a descriptor: ids")
    sim.close()


@pytest.mark.parametrize("players", [0b11, 0b01])
@pytest.mark.parametrize("mode", ["robin", "random"])
def test_both_families_resample_the_beam_alike(mode, players, hip_lib):
    """The resamples of the three families are one path behind the family's own check of the game.  The balance beam is the one
    game two families play: ``mlpbase_resample`` and ``wide_resample`` from equal ids and episodes, behind the same steps, leave the
    same bytes, and these are ``resample_twin``'s.  The steps, the late reset and the demand on DONE are those of
    ``test_resample_against_the_twin``: neither "nobody finished" nor "everybody finished" passes."""
    n = 33
    sim = make_sim(n)
    rng, first, num, ids_host = resample_start(n)
    copies = {resample: (torch.from_numpy(ids_host).to(DEV), torch.full((n,), 40, dtype=torch.int32, device=DEV))
              for resample in (mlpbase_resample, wide_resample)}
    want_ids, want_episodes = ids_host.copy(), np.full(n, 40, np.int32)
    seen = []
    for t in resample_schedule(sim, n, rng):
        for resample, (ids, episodes) in copies.items():
            resample(sim, ids, episodes, mode, first, num, players=players, seed=11)
        torch.cuda.synchronize()
        done = cpu(sim.done_tensor()).reshape(-1)
        seen.append(int((done != 0).sum()))
        resample_twin(want_ids, want_episodes, done, mode, first, num, players, seed=11)
        for resample, (ids, episodes) in copies.items():
            same_bits(cpu(ids), want_ids, f"{resample.__name__}, {mode}, step {t}: ids")
            same_bits(cpu(episodes), want_episodes, f"{resample.__name__}, {mode}, step {t}: episodes")
    assert_mixed_done(seen, n, want_episodes)
    assert (want_ids != ids_host).any() and (want_ids < 0).sum() == (ids_host < 0).sum()
    sim.close()


# ---------------------------------------------------------------- 7: the rollout against the hand-issued loop

ROLLOUT = dict(n=33, t=12, k=3, seed=21, first_step=100)


def rollout_ids(n):
    """seat 0 of world n starts under n mod 3, seat 1 under (n + 1) mod 3; two cells are never acted"""
    ids = torch.stack([torch.arange(n) % 3, (torch.arange(n) + 1) % 3], dim=1).to(torch.int32)
    ids[4, 0] = ids[9, 1] = -1
    return ids.to(DEV).contiguous()


def final_state(env):
    return {"observation": cpu(env.static_observations), "action_tensor": cpu(env.static_actions), "done": cpu(env.static_dones),
            "reward": cpu(env.static_rewards)}


def start_env(n):
    """a fresh env whose two never-acted cells hold an action that is theirs for the whole run"""
    env = BalanceMadronaTorch(n, 0)
    env.static_actions.fill_(2)
    return env


@functools.lru_cache(maxsize=None)
def rollout_case(mode, pieces=1):
    """one rollout of T, or ``pieces`` chained ones of T / pieces with their records put together"""
    r = ROLLOUT
    env = start_env(r["n"])
    bank = make_bank(r["k"])
    ids, episodes = rollout_ids(r["n"]), torch.zeros(r["n"], dtype=torch.int32, device=DEV)
    resample = CnnResample(mode, [0, 1], [3, 2], 2, seed=r["seed"]) if mode else None
    t = r["t"] // pieces
    parts = []
    for piece in range(pieces):
        record, ids_record = env.rollout_bank(bank, ids, t, episodes=episodes, resample=resample, seed=r["seed"],
                                              first_step=r["first_step"] + piece * t, record=MlpBaseRecord(t, r["n"], 2, DEV, logits=True))
        torch.cuda.synchronize()
        parts.append((record_arrays(record), cpu(ids_record)))
    out = {name: np.concatenate([part[0][name][:t] for part in parts]) for name in ("actions", "logprobs", "rewards", "dones", "logits")}
    for name in ("values", "obs"):
        out[name] = np.concatenate([part[0][name][:t] for part in parts] + [parts[-1][0][name][t:]])
    out["next_done"] = parts[-1][0]["next_done"]
    out["ids_record"] = np.concatenate([part[1][:t] for part in parts] + [parts[-1][1][t:]])
    out["ids"], out["episodes"] = cpu(ids), cpu(episodes)
    out["final"] = final_state(env)
    env.close()
    return out


@functools.lru_cache(maxsize=None)
def hand_case(mode):
    """the same as calls: act_bank, step, resample, T times; the closing value-only act"""
    r = ROLLOUT
    n, t = r["n"], r["t"]
    env = start_env(n)
    bank = make_bank(r["k"])
    ids, episodes = rollout_ids(n), torch.zeros(n, dtype=torch.int32, device=DEV)
    record = MlpBaseRecord(t, n, 2, DEV, logits=True)
    ids_record = torch.empty((t + 1, n, 2), dtype=torch.int32, device=DEV)
    for k in range(t):
        env.act_bank(bank, ids, record=record, ids_row=ids_record[k], row=k, seed=r["seed"], step=r["first_step"] + k)
        env.sim.step()
        if mode:
            mlpbase_resample(env.sim, ids, episodes, mode, [0, 1], [3, 2], seed=r["seed"])
    mlpbase_act_bank(env.sim, bank, ids, None, record, ids_record[t], row=t, value_only=True)
    torch.cuda.synchronize()
    out = record_arrays(record)
    out.update(ids_record=cpu(ids_record), ids=cpu(ids), episodes=cpu(episodes), final=final_state(env))
    env.close()
    return out


def assert_same_rollout(got, want, what):
    for name in tuple(RECORDED) + ("ids_record", "ids", "episodes"):
        same_bits(got[name], want[name], f"{what}: {name}")
    for name in want["final"]:
        same_bits(got["final"][name], want["final"][name], f"{what}: the simulator's {name}")


@pytest.mark.parametrize("mode", ["robin", "random"])
def test_rollout_bank_equals_the_hand_issued_loop(mode, hip_lib):
    got, want = rollout_case(mode), hand_case(mode)
    t = ROLLOUT["t"]
    assert_same_rollout(got, want, f"rollout against calls, {mode}")
    # it is a test of something: episodes end (at least six per world in twelve steps), ids move, acted cells only are recorded
    assert (got["episodes"] >= 6).all() and not np.array_equal(got["ids_record"][0], got["ids_record"][t])
    assert (got["ids_record"][:, 4, 0] == -1).all() and (got["ids_record"][:, 9, 1] == -1).all() and (got["ids_record"] >= 0).sum() > 0
    assert ((got["ids_record"][:, :, 0] <= 2) & (got["ids_record"][:, :, 1] <= 2)).all()
    assert (got["ids_record"][4:, [0, 1, 2], 1] >= 1).all()  # seat 1 draws from {1, 2} once its first episode is over
    assert not got["values"][:, 4, 0].any() and not got["actions"][:, 9, 1].any() and not got["obs"][:, 4, 0].any()  # started at zero
    # the rows' ids are the resample twin's
    ids, episodes = cpu(rollout_ids(ROLLOUT["n"])), np.zeros(ROLLOUT["n"], np.int32)
    for k in range(t):
        same_bits(got["ids_record"][k], ids, f"ids_record[{k}] against the twin")
        done = got["dones"][k + 1] if k + 1 < t else got["next_done"]  # DONE behind step k, in the columns of acted cells
        resample_twin(ids, episodes, done.max(axis=1), mode, [0, 1], [3, 2], 0b11, seed=ROLLOUT["seed"])
    same_bits(got["ids"], ids, "ids after the rollout against the twin")
    same_bits(got["episodes"], episodes, "episodes after the rollout against the twin")


@pytest.mark.parametrize("mode", ["robin", "random"])
def test_two_chained_bank_rollouts_equal_one(mode, hip_lib):
    assert_same_rollout(rollout_case(mode, pieces=2), rollout_case(mode), f"two rollouts of 6 against one of 12, {mode}")


def test_bank_of_one_rollout_equals_the_plain_rollout(hip_lib):
    r = ROLLOUT
    n, t = r["n"], r["t"]
    runs = []
    for banked in (False, True):
        env = BalanceMadronaTorch(n, 0)
        bank = make_bank(1)
        record = MlpBaseRecord(t, n, 2, DEV, logits=True)
        if banked:
            ids = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
            _, ids_record = env.rollout_bank(bank, ids, t, seed=r["seed"], first_step=r["first_step"], record=record)
            assert not cpu(ids_record).any() and not cpu(ids).any()
        else:
            env.rollout(bank.policy(0), t, seed=r["seed"], first_step=r["first_step"], record=record)
        torch.cuda.synchronize()
        runs.append(dict(record_arrays(record), final=final_state(env)))
        env.close()
    for name in RECORDED:
        same_bits(runs[1][name], runs[0][name], f"K = 1 rollout against mrl_rollout_mlpbase: {name}")
    for name in runs[0]["final"]:
        same_bits(runs[1]["final"][name], runs[0]["final"][name], f"K = 1 rollout against mrl_rollout_mlpbase: the simulator's {name}")
    assert runs[0]["dones"].any() and runs[0]["rewards"].any()


# ---------------------------------------------------------------- 8: the population agent

def test_population_agent_reproduces_the_rollout(hip_lib):
    """seat 1 is an MlpBasePopulationAgent inside VectorMultiAgentEnv.step, seat 0 the same calls by hand: test 7's ids and actions"""
    r = ROLLOUT
    n, t, mode = r["n"], r["t"], "random"
    want = rollout_case(mode)
    env = start_env(n)
    bank = make_bank(r["k"])
    partner = MlpBasePopulationAgent(env, bank, members=[1, 2], resample=mode, seed=r["seed"])
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
        mlpbase_act_bank(env.sim, bank, ego_ids, 0b01, seed=r["seed"], step=r["first_step"] + k)
        env.step(env.static_actions[0].clone())
        torch.cuda.synchronize()
        acted = want["ids_record"][k] >= 0
        same_bits(cpu(env.static_actions)[:, :, 0].T[acted], want["actions"][k][acted], f"step {k}: actions")
        mlpbase_resample(env.sim, ego_ids, ego_episodes, mode, [0, 1], [3, 2], players=0b01, seed=r["seed"])
    same_bits(cpu(partner.ids)[:, 1], want["ids"][:, 1], "the partner's ids at the end")
    same_bits(cpu(partner.episodes), want["episodes"], "the partner's episode counts")
    assert (cpu(partner.ids)[:, 0] == -1).all()
    env.close()
    # defaults: world n starts with members[n % len(members)], the other seat's column is -1
    env = BalanceMadronaTorch(7, 0)
    agent = MlpBasePopulationAgent(env, bank, members=[2, 0], resample=None)
    env.add_partner_agent(agent)
    agent.get_action()
    agent.update(None, None)
    assert cpu(agent.ids).tolist() == [[-1, 2], [-1, 0]] * 3 + [[-1, 2]] and not cpu(agent.episodes).any()
    with pytest.raises(ValueError, match="consecutive"):
        MlpBasePopulationAgent(env, bank, members=[2, 0], resample="robin")
    with pytest.raises(TypeError, match="no torch fallback"):
        MlpBasePopulationAgent(object(), bank)
    env.close()


# ---------------------------------------------------------------- 9: cross-play

def test_cross_play_matches_the_hand_loop(hip_lib):
    k, n, steps, seed = 3, 9 * 4, 12, 3
    bank = make_bank(k)
    env = BalanceMadronaTorch(n, 0)
    result = cross_play(env, bank, greedy=False, seed=seed)  # the default: twelve steps
    torch.cuda.synchronize()
    mean_return, episodes = cpu(result.mean_return), cpu(result.episodes)
    env.close()
    # by hand on a twin simulator: ACTION composed from three plain acts by id, the same accumulation
    sim = make_sim(n)
    sim.enable_episode_stats()
    sim.reset_worlds(None)
    pair = np.arange(n) % (k * k)
    ids = np.stack([pair // k, pair % k], axis=1)  # (N, P)
    total, finished = np.zeros(n, np.float64), np.zeros(n, np.int64)
    for t in range(steps):
        composed = np.full((P, n, 1), ACTION_MARK, np.int32)
        for j in range(k):
            mlpbase_act(sim, bank.policy(j), None, seed=seed, step=t)
            torch.cuda.synchronize()
            under_j = cpu(sim.action_tensor())
            composed[ids.T == j] = under_j[ids.T == j]
        assert (composed >= 0).all()
        sim.action_tensor().to_torch().copy_(torch.from_numpy(composed).to(DEV))
        sim.step()
        torch.cuda.synchronize()
        over = cpu(sim.done_tensor()).reshape(n) != 0
        last = cpu(sim.last_episode_return_tensor()).reshape(P, n)[0]
        assert last.dtype == np.float32
        total += np.where(over, last.astype(np.float64), 0.0)
        finished += over
    sim.close()
    want_count = np.bincount(pair, weights=finished, minlength=k * k).astype(np.int64).reshape(k, k)
    want_sum = np.array([total[pair == q].sum() for q in range(k * k)]).reshape(k, k)
    assert mean_return.shape == (k, k) and mean_return.dtype == np.float64 and episodes.dtype == np.int64
    same_bits(episodes, want_count, "finished episodes per pair")
    same_bits(mean_return, want_sum / want_count, "mean return per pair")
    assert (episodes >= 4 * 6).all()  # four worlds per pair, an episode lasts at most two steps
    assert len(np.unique(mean_return)) > 1  # the pairs do not all play alike
    # members and steps
    env = BalanceMadronaTorch(n, 0)
    small = cross_play(env, bank, members_a=[2], members_b=[0, 1], steps=3)
    assert tuple(small.mean_return.shape) == (1, 2) and (cpu(small.episodes) >= n // 2).all()
    env.close()
    env = BalanceMadronaTorch(3, 0)
    with pytest.raises(ValueError, match="cannot play"):
        cross_play(env, bank)
    env.close()


# ---------------------------------------------------------------- 10 and 11: training a member, the ego's advantages

@functools.lru_cache(maxsize=None)
def training_record():
    """a rollout of bank member 1 (seat 0) against members 0 and 2 (seat 1): the record, the bank's parameters at that time"""
    n, t = 33, 6
    env = BalanceMadronaTorch(n, 0)
    bank = make_bank(3)
    ids = torch.stack([torch.ones(n), (torch.arange(n) % 2) * 2], dim=1).to(torch.int32).to(DEV).contiguous()
    record, _ = env.rollout_bank(bank, ids, t, seed=8)
    torch.cuda.synchronize()
    env.close()
    return record, bank.params.clone()


def test_update_through_a_view_moves_its_row_only(hip_lib):
    record, start = training_record()
    n, t = record.num_worlds, record.num_steps
    bank = MlpBasePolicyBank(3, device=DEV)
    bank.params.copy_(start)
    alone = MlpBasePolicy(device=DEV)
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
            stats.append(cpu(mappo_update(policy, optimizer, record, None, advantages, returns, indices, value_norm=value_norm).stats))
    torch.cuda.synchronize()
    after = cpu(bank.params)
    same_bits(after[0], cpu(start)[0], "row 0")
    same_bits(after[2], cpu(start)[2], "row 2")
    same_bits(after[1], cpu(alone.params), "row 1 against the same update on a stand-alone copy")
    assert not np.array_equal(after[1], cpu(start)[1])
    same_bits(stats[0], stats[2], "stats of the first update")
    same_bits(stats[1], stats[3], "stats of the second update")
    # the member's module reads the updated row
    module = bank.policy(1).module()
    same_bits(cpu(torch.nn.utils.parameters_to_vector(module.parameters()).detach()), after[1], "the member's module")


def test_advantages_over_the_ego_seat(hip_lib):
    record, _ = training_record()
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
    whole, _ = mappo_advantages(record, None)
    assert float((whole[:, :, 0] - ego).abs().max()) > 1e-4  # and differs: the partner's critics are other nets


# ---------------------------------------------------------------- 12: refusals

def test_refusals_enqueue_nothing(hip_lib):
    n, t, k = 33, 2, 3
    L = _lib.lib()
    sim = make_sim(n)
    bank = make_bank(k)
    record = mark(MlpBaseRecord(t, n, P, DEV, logits=True))
    sim.action_tensor().to_torch().fill_(ACTION_MARK)
    size = int(L.mrl_mlpbase_bank_workspace_bytes(n, k))
    assert size == int(L.mrl_cnn_bank_workspace_bytes(n, P, k)) > 0
    ws = torch.full((size + 16,), 0xA5, dtype=torch.uint8, device=DEV)
    ids = torch.ones((n, P), dtype=torch.int32, device=DEV)
    episodes = torch.full((n,), 5, dtype=torch.int32, device=DEV)
    ids_record = torch.full((t + 1, n, P), 9, dtype=torch.int32, device=DEV)
    sim.done_tensor().to_torch().fill_(1)  # a resample that ran would move every id
    good, rec = bank.desc(), record.struct
    first, num = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(3, 3)
    fine = _lib.CnnResampleDesc(1, first, num, 0)

    def desc(params=bank.params.data_ptr(), count=k, stride=bank.num_params, hidden=64, layer_N=2, flags=0):
        return _lib.MlpBaseBankDesc(params, count, stride, hidden, layer_N, flags)

    def act(handle=None, players=3, d=good, ids_ptr=None, r=rec, row=0, flags=0, workspace=None, wsize=None):
        return L.mrl_mlpbase_act_bank(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                      ids.data_ptr() if ids_ptr is None else ids_ptr, ctypes.byref(r) if r is not None else None, None, row,
                                      1, 0, flags, ws.data_ptr() if workspace is None else workspace, size if wsize is None else wsize, None)

    def resample(handle=None, players=3, d=fine, ids_ptr=None, episodes_ptr=None):
        return L.mrl_mlpbase_bank_resample(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                           ids.data_ptr() if ids_ptr is None else ids_ptr,
                                           episodes.data_ptr() if episodes_ptr is None else episodes_ptr, None)

    def rollout(handle=None, players=3, d=good, ids_ptr=None, episodes_ptr=None, again=fine, r=rec, wsize=None):
        return L.mrl_rollout_mlpbase_bank(sim._handle if handle is None else handle, players, ctypes.byref(d) if d is not None else None,
                                          ids.data_ptr() if ids_ptr is None else ids_ptr,
                                          episodes.data_ptr() if episodes_ptr is None else episodes_ptr,
                                          ctypes.byref(again) if again is not None else None, ctypes.byref(r) if r is not None else None,
                                          ids_record.data_ptr(), 1, 0, ws.data_ptr(), size if wsize is None else wsize, None)

    def sampler(mode=1, first_id=(0, 0), num_ids=(3, 3), null=False):
        f, m = (ctypes.c_uint32 * 2)(*first_id), (ctypes.c_uint32 * 2)(*num_ids)
        keep.append((f, m))
        return _lib.CnnResampleDesc(mode, None if null else f, m, 0)

    keep = []
    other = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    holes = _lib.MlpBaseRecordDesc(*[None if name == "values" else getattr(record, name).data_ptr() for name in RECORDED], t)
    no_obs = _lib.MlpBaseRecordDesc(*[None if name == "obs" else getattr(record, name).data_ptr() for name in RECORDED], t)
    refused = [
        act(handle=other._handle), rollout(handle=other._handle), resample(handle=other._handle),  # not the balance beam
        act(d=None), rollout(d=None), act(d=desc(params=None)), act(d=desc(hidden=128)), act(d=desc(flags=2)),
        act(d=desc(layer_N=0)), act(d=desc(layer_N=3)), rollout(d=desc(layer_N=3)),
        act(d=desc(count=0)), act(d=desc(count=257)), rollout(d=desc(count=0)), rollout(d=desc(count=257)),
        act(d=desc(stride=bank.num_params - 1)), rollout(d=desc(stride=0)),
        act(d=desc(layer_N=1, stride=int(L.mrl_mlpbase_policy_num_params(7, 64, 1, 4)) - 1)),
        act(ids_ptr=0), rollout(ids_ptr=0), resample(ids_ptr=0), resample(episodes_ptr=0), rollout(episodes_ptr=0),
        act(players=0), act(players=4), rollout(players=0), resample(players=0), resample(players=4),
        act(r=holes), act(r=no_obs), rollout(r=holes), rollout(r=None),
        act(row=t), act(row=t - 1, flags=_lib.MLPBASE_VALUE_ONLY), act(r=None, row=t, flags=_lib.MLPBASE_VALUE_ONLY), act(flags=8),
        act(workspace=0), act(workspace=ws.data_ptr() + 8), act(wsize=size - 1), rollout(wsize=size - 1),
        resample(d=None), resample(d=sampler(mode=0)), resample(d=sampler(mode=3)), resample(d=sampler(null=True)),
        resample(d=sampler(num_ids=(3, 0))), resample(d=sampler(first_id=(0, 255), num_ids=(3, 2))), resample(d=sampler(num_ids=(257, 1))),
        rollout(again=sampler(num_ids=(0, 3))), rollout(again=sampler(mode=7)),
    ]
    assert refused == [_lib.MRL_ERR_INVALID] * len(refused), refused
    # a seat outside `players` may carry any range: it is not read
    nobody = torch.full((n, P), -1, dtype=torch.int32, device=DEV)
    assert resample(players=1, d=sampler(num_ids=(3, 0)), ids_ptr=nobody.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (cpu(nobody) == -1).all() and (cpu(episodes) == 6).all()
    episodes.fill_(5)
    # the Python layer's own refusals
    with pytest.raises(ValueError):
        mlpbase_act_bank(sim, bank, ids.to(torch.int64))
    with pytest.raises(ValueError):
        mlpbase_act_bank(sim, bank, ids[:-1])
    with pytest.raises(ValueError):
        mlpbase_act_bank(sim, bank.policy(0), ids)
    with pytest.raises(ValueError):
        mlpbase_act_bank(other, bank, ids)
    with pytest.raises(ValueError):
        mlpbase_resample(sim, ids, episodes.to(torch.int64), "robin", 0, 3)
    with pytest.raises(ValueError):
        mlpbase_resample(other, ids, episodes, "robin", 0, 3)
    with pytest.raises(ValueError):
        sim.rollout_mlpbase_bank(bank, ids, record, resample=CnnResample("robin", 0, 3, 2))  # no episodes
    # a capturing stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                mlpbase_act_bank(sim, bank, ids, None, record, row=0, workspace=ws[:size])
            scratch.add_(0)
    torch.cuda.synchronize()
    # nothing was enqueued
    for name, value in record_arrays(record).items():
        assert (value == MARK).all(), name
    assert (cpu(sim.action_tensor()) == ACTION_MARK).all() and (cpu(ws) == 0xA5).all()
    assert (cpu(ids) == 1).all() and (cpu(episodes) == 5).all() and (cpu(ids_record) == 9).all()
    # and the simulator still acts, steps and resamples
    mlpbase_act_bank(sim, bank, ids, None, record, row=0, workspace=ws[:size])
    sim.step()
    sim.done_tensor().to_torch().fill_(1)
    mlpbase_resample(sim, ids, episodes, "robin", 0, 3)
    torch.cuda.synchronize()
    assert (cpu(record.actions)[0] >= 0).all() and (cpu(ids) == 2).all() and (cpu(episodes) == 6).all()
    other.close()
    sim.close()
