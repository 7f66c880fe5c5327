"""GPU: training every member of a policy bank in one call -- ``mappo_update_bank`` (``mrl_mappo_bank_update`` for the kitchens' CNN
bank, ``mrl_mappo_mlp_bank_update`` for the balance beam's MLP bank), ``mappo_advantages_bank`` and the closed loop around them
(DESIGN.md section 22).

The contract is bit-for-bit equality with the plain call, no tolerance: for every trained member z its row of the bank, both moment
rows, its ValueNorm row, ``stats[z]`` and ``grads[z]`` are what ``mappo_update`` leaves on a copy of the bank for
``bank_copy.policy(first + z)`` with a ``MappoOptimizer`` at the same step, a ``ValueNorm`` in the same state, the same record, ring,
advantages and returns and ``indices[z]``.  Every case runs on the beam with ``layer_N`` 1 and 2 and on ``cramped_room``, except the
one beyond the cap on partial vectors (beam only).  The records are real bank rollouts (world n under member n mod K, both seats);
advantages and returns are planted so that the members' gradient norms differ by orders of magnitude."""
import ctypes
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs import OvercookedMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnActorCritic, CnnPolicyBank, CnnRecord, MappoBankOptimizer, MappoOptimizer,  # noqa: E402
                                                         MlpBaseActorCritic, MlpBasePolicyBank, MlpBaseRecord, ValueNorm, ValueNormBank,
                                                         cnn_act, mappo_advantages, mappo_advantages_bank, mappo_update,
                                                         mappo_update_bank, member_samples, mlpbase_act)

DEV = torch.device("cuda", 0)
STAT = _lib.MAPPO_STATS.index
KINDS = ("beam1", "beam2", "kitchen")
K, N, T, P = 4, 12, 8, 2          # the shared records: four members, three worlds each
HORIZON = 5                      # the kitchen's episodes end inside the record
MAX_GRAD_NORM = 1.0
LOUD, QUIET = 1, 2                # the member whose two gradient norms are far above MAX_GRAD_NORM, and the one far below
# a ValueNorm row (running_mean, running_mean_sq, debiasing_term = 1): mean m, variance s^2
VN_MEAN, VN_STD = (0.0, 0.4, -0.3, 0.2), (1.0, 1.5, 0.8, 1.2)


def cpu(tensor):
    return tensor.detach().cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def is_beam(kind):
    return kind.startswith("beam")


def make_env(kind, n):
    return BalanceMadronaTorch(n, 0) if is_beam(kind) else OvercookedMadrona("cramped_room", n, 0, horizon=HORIZON)


def make_bank(kind, env, members, seed=100):
    """``members`` policies of the env's shape: the reference's initialisation under seeds ``seed``, ``seed`` + 1, ..."""
    if is_beam(kind):
        layer_N = int(kind[-1])
        bank, module = MlpBasePolicyBank(members, layer_N, device=DEV), lambda: MlpBaseActorCritic(layer_N=layer_N)
    else:
        _, _, height, width, channels = env.static_world_major_observations.shape
        bank, module = CnnPolicyBank(width, height, channels, members, device=DEV), lambda: CnnActorCritic(width, height, channels)
    with torch.no_grad():
        for k in range(members):
            torch.manual_seed(seed + k)
            bank.params[k].copy_(torch.nn.utils.parameters_to_vector(module().parameters()))
    return bank


def owner_table(n, members):
    return (torch.arange(n, device=DEV) % members).view(n, 1).expand(n, P).to(torch.int32).contiguous()


def bank_rollout(kind, env, bank, owner, steps, seed, first_step=0):
    """-> (record, ring or None)"""
    if is_beam(kind):
        record, _ = env.rollout_bank(bank, owner, steps, seed=seed, first_step=first_step)
        return record, None
    record, ring, _ = env.rollout_bank(bank, owner, steps, seed=seed, first_step=first_step)
    return record, ring


class World:
    """What the update cases share, made once per kind and never changed: a bank's parameters, the record (and ring) of one bank
    rollout under it, planted advantages and returns, the members' samples, starting moments and ValueNorm rows."""

    def __init__(self, kind):
        self.kind = kind
        env = make_env(kind, N)
        bank = make_bank(kind, env, K)
        self.shape = {name: getattr(bank, name) for name in bank._shape}
        self.params = bank.params.clone()
        self.owner = owner_table(N, K)
        self.record, self.ring = bank_rollout(kind, env, bank, self.owner, T, seed=7)
        env.close()
        self.cells = member_samples(self.owner, range(K), T)  # (K, 48)
        gen = torch.Generator().manual_seed(5)
        own = self.owner.view(1, N, P).expand(T, N, P)
        mean = torch.tensor(VN_MEAN, device=DEV)[own.long()]
        std = torch.tensor(VN_STD, device=DEV)[own.long()]
        noise = torch.randn((T, N, P), generator=gen).to(DEV)
        # every member's returns are its recorded values in its own ValueNorm scale plus noise: far outside Huber's delta for LOUD,
        # nothing for QUIET (its normalised targets are its values up to the one-in-10^5 move of the running statistics per row)
        spread = torch.where(own == LOUD, 40.0, torch.where(own == QUIET, 0.0, 1.0)).to(DEV)
        self.returns = (self.record.values[:T] * std + mean + spread * std * (noise.sign() + 0.1 * noise)).contiguous()
        scale = torch.where(own == LOUD, 100.0, torch.where(own == QUIET, 1e-3, 1.0)).to(DEV)
        self.advantages = (scale * torch.randn((T, N, P), generator=gen).to(DEV)).contiguous()
        self.exp_avg = (1e-3 * torch.randn(self.params.shape, generator=gen)).to(DEV)
        self.exp_avg_sq = (1e-6 * torch.rand(self.params.shape, generator=gen)).to(DEV)
        self.vn_state = torch.tensor([[m, m * m + s * s, 1.0] for m, s in zip(VN_MEAN, VN_STD)], dtype=torch.float32, device=DEV)
        self.step = 5
        torch.cuda.synchronize()

    def bank(self):
        """a fresh bank holding the world's parameters"""
        cls = MlpBasePolicyBank if is_beam(self.kind) else CnnPolicyBank
        bank = cls(num_policies=K, device=DEV, **self.shape)
        bank.params.copy_(self.params)
        return bank

    def rows(self, members, rows, width, seed):
        """int32 (M, rows, width): samples of each member's own cells, drawn with replacement (``width`` may exceed the record)"""
        gen = torch.Generator().manual_seed(seed)
        picks = torch.randint(0, self.cells.shape[1], (len(members), rows * width), generator=gen).to(DEV)
        return self.cells[list(members)].gather(1, picks).view(len(members), rows, width).contiguous()


@functools.lru_cache(maxsize=None)
def world(kind):
    return World(kind)


def state_of(bank, exp_avg, exp_avg_sq, vn_state):
    torch.cuda.synchronize()
    return {"params": cpu(bank.params), "exp_avg": cpu(exp_avg), "exp_avg_sq": cpu(exp_avg_sq), "value_norm": cpu(vn_state)}


def run_bank(w, indices, first, norm=True, bank=None, step=None, **options):
    """one ``mappo_update_bank`` from the world's starting state -> (stats, grads, state, optimizer)"""
    bank = w.bank() if bank is None else bank
    optimizer = MappoBankOptimizer(bank)
    optimizer.exp_avg.copy_(w.exp_avg)
    optimizer.exp_avg_sq.copy_(w.exp_avg_sq)
    optimizer.step = w.step if step is None else step
    norms = ValueNormBank(K, DEV)
    norms.state.copy_(w.vn_state)
    result = mappo_update_bank(bank, optimizer, w.record, w.ring, w.advantages, w.returns, indices, norms if norm else None, first_member=first,
                               max_grad_norm=MAX_GRAD_NORM, stats=True, grads=True, **options)
    return cpu(result.stats), cpu(result.grads), state_of(bank, optimizer.exp_avg, optimizer.exp_avg_sq, norms.state), optimizer


def run_plain(w, indices, first, norm=True, bank=None):
    """the same members one after another through the plain ``mappo_update`` on a copy of the bank: each through its view of the
    bank, a ``MappoOptimizer`` at the same step with the member's moments, a ``ValueNorm`` in the member's state"""
    bank = w.bank() if bank is None else bank
    exp_avg, exp_avg_sq, vn_state = w.exp_avg.clone(), w.exp_avg_sq.clone(), w.vn_state.clone()
    stats, grads = [], []
    for z in range(indices.shape[0]):
        k = first + z
        policy = bank.policy(k)
        optimizer = MappoOptimizer(policy)
        optimizer.exp_avg.copy_(exp_avg[k])
        optimizer.exp_avg_sq.copy_(exp_avg_sq[k])
        optimizer.step = w.step
        value_norm = ValueNorm(DEV)
        value_norm.state.copy_(vn_state[k])
        result = mappo_update(policy, optimizer, w.record, w.ring, w.advantages, w.returns, indices[z].contiguous(),
                              value_norm=value_norm if norm else None, max_grad_norm=MAX_GRAD_NORM, stats=True, grads=True)
        assert optimizer.step == w.step + indices.shape[1]
        exp_avg[k].copy_(optimizer.exp_avg)
        exp_avg_sq[k].copy_(optimizer.exp_avg_sq)
        vn_state[k].copy_(value_norm.state)
        stats.append(cpu(result.stats))
        grads.append(cpu(result.grads))
    return np.stack(stats), np.stack(grads), state_of(bank, exp_avg, exp_avg_sq, vn_state)


def assert_same_update(got, want, what):
    same_bits(got[0], want[0], f"{what}: stats")
    same_bits(got[1], want[1], f"{what}: grads")
    for name, value in want[2].items():
        same_bits(got[2][name], value, f"{what}: {name}")


# ---------------------------------------------------------------- 1: members equal plain calls

@pytest.mark.parametrize("kind", KINDS)
def test_members_equal_plain_calls(hip_lib, kind):
    w = world(kind)
    first, members, rows, width = 1, 2, 3, 33  # one full tile and a ragged one
    assert (first, first + 1) == (LOUD, QUIET)
    indices = w.rows(range(first, first + members), rows, width, seed=11)
    before = state_of(w.bank(), w.exp_avg, w.exp_avg_sq, w.vn_state)
    got = run_bank(w, indices, first)
    want = run_plain(w, indices, first)
    assert got[3].step == w.step + rows
    assert got[0].shape == (members, rows, 8) and got[1].shape == (members, rows, w.params.shape[1])
    assert_same_update(got[:3], want, kind)
    # clipping was engaged for LOUD on both nets in every row and for neither net of QUIET
    stats = got[0]
    for name in ("actor_grad_norm", "critic_grad_norm"):
        print(kind, name, "LOUD", stats[0][:, STAT(name)], "QUIET", stats[1][:, STAT(name)])
        assert (stats[0][:, STAT(name)] > 2 * MAX_GRAD_NORM).all() and (stats[1][:, STAT(name)] < MAX_GRAD_NORM / 2).all()
    assert np.isfinite(stats).all() and np.isfinite(got[1]).all()
    # it is a test of something: the trained rows moved, each ValueNorm row moved
    after = got[2]
    for k in (first, first + 1):
        for name in after:
            assert not np.array_equal(after[name][k], before[name][k]), (name, k)
    # rows 0 and 3, their moments and their ValueNorm rows keep every bit
    for k in (0, 3):
        for name in after:
            same_bits(after[name][k], before[name][k], f"{kind}: {name} of untrained row {k}")


# ---------------------------------------------------------------- 2: one member at row 0 is the plain update

@pytest.mark.parametrize("norm", [True, False], ids=["valuenorm", "no_valuenorm"])
@pytest.mark.parametrize("kind", KINDS)
def test_one_member_at_row_zero_is_the_plain_update(hip_lib, kind, norm):
    w = world(kind)
    indices = w.rows([0], 3, 33, seed=13)
    before = state_of(w.bank(), w.exp_avg, w.exp_avg_sq, w.vn_state)
    got = run_bank(w, indices, 0, norm=norm)
    want = run_plain(w, indices, 0, norm=norm)
    assert_same_update(got[:3], want, f"{kind}, M = 1")
    assert not np.array_equal(got[2]["params"][0], before["params"][0])
    if not norm:
        same_bits(got[2]["value_norm"], before["value_norm"], "the ValueNorm rows without a ValueNormBank")
    for name in before:
        same_bits(got[2][name][1:], before[name][1:], f"{kind}: {name} of the other rows")


# ---------------------------------------------------------------- 3: beyond the cap on partial vectors

@pytest.mark.parametrize("layer_N", [1, 2])
def test_beyond_the_cap_on_partial_vectors(hip_lib, layer_N):
    w = world(f"beam{layer_N}")
    width = 256 * 32 + 33  # 258 tiles over 256 workgroups: two tiles each, so 129 workgroups per net and member
    indices = w.rows([2, 3], 1, width, seed=17)
    got = run_bank(w, indices, 2)
    want = run_plain(w, indices, 2)
    assert_same_update(got[:3], want, f"layer_N {layer_N}, B = {width}")
    here, far = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, layer_N, 4, width, 1, 2, ctypes.byref(here)) == 0
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, layer_N, 4, 2 ** 30, 1, 2, ctypes.byref(far)) == 0
    assert here.value == far.value


# ---------------------------------------------------------------- 4: R rows at once, and a second run

@pytest.mark.parametrize("kind", KINDS)
def test_rows_in_one_call_equal_calls_of_one_row_and_runs_repeat(hip_lib, kind):
    w = world(kind)
    first, members, rows = 0, 3, 3
    indices = w.rows(range(members), rows, 33, seed=19)
    whole = run_bank(w, indices, first)
    again = run_bank(w, indices, first)
    assert_same_update(again[:3], whole[:3], f"{kind}: a second run")
    # row by row on one bank, optimizer and ValueNormBank
    bank = w.bank()
    optimizer = MappoBankOptimizer(bank)
    optimizer.exp_avg.copy_(w.exp_avg)
    optimizer.exp_avg_sq.copy_(w.exp_avg_sq)
    optimizer.step = w.step
    norms = ValueNormBank(K, DEV)
    norms.state.copy_(w.vn_state)
    stats, grads = [], []
    for r in range(rows):
        result = mappo_update_bank(bank, optimizer, w.record, w.ring, w.advantages, w.returns, indices[:, r:r + 1].contiguous(), norms,
                                   max_grad_norm=MAX_GRAD_NORM, grads=True)
        stats.append(cpu(result.stats))
        grads.append(cpu(result.grads))
    assert optimizer.step == w.step + rows
    parts = (np.concatenate(stats, axis=1), np.concatenate(grads, axis=1), state_of(bank, optimizer.exp_avg, optimizer.exp_avg_sq, norms.state))
    assert_same_update(parts, whole[:3], f"{kind}: {rows} calls of one row")


# ---------------------------------------------------------------- 5: members do not see each other

@pytest.mark.parametrize("kind", KINDS)
def test_members_do_not_see_each_other(hip_lib, kind):
    w = world(kind)
    indices = w.rows([0, 1], 2, 33, seed=23)
    base = run_bank(w, indices, 0)
    changed_bank = w.bank()
    changed_bank.params[0].mul_(1.5).add_(0.01)
    other = indices.clone()
    other[0] = w.rows([0], 2, 33, seed=29)[0]
    assert not torch.equal(other[0], indices[0]) and torch.equal(other[1], indices[1])
    changed = run_bank(w, other, 0, bank=changed_bank)
    same_bits(changed[0][1], base[0][1], "member 1's stats")
    same_bits(changed[1][1], base[1][1], "member 1's gradients")
    for name in base[2]:
        same_bits(changed[2][name][1], base[2][name][1], f"member 1's {name}")
    assert not np.array_equal(changed[1][0], base[1][0]) and not np.array_equal(changed[0][0], base[0][0])  # member 0's did change


# ---------------------------------------------------------------- 6: advantages

def test_advantages_per_member_equal_the_plain_ones_on_the_members_worlds(hip_lib):
    k, n, t = 3, 12, 8
    env = BalanceMadronaTorch(n, 0)
    bank = make_bank("beam2", env, k)
    owner = owner_table(n, k)
    record, _ = bank_rollout("beam2", env, bank, owner, t, seed=3)
    env.close()
    assert cpu(record.dones).any() and cpu(record.rewards).any()  # episodes end inside the record
    norms = ValueNormBank(k, DEV)
    norms.state.copy_(torch.tensor([[m, m * m + s * s, 1.0] for m, s in zip(VN_MEAN[:k], VN_STD[:k])], device=DEV))
    cells = member_samples(owner, range(k), t)
    raw = cpu(mappo_advantages_bank(record, cells[:2], norms)[0])  # member 2's cells are nobody's here
    advantages, returns = mappo_advantages_bank(record, cells, norms)
    assert tuple(advantages.shape) == tuple(returns.shape) == (t, n, P)
    got_adv, got_ret = cpu(advantages), cpu(returns)
    plain_adv = cpu(mappo_advantages(record, None)[0])
    for member in range(k):
        worlds = [i for i in range(n) if i % k == member]
        sub = MlpBaseRecord(t, len(worlds), P, DEV)
        for name in ("actions", "logprobs", "values", "rewards", "dones"):
            getattr(sub, name).copy_(getattr(record, name)[:, worlds])
        sub.next_done.copy_(record.next_done[worlds])
        want_adv, want_ret = mappo_advantages(sub, norms.member(member))
        same_bits(got_adv[:, worlds], cpu(want_adv), f"member {member}'s advantages")
        same_bits(got_ret[:, worlds], cpu(want_ret), f"member {member}'s returns")
        assert not np.array_equal(got_adv[:, worlds], plain_adv[:, worlds])
    # cells of no member keep their raw advantages: GAE on the values as recorded
    sub = MlpBaseRecord(t, 4, P, DEV)
    worlds = [i for i in range(n) if i % k == 2]
    for name in ("actions", "logprobs", "values", "rewards", "dones"):
        getattr(sub, name).copy_(getattr(record, name)[:, worlds])
    sub.next_done.copy_(record.next_done[worlds])
    from madrona_rl_envs_playground_amd.simulators import gae
    same_bits(raw[:, worlds], cpu(gae(sub.rollout(), 0.99, 0.95)[0]).reshape(t, 4, P), "raw advantages of nobody's cells")


# ---------------------------------------------------------------- 7: the closed loop

@pytest.mark.parametrize("kind", KINDS)
def test_closed_loop_rollout_advantages_update_act(hip_lib, kind):
    """rollout_bank -> mappo_advantages_bank -> mappo_update_bank, twice; the second rollout's record is what plain acts under the
    updated rows give, issued by hand on a second simulator that went through the same first rollout"""
    k, n, t, seed = 3, 33, 8, 41
    env, hand = make_env(kind, n), make_env(kind, n)
    bank = make_bank(kind, env, k)
    start = bank.params.clone()
    owner = owner_table(n, k)
    cells = member_samples(owner, range(k), t)
    optimizer, norms = MappoBankOptimizer(bank), ValueNormBank(k, DEV)
    gen = torch.Generator().manual_seed(1)
    records = []
    for iteration in range(2):
        record, ring = bank_rollout(kind, env, bank, owner, t, seed=seed, first_step=iteration * t)
        records.append({name: cpu(getattr(record, name)) for name in ("actions", "logprobs", "values", "rewards", "dones", "next_done")})
        advantages, returns = mappo_advantages_bank(record, cells, norms)
        order = torch.stack([torch.randperm(cells.shape[1], generator=gen) for _ in range(k)]).to(DEV)
        indices = cells.gather(1, order).view(k, 2, cells.shape[1] // 2).contiguous()
        result = mappo_update_bank(bank, optimizer, record, ring, advantages, returns, indices, norms)
        if iteration == 0:
            updated = bank.params.clone()
            stats = cpu(result.stats)
            # before any update the recomputed log-probs are the record's bit for bit: ratio exactly 1 on every member's first row
            assert (stats[:, 0, STAT("ratio")] == 1.0).all() and (stats[:, 0, STAT("clipfrac")] == 0.0).all()
            assert (stats[:, 1, STAT("ratio")] != 1.0).all()
        assert np.isfinite(cpu(result.stats)).all() and np.isfinite(cpu(advantages)).all() and np.isfinite(cpu(returns)).all()
    assert optimizer.step == 4
    assert np.isfinite(cpu(bank.params)).all() and np.isfinite(cpu(norms.state)).all() and cpu(norms.state).all()
    for member in range(k):
        assert not torch.equal(updated[member], start[member]) and not torch.equal(bank.params[member], updated[member])
    # by hand: the same first rollout under the starting rows, then T plain acts per member under the rows after the first update
    first_bank, second_bank = make_bank(kind, hand, k), make_bank(kind, hand, k)
    first_bank.params.copy_(start)
    second_bank.params.copy_(updated)
    bank_rollout(kind, hand, first_bank, owner, t, seed=seed, first_step=0)
    record_class, value_only = (MlpBaseRecord, mlpbase_act) if is_beam(kind) else (CnnRecord, cnn_act)
    by_member = [record_class(t, n, P, DEV) for _ in range(k)]
    mine = [(owner.t() == member).reshape(hand.static_actions.shape) for member in range(k)]  # ACTION is (P, N, 1)
    for step in range(t):
        composed = torch.full_like(hand.static_actions, -1)
        for member in range(k):
            actions = hand.act(second_bank.policy(member), record=by_member[member], row=step, seed=seed, step=t + step)
            composed = torch.where(mine[member], actions, composed)
        hand.static_actions.copy_(composed)
        hand.sim.step()
    for member in range(k):
        value_only(hand.sim, second_bank.policy(member), record=by_member[member], row=t, value_only=True)
    torch.cuda.synchronize()
    got = records[1]
    cell_owner = cpu(owner)
    for name in ("actions", "logprobs", "values"):
        want = np.zeros_like(got[name])
        for member in range(k):
            own = np.broadcast_to(cell_owner == member, want.shape)
            want[own] = cpu(getattr(by_member[member], name))[own]
        same_bits(got[name], want, f"{kind}: {name} of the second rollout")
    for name in ("rewards", "dones", "next_done"):
        same_bits(got[name], cpu(getattr(by_member[0], name)), f"{kind}: {name} of the second rollout")
    assert got["dones"].any()
    assert not np.array_equal(records[0]["values"], got["values"])
    env.close()
    hand.close()


# ---------------------------------------------------------------- 8: the tool

def load_tool():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "population_train_device.py")
    spec = importlib.util.spec_from_file_location("population_train_device", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("game, options", [("balance", {}), ("simplecooked", {"layout": "simple", "horizon": 6})])
def test_the_tool_runs(hip_lib, game, options):
    tool = load_tool()
    seen = []
    out = tool.run(game, [3, 4, 5], 24, 8, 2, play_worlds=18, log=seen.append, ppo_epoch=2, num_mini_batch=2, **options)
    history = out["history"]
    assert history == seen and len(history) == 2 and [entry["optimizer_step"] for entry in history] == [4, 8]
    for entry in history:
        assert len(entry["mean_return"]) == 3 and entry["worlds"] == [8, 8, 8]  # every world finished an episode in eight steps
        assert all(r is not None and np.isfinite(r) for r in entry["mean_return"])
        for name in _lib.MAPPO_STATS[:7]:
            assert len(entry[name]) == 3 and np.isfinite(entry[name]).all(), name
    assert history[0]["value_loss"] != history[1]["value_loss"]  # the parameters moved between the updates
    matrix, episodes = np.array(out["mean_return"]), np.array(out["episodes"])
    assert matrix.shape == episodes.shape == (3, 3) and np.isfinite(matrix).all() and (episodes >= 2).all()


# ---------------------------------------------------------------- 9: refusals at the C ABI

@pytest.mark.parametrize("kind", ["beam2", "kitchen"])
def test_c_level_refusals_change_nothing(hip_lib, kind):
    L, INVALID = hip_lib, _lib.MRL_ERR_INVALID
    w = world(kind)
    bank = w.bank()
    optimizer = MappoBankOptimizer(bank)
    optimizer.exp_avg.copy_(w.exp_avg)
    optimizer.exp_avg_sq.copy_(w.exp_avg_sq)
    norms = ValueNormBank(K, DEV)
    norms.state.copy_(w.vn_state)
    before = state_of(bank, optimizer.exp_avg, optimizer.exp_avg_sq, norms.state)
    members, rows, width = 2, 1, 33
    indices = w.rows([1, 2], rows, width, seed=31)
    workspace = optimizer.workspace(width, rows, members)
    count = T * N * P
    policy = bank.policy(0)
    (_, entry), shape, batch_type, obs = policy._mappo_batch(w.record, w.ring, count)
    stream = torch.cuda.current_stream().cuda_stream
    num_params = bank.num_params

    def update(shape=shape, inds=indices.data_ptr(), width=width, cfg_flags=15, norm=norms.state.data_ptr(), ws=workspace.data_ptr(),
               ws_bytes=workspace.numel(), size=count, hip_stream=stream, **changes):
        fields = dict(params_dev=bank.params.data_ptr(), exp_avg=optimizer.exp_avg.data_ptr(), exp_avg_sq=optimizer.exp_avg_sq.data_ptr(),
                      row_bytes=4 * num_params, num_policies=K, first_member=1, num_members=members, step=0)
        fields.update(changes)
        opt = _lib.MappoBankOptimizerDesc(**fields)
        r = w.record
        batch = batch_type(obs.data_ptr(), r.actions.data_ptr(), r.logprobs.data_ptr(), r.values.data_ptr(), w.returns.data_ptr(),
                           w.advantages.data_ptr(), size)
        cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, cfg_flags)
        return entry(ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch), inds, rows, width, ctypes.byref(cfg), norm, ws, ws_bytes,
                     None, None, 0, hip_stream)

    # the bank's own refusals
    assert update(num_members=0) == INVALID
    assert update(first_member=3) == INVALID and update(first_member=K) == INVALID  # first_member + num_members > K
    assert update(num_policies=257, first_member=0) == INVALID and update(num_policies=0) == INVALID
    assert update(row_bytes=4 * num_params - 4) == INVALID and update(row_bytes=4 * num_params + 2) == INVALID
    assert update(ws_bytes=workspace.numel() - 1) == INVALID  # short of M times the plain one
    assert update(ws_bytes=workspace.numel() // members) == INVALID  # the plain call's size
    assert update(ws=workspace.data_ptr() + 4) == INVALID
    # everything the plain call refuses
    assert update(inds=None) == INVALID and update(ws=None) == INVALID and update(norm=None) == INVALID
    assert update(params_dev=None) == INVALID and update(exp_avg=None) == INVALID and update(exp_avg_sq=None) == INVALID
    assert update(params_dev=bank.params.data_ptr() + 4 * num_params) == INVALID  # not the bank's first row: not the policy's array
    assert update(exp_avg=optimizer.exp_avg.data_ptr() + 2) == INVALID and update(inds=indices.data_ptr() + 1) == INVALID
    assert update(cfg_flags=16) == INVALID and update(width=0) == INVALID and update(size=0) == INVALID
    if is_beam(kind):
        assert update(shape=_lib.MlpBasePolicyDesc(bank.params.data_ptr(), 64, 3, 0)) == INVALID
        assert update(shape=_lib.MlpBasePolicyDesc(bank.params.data_ptr(), 512, 2, 0)) == INVALID
    else:
        assert update(shape=_lib.MappoPolicyDesc(bank.params.data_ptr(), 512, 0, bank.width, bank.height, bank.channels)) == INVALID
        assert update(shape=_lib.MappoPolicyDesc(bank.params.data_ptr(), 64, 0, 2, bank.height, bank.channels)) == INVALID
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            rc = update(hip_stream=torch.cuda.current_stream().cuda_stream)
            scratch.add_(0)  # (a capture must record something)
    assert rc == INVALID
    torch.cuda.synchronize()
    after = state_of(bank, optimizer.exp_avg, optimizer.exp_avg_sq, norms.state)
    for name, value in before.items():
        same_bits(after[name], value, f"{kind}: {name} after the refusals")
    # and the same arguments unchanged are accepted
    assert update() == 0
    torch.cuda.synchronize()
    after = state_of(bank, optimizer.exp_avg, optimizer.exp_avg_sq, norms.state)
    assert not np.array_equal(after["params"][1], before["params"][1]) and not np.array_equal(after["params"][2], before["params"][2])
    same_bits(after["params"][[0, 3]], before["params"][[0, 3]], "the untrained rows")
