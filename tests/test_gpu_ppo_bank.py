"""GPU: K seeds of the small PPO agent on one batch -- ``rollout_policy_bank`` and ``ppo_update_bank`` (``mrl_rollout_policy`` and
``mrl_ppo_update`` with ``num_members`` set) against the plain calls they promise to equal.  Every comparison is ``torch.equal``
on the raw bits: the contracts are bitwise, there is no tolerance anywhere in this file.

Shapes.  K = 3 members of W = 65 worlds (N = 195): every member has one full wavefront and one of a single lane, and the member
boundaries (65, 130) fall where a plain launch's wavefronts (64, 128) straddle them.  The simulators start where episodes end
inside the few rows looked at -- Cartpole after 12 random steps, Acrobot 3 steps short of its 500-step limit, the beam anywhere
(an episode lasts at most three steps) -- so the rows hold restarts.

One departure from "compare the plain call's next_* with the bank's", stated here because it is a property of the simulators and
not of the feature: the plain one-step call lets ALL N worlds act under policy k, so in the worlds of the other members other
episodes end in that step than in the bank's, and a world that restarts in a step takes its episode number -- and with it its
first state -- from a count over the whole batch.  The state BEHIND the step is therefore comparable only in the worlds that did
not restart in it.  The test compares the plain call's next_obs and next_value there, its next_done everywhere, and then every
world's next_* against the plain call's CLOSING launch (``num_steps = 0``) on a simulator replayed through all T steps, which
is the same kernel on the same state and leaves no world out.  (Measured once on an MI355X with these seeds: on the beam the
plain call's next_obs differs from the bank's in 41 of the 44 worlds of member 1 that restarted in the last step, and in no
world that went on; on Cartpole and Acrobot in none.)"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AcrobotSimulator, BalanceBeamSimulator, CartpoleSimulator, ExecMode, MlpAgent,  # noqa: E402
                                                         MlpPolicy, MlpPolicyBank, PpoBankOptimizer, PpoOptimizer, Rollout, gae,
                                                         member_minibatch_indices, ppo_update, ppo_update_bank, random_balance_action)

CONFIGS = {"cartpole": (4, 2, "state"), "acrobot": (4, 3, "state"), "acrobot-gym": (6, 3, "gym"), "beam": (7, 4, "beam")}
K, W = 3, 65
N = K * W
SEED, FIRST = 23, 7
DEV = "cuda:0"


def prepare(config, n=N):
    if config == "cartpole":
        sim = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
        sim.rollout_random(12, seed=5)
    elif config == "beam":
        sim = BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    else:
        sim = AcrobotSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
        sim.rollout_random(497, seed=5)
    return sim


def make_bank(config, members=K):
    d, a, observation = CONFIGS[config]
    agents = []
    for k in range(members):
        torch.manual_seed(100 + k)
        agent = MlpAgent(d, a)
        with torch.no_grad():
            agent.actor[4].weight.mul_(4.0)  # (torch's default last layer is nearly uniform: let the members prefer different moves)
        agents.append(agent)
    return MlpPolicyBank.from_modules(agents, observation=observation, device=DEV)


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype and torch.equal(bits(got), bits(want)), f"{what} differs"


def joint(config, actions, t, seed=SEED, first_step=FIRST):
    """row t of a record's actions as the ACTION tensor ``step_with_actions`` takes; on the beam with the partner's replayable move"""
    n = actions.shape[1]
    if config != "beam":
        return actions[t].reshape(n, 1).contiguous()
    partner = torch.from_numpy(np.asarray(random_balance_action(seed, first_step + t, np.arange(n), 1)).astype(np.int32)).to(DEV)
    return torch.stack([actions[t], partner.reshape(n)]).reshape(2, n, 1).contiguous()


def tensors(sim, config):
    names = ["observation_tensor", "done_tensor" if config == "beam" else "reset_tensor", "reward_tensor", "reset_count_tensor"]
    if config.startswith("acrobot"):
        names.append("episode_length_tensor")
    return {name: getattr(sim, name)().to_torch().clone() for name in names}


def next_episode_state(sim):
    """where the episode counter stands, read through a forced restart of world 0 (it changes that world: the last use)"""
    mask = torch.zeros(sim.num_worlds, dtype=torch.uint8)
    mask[0] = 1
    sim.reset_worlds(mask)
    return sim.observation_tensor().to_torch().clone()


@functools.lru_cache(maxsize=None)
def collected(config, steps, members=K, worlds=W, greedy=False):
    """one bank rollout per (configuration, length), shared by the tests below and left unchanged by them"""
    sim = prepare(config, members * worlds)
    bank = make_bank(config, members)
    rollout = sim.rollout_policy_bank(bank, steps, seed=SEED, first_step=FIRST, greedy=greedy)
    final = tensors(sim, config)
    action = sim.action_tensor().to_torch().clone()
    counter = next_episode_state(sim)
    sim.close()
    torch.cuda.synchronize()
    return {"bank": bank, "rollout": rollout, "final": final, "action": action, "counter": counter}


def check_rows(config, c, steps, members=K, worlds=W, greedy=False):
    """every (member, row) of a bank rollout against the plain one-step rollout of that member on a replayed simulator"""
    r, bank, n = c["rollout"], c["bank"], members * worlds
    restarted = 0
    for t in range(steps):
        for k in range(members):
            sim = prepare(config, n)
            for s in range(t):
                sim.step_with_actions(joint(config, r.actions, s))
            p = sim.rollout_policy(bank.policy(k), 1, seed=SEED, first_step=FIRST + t, greedy=greedy)
            own = slice(k * worlds, (k + 1) * worlds)
            for name in ("obs", "dones", "values", "actions", "logprobs"):
                same(getattr(p, name)[0, own], getattr(r, name)[t, own], f"{config}: member {k}, row {t}: {name}")
            same(p.rewards[0, own], r.rewards[t, own], f"{config}: member {k}, row {t}: rewards")
            if t == steps - 1:
                same(p.next_done[own], r.next_done[own], f"{config}: member {k}: next_done")
                stayed = r.next_done[own] == 0  # (see the header: a restart's first state is numbered over the whole batch)
                restarted += int((~stayed).sum())
                same(p.next_obs[own][stayed], r.next_obs[own][stayed], f"{config}: member {k}: next_obs of the worlds that went on")
                same(p.next_value[own][stayed], r.next_value[own][stayed], f"{config}: member {k}: next_value of the worlds that went on")
            sim.close()
    # ... and every world's closing row: the plain closing launch on the state all T steps lead to
    sim = prepare(config, n)
    for s in range(steps):
        sim.step_with_actions(joint(config, r.actions, s))
    for k in range(members):
        p = sim.rollout_policy(bank.policy(k), 0)
        own = slice(k * worlds, (k + 1) * worlds)
        for name in ("next_obs", "next_value", "next_done"):
            same(getattr(p, name)[own], getattr(r, name)[own], f"{config}: member {k}: {name} of the closing launch")
    sim.close()
    return restarted


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_rollout_parity(config, hip_lib):
    steps = 5
    c = collected(config, steps)
    r = c["rollout"]
    d = CONFIGS[config][0]
    assert tuple(r.obs.shape) == (steps, N, d) and tuple(r.actions.shape) == (steps, N) and tuple(r.next_obs.shape) == (N, d)
    restarted = check_rows(config, c, steps)
    done = int((r.dones != 0).sum()) + int((r.next_done != 0).sum())
    print(f"{config}: {done} restarts inside the rows, {restarted} of them in the last step")
    assert done > 0, "the rows should hold restarts"
    # the members do act under different parameters: the same observation column-wise would not tell, the values do
    assert len({float(r.values[0, k * W]) for k in range(K)}) == K


@pytest.mark.parametrize("config", ["cartpole", "beam"])
def test_greedy_rollout_parity(config, hip_lib):
    c = collected(config, 2, greedy=True)
    check_rows(config, c, 2, greedy=True)
    sampled = collected(config, 5)["rollout"]
    assert not torch.equal(c["rollout"].actions[0], sampled.actions[0]), "greedy and sampled rows should differ somewhere"


def test_one_world_per_member(hip_lib):
    """W = 1 with K = 5: every workgroup holds one live lane"""
    c = collected("cartpole", 3, members=5, worlds=1)
    assert tuple(c["rollout"].actions.shape) == (3, 5)
    check_rows("cartpole", c, 3, members=5, worlds=1)


@pytest.mark.parametrize("config", ["cartpole", "beam"])
def test_a_bank_of_one_is_the_plain_rollout_and_out_is_reused(config, hip_lib):
    bank = make_bank(config, 1)
    banked, plain = prepare(config), prepare(config)
    r = banked.rollout_policy_bank(bank, 5, seed=SEED, first_step=FIRST)
    p = plain.rollout_policy(bank.policy(0), 5, seed=SEED, first_step=FIRST)
    for name, got, want in zip(Rollout._fields, r, p):
        same(got, want, f"{config}: {name}")
    for (name, got), want in zip(tensors(banked, config).items(), tensors(plain, config).values()):
        same(got, want, f"{config}: {name} afterwards")
    same(banked.action_tensor().to_torch(), plain.action_tensor().to_torch(), f"{config}: ACTION afterwards")
    # out=: the same tensors, filled again with the next rows
    pointers = [t.data_ptr() for t in r]
    again = banked.rollout_policy_bank(bank, 5, seed=SEED, first_step=FIRST + 5, out=r)
    assert again is r and [t.data_ptr() for t in r] == pointers
    p = plain.rollout_policy(bank.policy(0), 5, seed=SEED, first_step=FIRST + 5)
    for name, got, want in zip(Rollout._fields, r, p):
        same(got, want, f"{config}: {name}, second call into out")
    with pytest.raises(ValueError, match=r"out\.obs must be a contiguous"):
        banked.rollout_policy_bank(bank, 4, out=r)
    banked.close()
    plain.close()


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_end_state(config, hip_lib):
    """afterwards the simulator is where T ``step_with_actions`` calls with the recorded actions leave it, the counter included"""
    steps = 5
    c = collected(config, steps)
    r = c["rollout"]
    sim = prepare(config)
    for s in range(steps):
        sim.step_with_actions(joint(config, r.actions, s))
    for (name, want), got in zip(tensors(sim, config).items(), c["final"].values()):
        same(got, want, f"{config}: {name}")
    # ACTION holds the last row (of both seats on the beam); step_with_actions leaves the other simulator's alone
    same(c["action"], joint(config, r.actions, steps - 1), f"{config}: ACTION")
    same(c["counter"], next_episode_state(sim), f"{config}: the state a restart draws next")
    sim.close()


OPTIONS = [(True, True), (True, False), (False, True), (False, False)]


def check_update(config, norm_adv, clip_vloss, first_member=0, members=K, calls=2):
    steps, minibatches, epochs = 6, 2, 2
    c = collected(config, steps)
    r = c["rollout"]
    d, a, observation = CONFIGS[config]
    advantages, returns = gae(r, 0.99, 0.95)
    indices = member_minibatch_indices(steps, N, K, minibatches, epochs, generator=torch.Generator().manual_seed(5), device=DEV)
    rows, width = epochs * minibatches, steps * W // minibatches
    assert tuple(indices.shape) == (K, rows, width) and width == 195
    start = c["bank"].params.clone()
    bank = MlpPolicyBank(d, a, K, observation=observation, device=DEV)
    bank.params.copy_(start)
    optimizer = PpoBankOptimizer(bank, lr=1e-3)
    options = dict(clip_coef=0.2, ent_coef=0.01, vf_coef=0.5, max_grad_norm=0.5, norm_adv=norm_adv, clip_vloss=clip_vloss,
                   stats=True, grads=True)
    alone = []
    for m in range(members):
        policy = MlpPolicy(d, a, observation=observation, device=DEV)
        policy.params.copy_(start[first_member + m])
        alone.append((policy, PpoOptimizer(policy, lr=1e-3)))
    trained = indices[first_member:first_member + members]
    for call in range(calls):
        got = ppo_update_bank(bank, optimizer, r, advantages, returns, trained, first_member=first_member, **options)
        assert tuple(got.stats.shape) == (members, rows, 8) and tuple(got.grads.shape) == (members, rows, bank.num_params)
        assert optimizer.step == rows * (call + 1)
        for m, (policy, plain) in enumerate(alone):
            want = ppo_update(policy, plain, r, advantages, returns, trained[m], **options)
            what = f"{config} {norm_adv, clip_vloss}: call {call}, member {first_member + m}"
            same(got.grads[m], want.grads, f"{what}: grads")
            same(got.stats[m], want.stats, f"{what}: stats")
            same(bank.params[first_member + m], policy.params, f"{what}: params")
            same(optimizer.exp_avg[first_member + m], plain.exp_avg, f"{what}: exp_avg")
            same(optimizer.exp_avg_sq[first_member + m], plain.exp_avg_sq, f"{what}: exp_avg_sq")
            assert plain.step == optimizer.step
            assert not torch.equal(policy.params, start[first_member + m]) and bool(torch.isfinite(got.stats[m]).all())
    for k in range(K):
        if not first_member <= k < first_member + members:
            same(bank.params[k], start[k], f"{config}: untrained row {k}")
            assert not optimizer.exp_avg[k].any() and not optimizer.exp_avg_sq[k].any(), f"{config}: untrained moments {k}"
    same(c["bank"].params, start, "the shared bank")


@pytest.mark.parametrize("norm_adv, clip_vloss", OPTIONS)
def test_update_parity(norm_adv, clip_vloss, hip_lib):
    check_update("cartpole", norm_adv, clip_vloss)


def test_update_of_two_members_from_the_second_leaves_the_first_alone(hip_lib):
    check_update("cartpole", True, True, first_member=1, members=2, calls=1)


@pytest.mark.parametrize("config, norm_adv, clip_vloss", [("beam", True, True), ("acrobot-gym", True, False)])
def test_update_parity_of_the_other_shapes(config, norm_adv, clip_vloss, hip_lib):
    check_update(config, norm_adv, clip_vloss, calls=1)


def test_one_call_of_r_rows_is_r_calls_of_one_row(hip_lib):
    c = collected("cartpole", 6)
    r = c["rollout"]
    advantages, returns = gae(r, 0.99, 0.95)
    indices = member_minibatch_indices(6, N, K, 2, 2, generator=torch.Generator().manual_seed(5), device=DEV)
    banks = []
    for split in (False, True):
        bank = MlpPolicyBank(4, 2, K, device=DEV)
        bank.params.copy_(c["bank"].params)
        optimizer = PpoBankOptimizer(bank, lr=1e-3)
        if split:
            stats = torch.stack([ppo_update_bank(bank, optimizer, r, advantages, returns, indices[:, k:k + 1].contiguous()).stats[:, 0]
                                 for k in range(indices.shape[1])], dim=1)
        else:
            stats = ppo_update_bank(bank, optimizer, r, advantages, returns, indices).stats
        banks.append((bank, optimizer, stats))
    (a, oa, sa), (b, ob, sb) = banks
    same(a.params, b.params, "params")
    same(oa.exp_avg, ob.exp_avg, "exp_avg")
    same(oa.exp_avg_sq, ob.exp_avg_sq, "exp_avg_sq")
    same(sa, sb, "stats")
    assert oa.step == ob.step == 4


def test_more_tiles_than_workgroups(hip_lib):
    """B = 256 * 64 + 65: 258 tiles on at most 256 workgroups, so a workgroup takes two tiles and the last one ends in a tile of one
    lane -- on a synthetic batch of random finite numbers, no simulator."""
    width, samples, members = 256 * 64 + 65, 40000, 2
    g = torch.Generator().manual_seed(9)
    obs = torch.randn((samples, 4), generator=g).to(DEV)
    batch = Rollout(obs, torch.randint(0, 2, (samples,), generator=g, dtype=torch.int32).to(DEV),
                    (-0.7 + 0.1 * torch.randn(samples, generator=g)).to(DEV), torch.randn(samples, generator=g).to(DEV), None, None, None,
                    None, None)
    advantages, returns = torch.randn(samples, generator=g).to(DEV), torch.randn(samples, generator=g).to(DEV)
    indices = torch.randint(0, samples, (members, 1, width), generator=g, dtype=torch.int32).to(DEV)
    start = make_bank("cartpole", members).params.clone()
    bank = MlpPolicyBank(4, 2, members, device=DEV)
    bank.params.copy_(start)
    optimizer = PpoBankOptimizer(bank)
    got = ppo_update_bank(bank, optimizer, batch, advantages, returns, indices, stats=True, grads=True)
    for m in range(members):
        policy = MlpPolicy(4, 2, device=DEV)
        policy.params.copy_(start[m])
        plain = PpoOptimizer(policy)
        want = ppo_update(policy, plain, batch, advantages, returns, indices[m], stats=True, grads=True)
        same(got.grads[m], want.grads, f"member {m}: grads")
        same(got.stats[m], want.stats, f"member {m}: stats")
        same(bank.params[m], policy.params, f"member {m}: params")
        same(optimizer.exp_avg[m], plain.exp_avg, f"member {m}: exp_avg")
        same(optimizer.exp_avg_sq[m], plain.exp_avg_sq, f"member {m}: exp_avg_sq")
        assert bool(torch.isfinite(want.stats).all()) and bool(want.grads.any())


@pytest.mark.parametrize("game", ["cartpole", "balance"])
def test_the_training_tool_on_three_seeds(game, hip_lib):
    """``tools/cartpole_train_device.py --seeds``: the loop on the bank calls, per-member numbers from the (K, W) view"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    try:
        import cartpole_train_device
    finally:
        sys.path.pop(0)
    history = cartpole_train_device.train_bank(64, 32, 2, [5, 6, 7], game=game)
    assert len(history) == 2 and history[-1]["optimizer_step"] == 2 * 4 * 4 and history[0]["lr"] > history[1]["lr"] > 0
    for entry in history:
        assert entry["seeds"] == [5, 6, 7]
        for name in _lib.PPO_STATS + ("mean_return",):
            assert len(entry[name]) == 3 and all(math.isfinite(v) for v in entry[name]), (name, entry)
        assert all(0 < n <= 64 for n in entry["worlds_finished"]) and all(h > 0.5 for h in entry["entropy"])
        assert len(set(entry["pg_loss"])) == 3, "three seeds, three different members"


def test_refusals_on_the_device(hip_lib):
    sim, clean = prepare("cartpole"), prepare("cartpole")
    good = make_bank("cartpole")
    before = tensors(sim, "cartpole")
    # N % K != 0, and more members than worlds
    with pytest.raises(_lib.MrlError, match="a bank of 2 members on 195 worlds"):
        sim.rollout_policy_bank(make_bank("cartpole", 2), 2)
    small = prepare("cartpole", 2)
    with pytest.raises(_lib.MrlError, match="a bank of 3 members on 2 worlds"):
        small.rollout_policy_bank(good, 2)
    small.close()
    # a bank of another shape than the game's: the plain call's words
    with pytest.raises(_lib.MrlError, match="need hidden = 64, num_actions = 2"):
        sim.rollout_policy_bank(make_bank("acrobot"), 2)
    with pytest.raises(_lib.MrlError, match="need hidden = 64, num_actions = 2"):
        sim.rollout_policy_bank(make_bank("beam"), 2)
    beam = prepare("beam")
    with pytest.raises(_lib.MrlError, match="the balance beam takes hidden = 64, obs_dim = 7"):
        beam.rollout_policy_bank(good, 2)
    beam.close()
    # a bank that is not on the simulator's GPU
    elsewhere = MlpPolicyBank(4, 2, K, device="cuda:1" if torch.cuda.device_count() > 1 else "cpu")
    with pytest.raises(ValueError, match=r"bank\.params must be a contiguous float32 tensor \(num_policies, num_params\) on cuda:0"):
        sim.rollout_policy_bank(elsewhere, 2)
    with pytest.raises(ValueError, match="num_steps must not be negative"):
        sim.rollout_policy_bank(good, -1)
    # a capturing stream, wherever the plain rollout refuses one
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    out = sim.rollout_policy_bank(good, 2, seed=SEED, first_step=FIRST)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                sim.rollout_policy_bank(good, 2, out=out)
            scratch.add_(0)
    torch.cuda.synchronize()
    # none of the refusals touched the simulator: it is where a clean one is after the same two steps
    assert any(not torch.equal(bits(t), bits(b)) for t, b in zip(tensors(sim, "cartpole").values(), before.values()))
    for s in range(2):
        clean.step_with_actions(joint("cartpole", out.actions, s))
    for (name, got), want in zip(tensors(sim, "cartpole").items(), tensors(clean, "cartpole").values()):
        same(got, want, f"after the refusals: {name}")
    sim.close()
    clean.close()
    # the update: a workspace of fewer slices than members (the optimizer's own is sized by the call; hand it a short one)
    c = collected("cartpole", 6)
    r = c["rollout"]
    advantages, returns = gae(r, 0.99, 0.95)
    indices = member_minibatch_indices(6, N, K, 2, 2, device=DEV)
    bank = MlpPolicyBank(4, 2, K, device=DEV)
    bank.params.copy_(c["bank"].params)
    optimizer = PpoBankOptimizer(bank)
    one = optimizer.workspace_bytes(195, 4)
    optimizer.workspace = lambda width, rows, members: torch.empty(one * (members - 1), dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.MrlError, match=f"workspace of {2 * one} bytes, mrl_ppo_workspace_bytes asks for {3 * one}"):
        ppo_update_bank(bank, optimizer, r, advantages, returns, indices)
    same(bank.params, c["bank"].params, "params after the refused update")
    with pytest.raises(ValueError, match="the bank holds members 0..2"):
        ppo_update_bank(bank, PpoBankOptimizer(bank), r, advantages, returns, indices, first_member=1)
    with pytest.raises(ValueError, match=r"indices must be \(members, rows, minibatch_size\)"):
        ppo_update_bank(bank, PpoBankOptimizer(bank), r, advantages, returns, indices[0])
