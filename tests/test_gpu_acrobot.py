"""GPU: the Acrobot step (csrc/acrobot.hip) against what the reference's own sim.cpp computed (tests/golden/acrobot_ref.npz,
written by tests/golden/make_acrobot_golden.py), in both forms of the step -- one launch with the in-kernel look-back
(``fused_step`` 1) and the two-launch pair (2).  A workgroup of the single-launch step owns 1024 worlds, so the sizes are
one lane, just under and just over a workgroup, and three workgroups with a ragged last one.

Tolerance: the fixture's own, per set and component: 4 x the reference's largest distance from the float64 twin (two
float32 implementations each within e of the exact step are within 2 e of each other; the other factor 2 is for the
device's sin / cos differing from the C library's by a few ulp).  No transition is left out: the generator dropped what
lies within 1e-3 of the termination threshold.  Everything else -- fresh states, done flags, episode order, clamped
velocities, the agreement of the code paths -- is bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import acrobot_twin as twin  # noqa: E402
from conftest import load_golden  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import AcrobotSimulator, ExecMode, random_acrobot_action  # noqa: E402

SIZES = [1, 1023, 1025, 2049]
FUSED = [1, 2]
FUSED_IDS = ["one_launch", "two_launches"]
GOLD = load_golden("acrobot_ref.npz")
FRESH = GOLD["fresh"]


def make(n, **knobs):
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    with debug_knobs(knobs):
        return AcrobotSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)


def cpu(t):
    return t.to_torch().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def plant(sim, states, lengths=0):
    """teacher-forcing: states (n, 4) into STATE, `lengths` into EPISODE_LENGTH"""
    sim.observation_tensor().to_torch().copy_(torch.from_numpy(np.ascontiguousarray(states, dtype=np.float32)))
    sim.episode_length_tensor().to_torch().fill_(lengths)


def snapshot(sim):
    return {name: cpu(getattr(sim, name)()).copy() for name in
            ("observation_tensor", "reset_tensor", "reward_tensor", "episode_length_tensor", "reset_count_tensor")}


def same(a, b, what):
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), f"{what}: {name} differs"


def next_episode_of(sim, expect):
    """Is `expect` the episode counter?  Read through one forced reset of world 0, which then holds that episode's start
    state (it changes that world: the last use of `sim`)."""
    mask = np.zeros(sim.num_worlds, np.uint8)
    mask[0] = 1
    sim.reset_worlds(mask)
    return cpu(sim.observation_tensor())[0].tobytes() == FRESH[expect].tobytes()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_construction(n, fused, hip_lib):
    sim = make(n, fused_step=fused)
    assert sim.kernel_name == ("mrl_acrobot_step_fused" if fused == 1 else "mrl_acrobot_step")
    assert sim.bytes_per_world_step == 52
    assert sim.observation_tensor().shape == (n, 4) and sim.action_tensor().shape == (n, 1)
    assert sim.reward_tensor().shape == (n, 1) and sim.reset_tensor().shape == (n, 1) and sim.episode_length_tensor().shape == (n, 1)
    assert cpu(sim.observation_tensor()).tobytes() == FRESH[:n].tobytes()
    assert not cpu(sim.reward_tensor()).any() and not cpu(sim.reset_tensor()).any() and not cpu(sim.episode_length_tensor()).any()
    assert np.array_equal(cpu(sim.world_id_tensor())[:, 0], np.arange(n))
    assert next_episode_of(sim, n)  # world w starts as episode w, the counter at N
    sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["reach", "swing"])
def test_teacher_forced_transitions(name, n, fused, hip_lib):
    """every transition of the set at n = 2049 (the set has 2048: world 2048 repeats transition 0), its first n otherwise"""
    idx = np.arange(n) % len(GOLD[name + "_state"])
    state, action = GOLD[name + "_state"][idx], GOLD[name + "_action"][idx]
    want, done, tol = GOLD[name + "_next"][idx], GOLD[name + "_done"][idx] != 0, GOLD[name + "_tol"]
    sim = make(n, fused_step=fused)
    plant(sim, state)
    sim.action_tensor().to_torch().copy_(torch.from_numpy(action[:, None].copy()))
    sim.step()
    got = cpu(sim.observation_tensor())
    assert np.array_equal(cpu(sim.reset_tensor())[:, 0] != 0, done), "RESET differs from the reference's done flags"
    live = ~done
    err = twin.distance(got[live], want[live])
    worst = err.max(axis=0) if live.any() else np.zeros(4)
    print(f"acrobot {name} n={n} fused={fused}: largest distance from the reference {worst}, tolerance {tol}, {int(done.sum())} finished")
    assert (err <= tol).all(), f"largest distance {worst} against tolerance {tol}"
    # every finished world is the next free episode, in ascending world order, bit for bit
    finished = np.flatnonzero(done)
    assert got[finished].tobytes() == FRESH[n + np.arange(len(finished))].tobytes()
    assert int(cpu(sim.reset_count_tensor())[0]) == len(finished)
    assert (cpu(sim.reward_tensor()) == -1.0).all()
    assert np.array_equal(cpu(sim.episode_length_tensor())[:, 0], np.where(done, 0, 1))
    assert np.array_equal(cpu(sim.action_tensor())[:, 0], action)
    assert int(cpu(sim.scan_timeout_tensor())[0]) == 0
    assert next_episode_of(sim, n + len(finished))
    sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", [64, 1025])
def test_clamped_velocities(n, fused, hip_lib):
    """velocities near the bounds: what the reference clamped is exactly +-4 pi / +-9 pi as floats here too, and the done
    flags agree (the states are too fast for a tolerance: the reference itself is 1e-2 from its twin there)"""
    idx = np.arange(n) % 64
    done, mask = GOLD["clamp_done"][idx] != 0, GOLD["clamp_mask"][idx]
    sim = make(n, fused_step=fused)
    plant(sim, GOLD["clamp_state"][idx])
    sim.action_tensor().to_torch().copy_(torch.from_numpy(GOLD["clamp_action"][idx][:, None].copy()))
    sim.step()
    got = cpu(sim.observation_tensor())
    assert np.array_equal(cpu(sim.reset_tensor())[:, 0] != 0, done)
    assert np.array_equal(bits(got[:, 2:])[mask], bits(GOLD["clamp_next"][idx][:, 2:])[mask])
    bound = np.array([twin.MAX_VEL_1, twin.MAX_VEL_2], np.float32)
    assert (np.abs(got[:, 2:]) <= bound).all() and (np.abs(got[:, :2]) <= np.float32(np.pi)).all()
    finished = np.flatnonzero(done)
    assert got[finished].tobytes() == FRESH[n + np.arange(len(finished))].tobytes()
    sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
def test_truncation_is_per_world(fused, hip_lib):
    """Zero torque from a fresh state never terminates (the generator checked episodes 0 .. 8191 on the reference), so every
    world of a new simulator ends its first episode by truncation, at step 501, all at once; worlds restarted 100 steps into
    their second episode finish it 100 steps after the others: the length is the world's own."""
    n = 2049
    assert int(GOLD["quiet_episodes"]) >= 3 * n and len(FRESH) >= 3 * n  # three episodes per world below
    sim = make(n, fused_step=fused)
    sim.action_tensor().to_torch().fill_(1)
    reset = sim.reset_tensor().to_torch()
    early = torch.zeros((), dtype=torch.int32, device="cuda")
    for _ in range(twin.MAX_STEPS):
        sim.step()
        early += reset.sum()
    assert int(early.item()) == 0, "a world finished before its 501st step"
    assert np.array_equal(cpu(sim.episode_length_tensor())[:, 0], np.full(n, twin.MAX_STEPS))
    sim.step()
    assert cpu(sim.reset_tensor()).all() and int(cpu(sim.reset_count_tensor())[0]) == n
    assert cpu(sim.observation_tensor()).tobytes() == FRESH[n:2 * n].tobytes()
    assert not cpu(sim.episode_length_tensor()).any() and (cpu(sim.reward_tensor()) == -1.0).all()
    # second episode: every other world restarted after 100 steps
    for _ in range(100):
        sim.step()
    again = np.arange(n) % 2 == 1
    sim.reset_worlds(again)
    assert np.array_equal(cpu(sim.episode_length_tensor())[:, 0], np.where(again, 0, 100))
    assert cpu(sim.observation_tensor())[again].tobytes() == FRESH[2 * n + np.arange(int(again.sum()))].tobytes()
    early.zero_()
    for _ in range(twin.MAX_STEPS - 100):
        sim.step()
        early += reset.sum()
    assert int(early.item()) == 0
    sim.step()  # step 501 of the untouched worlds
    assert np.array_equal(cpu(sim.reset_tensor())[:, 0] != 0, ~again)
    first_free = 2 * n + int(again.sum())
    assert cpu(sim.observation_tensor())[~again].tobytes() == FRESH[first_free + np.arange(int((~again).sum()))].tobytes()
    early.zero_()
    for _ in range(99):
        sim.step()
        early += reset.sum()
    assert int(early.item()) == 0
    sim.step()  # step 501 of the restarted ones, 100 steps later
    assert np.array_equal(cpu(sim.reset_tensor())[:, 0] != 0, again)
    assert int(cpu(sim.reset_count_tensor())[0]) == int(again.sum())
    sim.close()


def test_episode_index_wraps_at_two_to_the_32(hip_lib):
    """the last eight episodes before 2^32, then 0, 1, ...: the generator's seed is a hash of the 32-bit index"""
    sim = make(16)
    sim.set_episode_counter(2 ** 32 - 8)
    sim.reset_worlds()
    got = cpu(sim.observation_tensor())
    assert got[:8].tobytes() == GOLD["fresh_last"].tobytes() and got[8:].tobytes() == FRESH[:8].tobytes()
    assert next_episode_of(sim, 8)
    sim.close()


def _swing_start(n):
    return GOLD["swing_state"][np.arange(n) % 2048]


def test_the_three_paths_agree(hip_lib):
    """64 steps of a seeded random policy from the swing states (terminations in nearly every step): one launch, two launches
    and one launch with workgroups that act as if dispatched late (the look-back recounts them from their inputs) leave
    identical tensors and the same episode counter."""
    n = 2049
    sims = [make(n, fused_step=1), make(n, fused_step=2), make(n, fused_step=1, fused_heal_test=1), make(n, fused_step=1, fused_heal_test=2)]
    for sim in sims:
        plant(sim, _swing_start(n))
    gen = torch.Generator(device="cuda").manual_seed(11)
    finished = 0
    for t in range(64):
        a = torch.randint(0, 3, (n, 1), dtype=torch.int32, device="cuda", generator=gen)
        for sim in sims:
            sim.step_with_actions(a)
        want = snapshot(sims[0])
        for k, sim in enumerate(sims[1:]):
            same(want, snapshot(sim), f"step {t}, path {k + 1}")
        finished += int(want["reset_count_tensor"][0])
    assert finished > 300
    assert all(next_episode_of(sim, n + finished) for sim in sims)
    for sim in sims:
        assert int(cpu(sim.scan_timeout_tensor())[0]) == 0
        sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
def test_random_rollout(fused, hip_lib):
    """rollout_random(K, seed, first) == K step_with_actions calls with random_acrobot_action's draws; ACTION holds the last"""
    n, steps, seed, first = 2049, 12, 2024, 5
    a, b = make(n, fused_step=fused), make(n, fused_step=fused)
    assert a.rollout_kernel_name == a.kernel_name
    for sim in (a, b):
        plant(sim, _swing_start(n))
    a.rollout_random(steps, seed=seed, first_step=first)
    world = np.arange(n)
    finished = 0
    for k in range(steps):
        want = random_acrobot_action(seed, first + k, world)
        b.step_with_actions(torch.from_numpy(want[:, None].copy()).cuda())
        finished += int(cpu(b.reset_count_tensor())[0])
    assert finished > 100
    same(snapshot(a), snapshot(b), "rollout against single steps")
    assert np.array_equal(cpu(a.action_tensor())[:, 0], random_acrobot_action(seed, first + steps - 1, world))
    assert next_episode_of(a, n + finished) and next_episode_of(b, n + finished)
    a.close()
    b.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
def test_reset_worlds(fused, hip_lib):
    n = 1025
    sim = make(n, fused_step=fused)
    plant(sim, _swing_start(n))
    counter = n
    for k in range(5):
        sim.rollout_random(1, seed=1, first_step=k)
        counter += int(cpu(sim.reset_count_tensor())[0])
    assert counter > n
    before = snapshot(sim)
    action = cpu(sim.action_tensor()).copy()
    sim.reset_worlds(np.zeros(n, np.uint8))  # an empty mask changes nothing
    same(before, snapshot(sim), "empty mask")
    mask = np.random.default_rng(3).random(n) < 0.3
    mask[[0, 1023, 1024]] = [True, False, True]
    sim.reset_worlds(torch.from_numpy(mask))
    after = snapshot(sim)
    assert after["observation_tensor"][mask].tobytes() == FRESH[counter + np.arange(int(mask.sum()))].tobytes()
    assert not after["episode_length_tensor"][mask].any()
    assert after["observation_tensor"][~mask].tobytes() == before["observation_tensor"][~mask].tobytes()
    assert np.array_equal(after["episode_length_tensor"][~mask], before["episode_length_tensor"][~mask])
    for name in ("reset_tensor", "reward_tensor", "reset_count_tensor"):
        assert after[name].tobytes() == before[name].tobytes(), name
    assert np.array_equal(cpu(sim.action_tensor()), action)
    assert next_episode_of(sim, counter + int(mask.sum()))  # later resets go on from there
    sim.close()


def test_two_shards_equal_one_simulator(hip_lib):
    """1025 + 1024 worlds as two shards in one process (reseed_shard, phase 1, the gathered phase 2) against one simulator of
    2049, over 16 steps from the swing states"""
    n, cut = 2049, 1025
    whole, lo, hi = make(n), make(cut), make(n - cut)
    lo.reseed_shard(0, n)
    hi.reseed_shard(cut, n)
    assert torch.equal(torch.cat([lo.observation_tensor().to_torch(), hi.observation_tensor().to_torch()]), whole.observation_tensor().to_torch())
    start = _swing_start(n)
    plant(whole, start)
    plant(lo, start[:cut])
    plant(hi, start[cut:])
    gen = torch.Generator(device="cuda").manual_seed(5)
    finished = 0
    for t in range(16):
        a = torch.randint(0, 3, (n, 1), dtype=torch.int32, device="cuda", generator=gen)
        whole.step_with_actions(a)
        lo.step_phase1(a[:cut].contiguous())
        hi.step_phase1(a[cut:].contiguous())
        counts = torch.cat([lo.shard_count_tensor().to_torch(), hi.shard_count_tensor().to_torch()]).contiguous()
        lo.step_phase2_gathered(counts, 0)
        hi.step_phase2_gathered(counts, 1)
        for name in ("observation_tensor", "reset_tensor", "reward_tensor", "episode_length_tensor"):
            both = torch.cat([getattr(lo, name)().to_torch(), getattr(hi, name)().to_torch()])
            assert torch.equal(both, getattr(whole, name)().to_torch()), f"step {t}: {name}"
        assert int(counts.sum().item()) == int(cpu(whole.reset_count_tensor())[0])
        finished += int(counts.sum().item())
    assert finished > 100
    for sim in (whole, lo, hi):
        sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
def test_captured_steps_replay(fused, hip_lib):
    """after prepare_graph_capture, 3 captured steps replayed twice on one stream equal 6 plain steps"""
    n = 2049
    eager, graphed = make(n, fused_step=fused), make(n, fused_step=fused)
    for sim in (eager, graphed):
        plant(sim, _swing_start(n))
    graphed.prepare_graph_capture()
    gen = torch.Generator(device="cuda").manual_seed(8)
    acts = [torch.randint(0, 3, (n, 1), dtype=torch.int32, device="cuda", generator=gen) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for a in acts:
                graphed.step_with_actions(a)
    torch.cuda.current_stream().wait_stream(side)
    finished = 0
    for _ in range(2):
        graph.replay()
        for a in acts:
            eager.step_with_actions(a)
            finished += int(cpu(eager.reset_count_tensor())[0])
    torch.cuda.synchronize()
    assert finished > 50
    same(snapshot(eager), snapshot(graphed), "two replays of three captured steps")
    eager.close()
    graphed.close()


def test_env_wrappers(hip_lib):
    from madrona_rl_envs_playground_amd.envs import AcrobotMadronaNumpy, AcrobotMadronaTorch
    n = 1025
    env = AcrobotMadronaTorch(n, 0)
    assert env.action_space.n == 3 and env.observation_space.shape == (4,)
    assert np.allclose(env.observation_space.high, [np.pi, np.pi, 4 * np.pi, 9 * np.pi])
    obs = env.reset()
    assert obs.shape == (n, 4) and obs.cpu().numpy().tobytes() == FRESH[:n].tobytes()
    actions = torch.randint(0, 3, (n,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    obs, rewards, dones, infos = env.step(actions)
    assert obs.shape == (n, 4) and rewards.shape == (n, 1) and dones.shape == (n,) and len(infos) == n
    assert (rewards == -1).all() and not dones.any()
    mask = torch.zeros(n, dtype=torch.bool)
    mask[[3, 1024]] = True
    obs = env.reset(worlds=mask)
    assert obs[mask.cuda()].cpu().numpy().tobytes() == FRESH[n:n + 2].tobytes()
    env.close()

    gym = AcrobotMadronaTorch(n, 0, observation="gym")
    assert gym.observation_space.shape == (6,)
    obs, _, _, _ = gym.step(actions)
    state = gym.sim.observation_tensor().to_torch()
    want = torch.stack([torch.cos(state[:, 0]), torch.sin(state[:, 0]), torch.cos(state[:, 1]), torch.sin(state[:, 1]), state[:, 2], state[:, 3]], dim=1)
    assert obs.shape == (n, 6) and torch.equal(obs, want)
    gym.close()

    host = AcrobotMadronaNumpy(n, 0, observation="gym")
    obs, rewards, dones, infos = host.step(actions.cpu().numpy())
    assert isinstance(obs, np.ndarray) and obs.shape == (n, 6) and np.array_equal(obs, want.cpu().numpy())
    assert rewards.shape == (n, 1) and dones.shape == (n,)
    assert host.reset().shape == (n, 6)
    host.close()
