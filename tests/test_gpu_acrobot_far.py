"""GPU: the Acrobot step (csrc/acrobot.hip) from angles far outside [-pi, pi] -- states a caller may write into STATE, and
the only way into the branches of the hot kernel that no pendulum within the velocity bounds reaches: the second select
of wrap_fast, the per-world fallback to step_plain behind `if (!all_good)` with its turn loop, wrap_plain's bounded loops
and its one-piece wrap beyond 64 turns.  Against what the reference's own sim.cpp computed from the same states
(tests/golden/acrobot_far_ref.npz, tests/golden/make_acrobot_golden.py: generate_far; tests/test_ref_acrobot.py asserts
from the float64 twin that each set's inputs lie on the path it is named after):

    turns2   the fast path accepted, both selects of wrap_fast
    turns3   the fast path evaluated and refused (the angle stays unwrapped): the fallback, 3 .. 20 trips of wrap_plain
    beyond   stage angles beyond kFastRange: the fallback, at most 64 trips
    piece    more than 64 turns off: the one-piece wrap, where the kernel departs from the reference's loop by design and is
             compared with it within the reference's own distance from the twin

Tolerance: the fixture's, per set and component, 4 x the reference's largest distance from the twin, as in
test_gpu_acrobot.py; nothing is left out.  Everything else is bit for bit: done flags, fresh states and their order, and
that a world's result depends neither on its thread-mates, nor on its slot in the thread, nor on the form of the step.
Measured on the MI355X, largest distance over tolerance (theta1, theta2, omega1, omega2): turns2 0.45, 0.42, 0.30, 0.33;
turns3 0.0008, 0.0018, 0.043, 0.034; beyond 0.0003, 0.0003, 0.0046, 0.0078; piece 0.17, 0.17, 0.0018, 0.0012 (step_plain
rounds where the reference rounds; the tolerance is the reference's float32 error at angles of hundreds of radians).

A workgroup owns 1024 worlds and thread t holds slots u = 0 .. 3 = worlds first + 256 u + t (per 1024-world trip in the
two-launch kernel), which is where the sizes and the planted pattern come from."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import acrobot_twin as twin  # noqa: E402
from conftest import load_golden  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import random_acrobot_action  # noqa: E402
from test_gpu_acrobot import FRESH, FUSED, FUSED_IDS, GOLD, cpu, make, next_episode_of, plant, same, snapshot  # noqa: E402

FAR = load_golden("acrobot_far_ref.npz")
SETS = ["turns2", "turns3", "beyond", "piece"]
FALLBACK = ["turns3", "beyond", "piece"]
N = 2049


def device_actions(action):
    return torch.from_numpy(np.ascontiguousarray(action, dtype=np.int32)[:, None].copy()).cuda()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", [1, 1025, 2049])
@pytest.mark.parametrize("name", SETS)
def test_teacher_forced_far_transitions(name, n, fused, hip_lib):
    """World w takes transition w mod 512 of the set.  n = 1: three padded slots mirror the one world.  The last world of
    n = 1025 and n = 2049 is `first` of a workgroup whose other 1023 lanes are padding that mirrors it: in the `turns2`
    case it is taken from `beyond`, so that in every case the padded lanes run the fallback and must leave nothing behind."""
    source = np.array([name] * n, dtype=object)
    if n > 1024 and name not in FALLBACK:
        source[n - 1] = "beyond"
    idx = np.arange(n) % 512
    pick = lambda key: np.stack([FAR[f"{s}_{key}"][i] for s, i in zip(source, idx)])  # noqa: E731
    state, action, want, done = pick("state"), pick("action"), pick("next"), pick("done") != 0
    tol = np.stack([FAR[s + "_tol"] for s in source])  # per world: its own set's
    sim = make(n, fused_step=fused)
    plant(sim, state)
    sim.action_tensor().to_torch().copy_(device_actions(action))
    sim.step()
    got = cpu(sim.observation_tensor())
    assert np.array_equal(cpu(sim.reset_tensor())[:, 0] != 0, done), "RESET differs from the reference's done flags"
    live = ~done
    err = twin.distance(got[live], want[live])
    ratio = (err / tol[live]).max(axis=0) if live.any() else np.zeros(4)
    print(f"acrobot far {name} n={n} fused={fused}: largest distance from the reference over the tolerance {ratio}, "
          f"tolerance {FAR[name + '_tol']}, {int(done.sum())} finished")
    assert (err <= tol[live]).all(), f"largest distance over tolerance {ratio}"
    if name != "piece":  # (the loops end within [-pi, pi]; the one-piece wrap's quotient is rounded: see DESIGN.md section 10)
        assert (np.abs(got[live][:, :2]) <= np.float32(np.pi)).all()
    finished = np.flatnonzero(done)
    assert got[finished].tobytes() == FRESH[n + np.arange(len(finished))].tobytes()
    assert int(cpu(sim.reset_count_tensor())[0]) == len(finished)
    assert (cpu(sim.reward_tensor()) == -1.0).all()
    assert np.array_equal(cpu(sim.episode_length_tensor())[:, 0], np.where(done, 0, 1))
    assert np.array_equal(cpu(sim.action_tensor())[:, 0], action)
    assert int(cpu(sim.scan_timeout_tensor())[0]) == 0
    assert next_episode_of(sim, n + len(finished))
    sim.close()


# ---- the planted batch: 2049 swing worlds, far states in chosen slots ----
def _far_worlds():
    """(world, set, row): thread t of workgroup 0 holds far states in the slots named by the four bits of t mod 16 -- every
    subset of a thread's slots, none and all included -- alternately from `beyond` and `turns3`; the same in workgroup 1
    from `piece` and `turns2` (a fast-path world among thread-mates that fall back); and the one world of the ragged third."""
    out = []
    for group, names in ((0, ("beyond", "turns3")), (1, ("piece", "turns2"))):
        for t in range(256):
            for u in range(4):
                if (t % 16) >> u & 1:
                    out.append((1024 * group + 256 * u + t, names[len(out) % 2], (len(out) // 2) % 512))
    out.append((2048, "beyond", 511))
    return out


PLANTED = _far_worlds()
ROTATE = 256 + 1  # another slot of another thread


def planted_batch(shift=0, far=True):
    """(state, action, worlds that hold far states): swing transition w mod 2048 in world w, the far states of PLANTED
    `shift` worlds further on (mod N)"""
    idx = np.arange(N) % 2048
    state, action = GOLD["swing_state"][idx].copy(), GOLD["swing_action"][idx].copy()
    where = np.array([(w + shift) % N for w, _, _ in PLANTED])
    if far:
        for at, (_, name, row) in zip(where, PLANTED):
            state[at], action[at] = FAR[name + "_state"][row], FAR[name + "_action"][row]
    return state, action, where


def planted_done():
    """the reference's done flags of PLANTED's transitions, and which of them take the fallback"""
    return (np.array([FAR[name + "_done"][row] != 0 for _, name, row in PLANTED]),
            np.array([name in FALLBACK for _, name, _ in PLANTED]))


def phase1(state, action):
    """the two-launch step's first launch: every world's post-transition state, finished ones included, and RESET"""
    sim = make(N, fused_step=2)
    plant(sim, state)
    sim.step_phase1(device_actions(action))
    out = cpu(sim.observation_tensor()).copy(), cpu(sim.reset_tensor())[:, 0].copy()
    sim.close()
    return out


def test_a_world_depends_on_neither_its_thread_mates_nor_its_slot(hip_lib):
    base_state, base_done = phase1(*planted_batch(far=False)[:2])
    assert 0.10 < (base_done != 0).mean() < 0.25
    results = []
    for shift in (0, ROTATE):
        state, action, where = planted_batch(shift)
        got, done = phase1(state, action)
        in_range = np.ones(N, bool)
        in_range[where] = False
        assert in_range.sum() == N - len(PLANTED)
        assert got[in_range].tobytes() == base_state[in_range].tobytes(), f"shift {shift}: an in-range world's state depends on its thread-mates"
        assert np.array_equal(done[in_range], base_done[in_range]), f"shift {shift}: an in-range world's done flag depends on its thread-mates"
        results.append((got[where], done[where]))
        # and the far worlds are the reference's: done flags, live states within the tolerance
        want_done, _ = planted_done()
        assert np.array_equal(done[where] != 0, want_done)
        for k, (_, name, row) in enumerate(PLANTED):
            if not want_done[k]:
                err = twin.distance(got[where[k]][None], FAR[name + "_next"][row][None])[0]
                assert (err <= FAR[name + "_tol"]).all(), (name, row, err)
    assert results[0][0].tobytes() == results[1][0].tobytes(), "a far world's state depends on its slot or its thread-mates"
    assert np.array_equal(results[0][1], results[1][1])
    # the one-launch step on the first batch: the same transition, finished worlds already re-seeded
    state, action, where = planted_batch(0)
    got, done = phase1(state, action)
    sim = make(N, fused_step=1)
    plant(sim, state)
    sim.step_with_actions(device_actions(action))
    fused_state, fused_done = cpu(sim.observation_tensor()), cpu(sim.reset_tensor())[:, 0]
    assert np.array_equal(fused_done, done)
    live = done == 0
    assert fused_state[live].tobytes() == got[live].tobytes()
    finished = np.flatnonzero(~live)
    assert fused_state[finished].tobytes() == FRESH[N + np.arange(len(finished))].tobytes()
    assert int(cpu(sim.reset_count_tensor())[0]) == len(finished)
    assert next_episode_of(sim, N + len(finished))
    sim.close()


def test_the_paths_agree_from_far_states(hip_lib):
    """one launch, two launches, and one launch with late workgroups that the look-back recounts from their inputs
    (recount_chunk's advance<1> meets the fallback's done flag), the pattern replanted before each of 3 steps, each time
    257 worlds further on"""
    sims = [make(N, fused_step=1), make(N, fused_step=2), make(N, fused_step=1, fused_heal_test=1), make(N, fused_step=1, fused_heal_test=2)]
    want_done, falls_back = planted_done()
    assert (want_done & falls_back).sum() >= 1, "no fallback world of the pattern finishes"
    finished = 0
    for t in range(3):
        state, action, where = planted_batch(t * ROTATE)
        a = device_actions(action)
        for sim in sims:
            plant(sim, state)
            sim.step_with_actions(a)
        want = snapshot(sims[0])
        for k, sim in enumerate(sims[1:]):
            same(want, snapshot(sim), f"step {t}, path {k + 1}")
        assert np.array_equal(want["reset_tensor"][where, 0] != 0, want_done), f"step {t}: done flags of the far worlds"
        finished += int(want["reset_count_tensor"][0])
    assert finished > 3 * int(want_done.sum())
    assert all(next_episode_of(sim, N + finished) for sim in sims)
    for sim in sims:
        assert int(cpu(sim.scan_timeout_tensor())[0]) == 0
        sim.close()


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
def test_random_rollout_from_far_states(fused, hip_lib):
    """rollout_random(2, seed, first) from the planted batch == two step_with_actions of random_acrobot_action's draws"""
    seed, first = 77, 3
    a, b = make(N, fused_step=fused), make(N, fused_step=fused)
    state, _, _ = planted_batch(0)
    for sim in (a, b):
        plant(sim, state)
    a.rollout_random(2, seed=seed, first_step=first)
    world = np.arange(N)
    finished = 0
    for k in range(2):
        b.step_with_actions(device_actions(random_acrobot_action(seed, first + k, world)))
        finished += int(cpu(b.reset_count_tensor())[0])
    assert finished > 100
    same(snapshot(a), snapshot(b), "rollout against single steps")
    assert np.array_equal(cpu(a.action_tensor())[:, 0], random_acrobot_action(seed, first + 1, world))
    assert next_episode_of(a, N + finished) and next_episode_of(b, N + finished)
    a.close()
    b.close()


def test_episode_statistics_from_far_states(hip_lib):
    """the kStats instance of the single-launch kernel: one step from the planted batch leaves what a simulator without
    statistics leaves, and every finished world's episode took one step"""
    state, action, where = planted_batch(0)
    plain, stats = make(N, fused_step=1), make(N, fused_step=1)
    for sim in (plain, stats):
        plant(sim, state)
    stats.enable_episode_stats()
    a = device_actions(action)
    plain.step_with_actions(a)
    stats.step_with_actions(a)
    same(snapshot(plain), snapshot(stats), "with episode statistics")
    done = cpu(stats.reset_tensor())[:, 0] != 0
    want_done, falls_back = planted_done()
    assert np.array_equal(done[where], want_done) and (want_done & falls_back).any()
    assert (cpu(stats.last_episode_steps_tensor()).reshape(N)[done] == 1).all()
    assert (cpu(stats.episode_steps_tensor()).reshape(N) == np.where(done, 0, 1)).all()
    assert stats.episode_totals()["episodes"] == int(done.sum())
    plain.close()
    stats.close()
