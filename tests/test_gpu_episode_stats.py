"""GPU: episode returns and lengths kept by the step (mrl_enable_episode_stats) in all six games.

The twin is the definition of include/mrl_envs.h restated in torch and fed with clones of REWARD / DONE after every single
step: per-world tensors must be equal exactly, TOTALS exactly where returns are integers and within the rounding bound of
its float64 additions for the balance beam.  Multi-step calls hide the intermediate REWARD / DONE, so there the twin is
fed by a second simulator B without statistics that is driven one step at a time by the same replayable stream, and at
the end every exported tensor of A must equal B's: enabling the statistics must not change the simulation.

Sizes: N = 1 and N = 1091 (two 1024-world workgroups, the last one partial and ending in a partial wave) for the games
with 1024 worlds per workgroup, N = 300 for those with 256."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd import _lib, layouts, simulators  # noqa: E402
from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AcrobotSimulator, BalanceBeamSimulator, CartpoleSimulator, ExecMode,  # noqa: E402
                                                        HanabiSimulator, OvercookedSimulator, SimplecookedSimulator)

HANABI = dict(colors=5, ranks=5, players=2, max_information_tokens=8, max_life_tokens=3)
# chosen with the CPU oracle (oracle.OvercookedOracle / SimplecookedOracle / HanabiOracle under the hash policy of
# mrl_rollout_random): cramped_room, horizon 20, seed 1, 45 steps -> 600 finished episodes of 300 worlds, 25 of them with a
# nonzero return; simple, horizon 20, seed 5, 45 steps, 70 worlds -> 5 such episodes; the full Hanabi game, seed 11: every
# one of 300 worlds has finished after 32 steps
COOKED_HORIZON, COOKED_SEED, COOKED_STEPS = 20, 1, 45
SIMPLE_SEED = 5
HANABI_SEED, HANABI_STEPS = 11, 40


class Twin:
    """The definition, in torch."""

    def __init__(self, n, players):
        self.n, self.P = n, players
        dev = "cuda"
        self.ret = torch.zeros(players, n, dtype=torch.float32, device=dev)
        self.last_ret = torch.zeros_like(self.ret)
        self.steps = torch.zeros(n, dtype=torch.int32, device=dev)
        self.last_steps = torch.zeros_like(self.steps)
        blocks = (n + 1023) // 1024
        self.totals = torch.zeros(blocks, 2 + players, dtype=torch.float64, device=dev)
        self.abs_return = torch.zeros(blocks, players, dtype=torch.float64, device=dev)  # sum of |return| per entry, for the bound
        self.block = torch.arange(n, device=dev) // 1024
        self.nonzero_finished = torch.zeros((), dtype=torch.int64, device=dev)  # finished episodes with a nonzero return

    def step(self, reward, done):
        r = reward.clone().reshape(self.P, self.n).to(torch.float32)
        d = done.clone().reshape(self.n) != 0
        self.ret += r  # one float32 add per step
        self.steps += 1
        self.last_ret = torch.where(d, self.ret, self.last_ret)
        self.last_steps = torch.where(d, self.steps, self.last_steps)
        w = d.to(torch.float64)
        contrib = torch.cat([w[:, None], (w * self.steps)[:, None], (w * self.ret.to(torch.float64)).t()], dim=1)
        self.totals.index_add_(0, self.block, contrib)
        self.abs_return.index_add_(0, self.block, contrib[:, 2:].abs())
        self.nonzero_finished += (d & (self.ret != 0).any(0)).sum()
        self.ret = torch.where(d, torch.zeros_like(self.ret), self.ret)
        self.steps = torch.where(d, torch.zeros_like(self.steps), self.steps)

    def reset(self, mask):
        m = mask.cuda() != 0
        self.ret = torch.where(m, torch.zeros_like(self.ret), self.ret)
        self.steps = torch.where(m, torch.zeros_like(self.steps), self.steps)


def views(sim):
    return {"ret": sim.episode_return_tensor().to_torch(), "steps": sim.episode_steps_tensor().to_torch(),
            "last_ret": sim.last_episode_return_tensor().to_torch(), "last_steps": sim.last_episode_steps_tensor().to_torch(),
            "totals": sim.episode_totals_tensor().to_torch()}


def check(sim, twin, exact_totals=True, what=""):
    v = views(sim)
    n, P = twin.n, twin.P
    assert v["ret"].shape == sim.reward_tensor().to_torch().shape and v["ret"].dtype == torch.float32
    done = sim.done_tensor() if hasattr(sim, "done_tensor") else sim.reset_tensor()
    assert v["steps"].shape == done.to_torch().shape and v["steps"].dtype == torch.int32
    assert v["totals"].shape == ((n + 1023) // 1024, 2 + P) and v["totals"].dtype == torch.float64
    assert torch.equal(v["ret"].reshape(P, n), twin.ret), f"EPISODE_RETURN {what}"
    assert torch.equal(v["steps"].reshape(n), twin.steps), f"EPISODE_STEPS {what}"
    assert torch.equal(v["last_ret"].reshape(P, n), twin.last_ret), f"LAST_RETURN {what}"
    assert torch.equal(v["last_steps"].reshape(n), twin.last_steps), f"LAST_STEPS {what}"
    if exact_totals:
        assert torch.equal(v["totals"], twin.totals), f"TOTALS {what}"
    else:
        assert torch.equal(v["totals"][:, :2], twin.totals[:, :2]), f"TOTALS counts {what}"
        # the rounding of the additions behind one entry: count * 2^-52 * sum |return|
        bound = twin.totals[:, :1] * 2.0 ** -52 * twin.abs_return
        error = (v["totals"][:, 2:] - twin.totals[:, 2:]).abs()
        print("TOTALS error / bound:", error.max().item(), bound.max().item())
        assert bool((error <= bound).all()), f"TOTALS returns {what}"
    sums = twin.totals.sum(0).tolist()
    totals = sim.episode_totals()
    assert totals["episodes"] == int(sums[0]) and totals["steps"] == int(sums[1]) and len(totals["returns"]) == P
    if exact_totals:
        assert totals["returns"] == sums[2:]
    return totals


def feed(twin, sim):
    done = sim.done_tensor() if hasattr(sim, "done_tensor") else sim.reset_tensor()
    twin.step(sim.reward_tensor().to_torch(), done.to_torch())


def exports(sim):
    """Every tensor the simulator exports besides the statistics."""
    names = [name for name in dir(type(sim)) if name.endswith("_tensor") and not name.startswith(("_", "episode_", "last_episode_"))]
    return {name: getattr(sim, name)().to_torch() for name in sorted(names)}


def same_exports(a, b):
    ea, eb = exports(a), exports(b)
    assert list(ea) == list(eb) and len(ea) >= 5
    for name in ea:
        assert torch.equal(ea[name], eb[name]), name


def captured(calls):
    """`calls` captured once into a HIP graph on a side stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            calls()
    torch.cuda.current_stream().wait_stream(side)
    return graph


# ---------------------------------------------------------------------------------------------------------------------
# 1. Cartpole
# ---------------------------------------------------------------------------------------------------------------------
def cartpole(n, stats=True, two_launches=False):
    with debug_knobs({"fused_step": 2} if two_launches else {}):
        sim = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    if stats:
        sim.enable_episode_stats()
    return sim


def cartpole_actions(n, steps, seed):
    w = np.arange(n)
    return torch.from_numpy(np.stack([simulators.random_cartpole_action(seed, k, w) for k in range(steps)])).cuda().view(steps, n, 1)


@pytest.mark.parametrize("path", ["single", "drawn", "two_launches", "phases"])
@pytest.mark.parametrize("n", [1, 1091])
def test_cartpole_single_steps(n, path, hip_lib):
    steps = 160
    sim = cartpole(n, two_launches=path == "two_launches")
    assert ("fused" in sim.kernel_name) == (path != "two_launches")
    twin = Twin(n, 1)
    acts = cartpole_actions(n, steps, 3)
    for k in range(steps):
        if path == "drawn":
            sim.rollout_random(1, seed=3, first_step=k)
        elif path == "phases":
            sim.step_phase1(acts[k])
            sim.step_phase2()
        else:
            sim.step_with_actions(acts[k])
        feed(twin, sim)
    totals = check(sim, twin, what=path)
    assert totals["episodes"] >= n and totals["steps"] == totals["returns"][0] >= 8 * totals["episodes"]
    sim.close()


@pytest.mark.parametrize("n", [1, 1091])
def test_cartpole_rollout_in_chunks_of_seven(n, hip_lib):
    steps = 160
    a, b = cartpole(n), cartpole(n, stats=False)
    assert a.rollout_kernel_name == "mrl_cartpole_step_fused" and b.rollout_kernel_name == "mrl_cartpole_rollout"
    twin = Twin(n, 1)
    for k0 in range(0, steps, 7):
        a.rollout_random(min(7, steps - k0), seed=5, first_step=k0)
    for k in range(steps):
        b.rollout_random(1, seed=5, first_step=k)
        feed(twin, b)
    assert check(a, twin)["episodes"] >= n
    same_exports(a, b)
    a.close()
    b.close()


@pytest.mark.parametrize("n", [1, 1091])
def test_cartpole_captured_steps_replayed(n, hip_lib):
    """3 steps captured once and replayed twice against 6 eager steps, after 40 eager steps on both sides so that episodes end
    inside the replays."""
    a, b = cartpole(n), cartpole(n, stats=False)
    a.prepare_graph_capture()
    twin = Twin(n, 1)
    for k in range(40):
        a.rollout_random(1, seed=8, first_step=k)
        b.rollout_random(1, seed=8, first_step=k)
        feed(twin, b)
    graph = captured(lambda: [a.rollout_random(1, seed=8, first_step=40 + k) for k in range(3)])
    check(a, twin, what="capturing runs nothing")
    for rep in range(2):
        graph.replay()
        for k in range(3):
            b.rollout_random(1, seed=8, first_step=40 + k)
            feed(twin, b)
    check(a, twin, what="after the replays")
    assert torch.equal(a.observation_tensor().to_torch(), b.observation_tensor().to_torch())
    assert torch.equal(a.reset_tensor().to_torch(), b.reset_tensor().to_torch())
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. Acrobot
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_launches", [False, True], ids=["single", "two_launches"])
def test_acrobot_truncation_then_random_play(two_launches, hip_lib):
    n = 1091
    with debug_knobs({"fused_step": 2} if two_launches else {}):
        sim = AcrobotSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    assert ("fused" in sim.kernel_name) == (not two_launches)
    sim.enable_episode_stats()
    twin = Twin(n, 1)
    hang = torch.ones(n, 1, dtype=torch.int32, device="cuda")  # zero torque: the episode runs into the 500-step limit
    for _ in range(503):
        sim.step_with_actions(hang)
        feed(twin, sim)
    v = views(sim)
    assert bool((v["last_steps"] == 501).all()) and bool((v["last_ret"] == -501).all()) and bool((v["steps"] == 2).all())
    assert v["totals"].sum(0).tolist() == [n, 501 * n, -501 * n]
    check(sim, twin, what="zero torque")
    for k in range(520):
        sim.rollout_random(1, seed=13, first_step=k)
        feed(twin, sim)
    assert check(sim, twin, what="random play")["episodes"] >= 2 * n
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. Balance beam
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_launches", [False, True], ids=["single", "two_launches"])
def test_balance_beam(two_launches, hip_lib):
    n = 1091
    with debug_knobs({"fused_step": 2} if two_launches else {}):
        sim = BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    assert ("fused" in sim.kernel_name) == (not two_launches)
    sim.enable_episode_stats()
    twin = Twin(n, 2)
    g = torch.Generator().manual_seed(17)
    for k in range(10):
        if k % 2:
            sim.rollout_random(1, seed=17, first_step=k)
        else:
            sim.step_with_actions(torch.randint(0, 4, (2, n, 1), dtype=torch.int32, generator=g).cuda())
        feed(twin, sim)
    totals = check(sim, twin, exact_totals=False)
    assert totals["episodes"] >= 3 * n and totals["returns"][0] == totals["returns"][1] != 0
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. Hanabi
# ---------------------------------------------------------------------------------------------------------------------
def hanabi(n, stats=True):
    sim = HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **HANABI)
    if stats:
        sim.enable_episode_stats()
    return sim


def test_hanabi_full_game(hip_lib):
    n = 300
    own, a, b = hanabi(n), hanabi(n), hanabi(n, stats=False)
    assert a.rollout_kernel_name == a.kernel_name != "mrl_hanabi_rollout"  # one step per launch, each followed by the update
    twin = Twin(n, 2)
    for k in range(HANABI_STEPS):
        own.rollout_random(1, seed=HANABI_SEED, first_step=k)
        feed(twin, own)
        b.rollout_random(1, seed=HANABI_SEED, first_step=k)
    for k0 in range(0, HANABI_STEPS, 5):
        a.rollout_random(5, seed=HANABI_SEED, first_step=k0)
    assert bool((twin.last_steps > 0).all()), "every world has finished at least once"
    totals = check(own, twin, what="one step per call")
    assert totals["episodes"] >= n
    check(a, twin, what="five steps per call")
    same_exports(a, b)
    same_exports(own, b)
    for sim in (own, a, b):
        sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. Overcooked and Simplecooked
# ---------------------------------------------------------------------------------------------------------------------
def cooked(n, stats=True, kind="overcooked"):
    if kind == "overcooked":
        params = layouts.get_base_layout_params("cramped_room", COOKED_HORIZON)
        sim = OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)
    else:
        params = layouts.get_simplecooked_layout_params("simple", COOKED_HORIZON)
        sim = SimplecookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)
    if stats:
        sim.enable_episode_stats()
    return sim


def cooked_actions(n, players, steps, seed):
    """The stream mrl_rollout_random draws, as (steps, P, N, 1) int32."""
    w = np.arange(n)
    acts = np.stack([np.stack([simulators.random_action(seed, k, w, np.full(n, p)) for p in range(players)]) for k in range(steps)])
    return torch.from_numpy(acts.astype(np.int32)).cuda().view(steps, players, n, 1)


def aligned_ring(slots, shape):
    stride = (int(np.prod(shape)) + 15) // 16 * 16
    inner = torch.empty(shape, dtype=torch.int8).stride()
    return torch.as_strided(torch.zeros(slots * stride, dtype=torch.int8, device="cuda"), (slots,) + shape, (stride,) + inner)


@pytest.mark.parametrize("path", ["with_actions", "i64", "many"])
def test_overcooked_single_steps(path, hip_lib):
    n = 300
    sim = cooked(n)
    other, alone = cooked(n, stats=False), cooked(n, stats=False)  # "many": a second simulator in the launch, without statistics
    twin = Twin(n, 2)
    acts = cooked_actions(n, 2, COOKED_STEPS, COOKED_SEED)
    flipped = acts.flip(1).contiguous()
    for k in range(COOKED_STEPS):
        if path == "with_actions":
            sim.step_with_actions(acts[k])
        elif path == "i64":
            sim.step_with_actions_i64(acts[k].to(torch.int64))
        else:
            simulators.step_many([sim, other], [acts[k], flipped[k]])
            alone.step_with_actions(flipped[k])
        feed(twin, sim)
    totals = check(sim, twin, what=path)
    assert totals["episodes"] == 2 * n and totals["steps"] == 2 * n * COOKED_HORIZON
    assert int(twin.nonzero_finished) > 0 and totals["returns"][0] != 0, "at least one finished episode has a nonzero return"
    if path == "many":
        same_exports(other, alone)
        for getter in (other.episode_return_tensor, other.episode_totals_tensor):
            with pytest.raises(MrlError, match="slot"):
                getter()
    for s in (sim, other, alone):
        s.close()


@pytest.mark.parametrize("path", ["sequence", "rollout"])
def test_overcooked_multi_step_calls_with_an_observation_ring(path, hip_lib):
    n, K = 300, 5
    a, b = cooked(n), cooked(n, stats=False)
    shape = tuple(a.observation_world_major_tensor().to_torch().shape)
    ring_a, ring_b = aligned_ring(3, shape), aligned_ring(3, shape)
    a.set_observation_ring(ring_a)
    b.set_observation_ring(ring_b)
    twin = Twin(n, 2)
    acts = cooked_actions(n, 2, COOKED_STEPS, COOKED_SEED)
    for k0 in range(0, COOKED_STEPS, K):
        if path == "sequence":
            a.step_sequence(acts[k0:k0 + K])
        else:
            a.rollout_random(K, seed=COOKED_SEED, first_step=k0)
    for k in range(COOKED_STEPS):
        if path == "sequence":
            b.step_with_actions(acts[k])
        else:
            b.rollout_random(1, seed=COOKED_SEED, first_step=k)
        feed(twin, b)
    totals = check(a, twin, what=path)
    assert totals["episodes"] == 2 * n and int(twin.nonzero_finished) > 0
    assert torch.equal(ring_a, ring_b)
    same_exports(a, b)
    a.close()
    b.close()


def test_overcooked_captured_steps_replayed(hip_lib):
    """3 steps captured once and replayed twice against 6 eager steps; 17 eager steps first, so that the horizon (20) falls
    inside the first replay."""
    n = 300
    a, b = cooked(n), cooked(n, stats=False)
    twin = Twin(n, 2)
    acts = cooked_actions(n, 2, 20, COOKED_SEED)
    for k in range(17):
        a.step_with_actions(acts[k])
        b.step_with_actions(acts[k])
        feed(twin, b)
    graph = captured(lambda: [a.step_with_actions(acts[17 + k]) for k in range(3)])
    for rep in range(2):
        graph.replay()
        for k in range(3):
            b.step_with_actions(acts[17 + k])
            feed(twin, b)
    assert check(a, twin)["episodes"] == n
    same_exports(a, b)
    a.close()
    b.close()


def test_simplecooked(hip_lib):
    n = 70
    sim = cooked(n, kind="simplecooked")
    twin = Twin(n, 2)
    acts = cooked_actions(n, 2, COOKED_STEPS, SIMPLE_SEED)
    for k in range(COOKED_STEPS):
        if k % 2:
            sim.step_with_actions(acts[k])
        else:
            sim.rollout_random(1, seed=SIMPLE_SEED, first_step=k)
        feed(twin, sim)
    totals = check(sim, twin)
    assert totals["episodes"] == 2 * n and int(twin.nonzero_finished) > 0
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. reset_worlds, 7. clear_episode_totals
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", ["cartpole", "overcooked"])
def test_reset_worlds_zeroes_running_values_only(game, hip_lib):
    if game == "cartpole":
        n, P, before, after = 1091, 1, 30, 130
        sim = cartpole(n)
        acts = cartpole_actions(n, before + after, 21)
    else:
        n, P, before, after = 300, 2, 33, 27
        sim = cooked(n)
        acts = cooked_actions(n, 2, before + after, COOKED_SEED)
    twin = Twin(n, P)
    for k in range(before):
        sim.step_with_actions(acts[k])
        feed(twin, sim)
    mask = torch.arange(n) % 3 == 0
    kept = {k: t.clone() for k, t in views(sim).items()}
    assert int(kept["steps"].reshape(n)[mask.cuda()].sum()) > 0 and float(kept["totals"][:, 0].sum()) > 0  # mid-episode, and episodes have ended
    sim.reset_worlds(mask)
    twin.reset(mask)
    now = views(sim)
    hit, rest = mask.cuda(), ~mask.cuda()
    assert int(now["steps"].reshape(n)[hit].abs().sum()) == 0 and float(now["ret"].reshape(P, n)[:, hit].abs().sum()) == 0
    assert torch.equal(now["steps"].reshape(n)[rest], kept["steps"].reshape(n)[rest])
    assert torch.equal(now["ret"].reshape(P, n)[:, rest], kept["ret"].reshape(P, n)[:, rest])
    for k in ("last_ret", "last_steps", "totals"):
        assert torch.equal(now[k], kept[k]), k
    check(sim, twin, what="right after the reset")
    # the next finished episode of a reset world counts only the steps since the reset
    seen = torch.zeros(n, dtype=torch.bool, device="cuda")
    too_long = torch.zeros((), dtype=torch.int64, device="cuda")
    for k in range(before, before + after):
        sim.step_with_actions(acts[k])
        feed(twin, sim)
        done = (sim.reset_tensor() if game == "cartpole" else sim.done_tensor()).to_torch().reshape(n) != 0
        first = done & hit & ~seen
        too_long += (first & (now["last_steps"].reshape(n) > k - before + 1)).sum()
        seen |= first
    check(sim, twin, what="after the reset")
    assert int(seen.sum()) > n // 6 and int(too_long) == 0
    sim.close()


def test_overcooked_reset_world_finishes_a_full_horizon_later(hip_lib):
    n = 300
    sim = cooked(n)
    acts = cooked_actions(n, 2, 33, COOKED_SEED)
    twin = Twin(n, 2)
    for k in range(7):
        sim.step_with_actions(acts[k])
        feed(twin, sim)
    mask = torch.arange(n) % 3 == 0
    sim.reset_worlds(mask)
    twin.reset(mask)
    for k in range(7, 33):
        sim.step_with_actions(acts[k])
        feed(twin, sim)
    check(sim, twin)
    last = views(sim)["last_steps"]
    assert bool((last[mask.cuda()] == COOKED_HORIZON).all()) and bool((last[~mask.cuda()] == COOKED_HORIZON).all())
    steps = views(sim)["steps"]
    assert bool((steps[mask.cuda()] == 33 - 7 - COOKED_HORIZON).all()) and bool((steps[~mask.cuda()] == 33 - COOKED_HORIZON).all())
    sim.close()


def test_clear_episode_totals_zeroes_totals_only(hip_lib):
    n = 1091
    sim = cartpole(n)
    sim.rollout_random(50, seed=2)
    kept = {k: t.clone() for k, t in views(sim).items()}
    assert sim.episode_totals()["episodes"] > 0
    sim.clear_episode_totals()
    now = views(sim)
    assert float(now["totals"].abs().sum()) == 0 and sim.episode_totals() == {"episodes": 0, "steps": 0, "returns": [0.0]}
    for k in ("ret", "steps", "last_ret", "last_steps"):
        assert torch.equal(now[k], kept[k]), k
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. Enabling
# ---------------------------------------------------------------------------------------------------------------------
def test_enabling(hip_lib):
    sim = cartpole(300, stats=False)
    for slot in range(64, 69):
        desc = _lib.TensorDesc()
        assert hip_lib.mrl_tensor(sim._handle, slot, ctypes.byref(desc)) == _lib.MRL_ERR_SLOT
    with pytest.raises(MrlError, match="slot 68"):
        sim.episode_totals_tensor()
    with pytest.raises(MrlError, match="mrl_enable_episode_stats first"):
        sim.clear_episode_totals()
    x = torch.zeros(4, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with pytest.raises(MrlError, match="capturing stream"):
            with torch.cuda.graph(graph, stream=side):
                x.add_(1)
                sim.enable_episode_stats()
    torch.cuda.current_stream().wait_stream(side)
    with pytest.raises(MrlError, match="slot 64"):
        sim.episode_return_tensor()
    sim.enable_episode_stats()
    sim.rollout_random(20, seed=1)
    first = {k: (t.data_ptr(), t.clone()) for k, t in views(sim).items()}
    sim.enable_episode_stats()  # a second call changes nothing
    sim._tensors.clear()
    for k, t in views(sim).items():
        assert t.data_ptr() == first[k][0] and torch.equal(t, first[k][1]), k
    assert int(first["steps"][1].max()) > 0
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. The env wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_cartpole_env_wrapper_against_the_reference_scripts_bookkeeping(hip_lib):
    from madrona_rl_envs_playground_amd.envs.cartpole_env import CartpoleMadronaTorch
    n = 1091
    env = CartpoleMadronaTorch(n, 0, record_episode_statistics=True)
    ep_rewards = torch.zeros(n, device="cuda")
    rewsum = torch.zeros((), device="cuda")
    numfin = torch.zeros((), device="cuda")
    g = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(60):
        _, rewards, next_done, infos = env.step(torch.randint(0, 2, (n,), dtype=torch.int32, device="cuda", generator=g))
        assert infos == [{}] * n
        # scripts/cartpole_train_torch.py:223-226 of the reference
        ep_rewards += rewards[:, 0]
        rewsum += torch.sum(torch.where(next_done == 1, ep_rewards, 0))
        numfin += torch.sum(next_done)
        ep_rewards *= 1 - next_done
    totals = env.episode_totals()
    assert totals == {"episodes": int(numfin), "steps": int(rewsum), "returns": [float(rewsum)]} and totals["episodes"] >= n
    assert torch.equal(env.episode_stats.episode_return[:, 0], ep_rewards)
    assert env.episode_stats.totals.shape == (2, 3) and env.episode_stats.last_steps.shape == (n, 1)
    env.clear_episode_totals()
    assert env.episode_totals()["episodes"] == 0
    env.close()
