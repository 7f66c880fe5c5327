"""GPU: restarting chosen worlds (mrl_reset_worlds / reset_worlds / n_reset(worlds=...)) in all five games.

Overcooked and Simplecooked: after t steps a random ~30 % of the worlds restart; for K more steps those worlds equal a fresh
simulator that ran only the K steps, the others one that ran all t + K -- observations (wherever the step writes them),
rewards, done flags and STATE_* tensors, after every step.  Hanabi, Cartpole and the balance beam: the restarted worlds
take the episodes counter, counter + 1, ... (checked against the CPU oracles and a simulator re-seeded at that index), the
next natural episode ends go on from counter + M, and the restarted worlds step in lock-step with that simulator until one
of them finishes -- by default, after mrl_prepare_graph_capture, under the persistent random-policy rollout and inside a
captured HIP graph."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd import hanabi_spec, layouts  # noqa: E402
from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (BalanceBeamSimulator, CartpoleSimulator, ExecMode, HanabiSimulator,  # noqa: E402
                                                        OvercookedSimulator, SimplecookedSimulator)

HANABI = dict(colors=5, ranks=5, players=2, max_information_tokens=8, max_life_tokens=3)
HORIZON = 200


def pick(n, density, seed):
    """A random mask over n worlds with world 0 set and world 1 clear (host, bool)."""
    mask = torch.rand(n, generator=torch.Generator().manual_seed(seed)) < density
    mask[0], mask[1] = True, False
    return mask


def split(mask):
    return mask.nonzero()[:, 0].cuda(), (~mask).nonzero()[:, 0].cuda()


def same(got, want, worlds, keys, what):
    for k in keys:
        g, axis = got[k]
        w, _ = want[k]
        assert torch.equal(g.index_select(axis, worlds), w.index_select(axis, worlds)), f"{k}: {what}"


def snapshot(tensors):
    return {k: (t.clone(), axis) for k, (t, axis) in tensors.items()}


# ---------------------------------------------------------------------------------------------------------------------
# Overcooked and Simplecooked
# ---------------------------------------------------------------------------------------------------------------------
COOKED = {
    "cramped_room_32768": ("overcooked", "cramped_room", None, 32768),   # the fixed-layout kernel
    "schelling_130": ("overcooked", "multiplayer_schelling", None, 130),  # the generic kernel, four players
    "many_player_50": ("overcooked", "many_player_layout", 2, 50),        # few worlds of a large layout: the team kernel
    "simple_4099": ("simplecooked", "simple", None, 4099),
}
COOKED_STATE = ["obs", "players", "objects", "timestep", "dishes"]
COOKED_ALL = COOKED_STATE + ["reward", "done"]


def cooked_sim(case):
    kind, layout, players, n = COOKED[case]
    if kind == "overcooked":
        params = layouts.get_base_layout_params(layout, HORIZON, max_num_players=players)
        return OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)
    params = layouts.get_simplecooked_layout_params(layout, HORIZON)
    return SimplecookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)


def cooked_tensors(sim, obs=None):
    """name -> (tensor, world axis); `obs`: where the simulator's observations go if not its own tensor."""
    t = {"obs": (sim.observation_world_major_tensor().to_torch() if obs is None else obs, 0),
         "players": (sim.state_players_tensor().to_torch(), 0),
         "objects": (sim.state_objects_tensor().to_torch(), 0),
         "timestep": (sim.state_timestep_tensor().to_torch(), 0),
         "reward": (sim.reward_tensor().to_torch(), 1),
         "done": (sim.done_tensor().to_torch(), 0)}
    t["dishes"] = (sim.dishes_out_tensor().to_torch(), 0) if isinstance(sim, SimplecookedSimulator) else t["timestep"]
    return t


def aligned_ring(slots, shape):
    """A zeroed ring of observation slots on 16-byte boundaries (a dense ring of slabs that are not a multiple of 16 bytes
    long would be staged, which a reset refuses)."""
    stride = (int(np.prod(shape)) + 15) // 16 * 16
    inner = torch.empty(shape, dtype=torch.int8).stride()
    return torch.as_strided(torch.zeros(slots * stride, dtype=torch.int8, device="cuda"), (slots,) + shape, (stride,) + inner)


def cooked_exports(sim):
    names = ["done_tensor", "active_agent_tensor", "action_tensor", "observation_tensor", "action_mask_tensor", "reward_tensor",
             "observation_world_major_tensor", "state_players_tensor", "state_objects_tensor", "state_timestep_tensor"]
    if isinstance(sim, SimplecookedSimulator):
        names.append("dishes_out_tensor")
    return {name: getattr(sim, name)().to_torch() for name in names}


@pytest.mark.parametrize("output", ["own", "slot", "ring"])
@pytest.mark.parametrize("case", list(COOKED))
def test_cooked_restart_equals_fresh_simulator(case, output, hip_lib):
    t, K = 23, 12
    sim, full, fresh = cooked_sim(case), cooked_sim(case), cooked_sim(case)
    n = sim.num_worlds
    P = sim.action_tensor().to_torch().shape[0]
    acts = torch.randint(0, 6, (t + K, P, n, 1), dtype=torch.int32, generator=torch.Generator().manual_seed(7)).cuda()
    mask = pick(n, 0.3, 8)
    sel, rest = split(mask)
    shape = tuple(sim.observation_world_major_tensor().to_torch().shape)
    ring = None
    if output == "slot":
        ring = torch.zeros((1,) + shape, dtype=torch.int8, device="cuda")
        sim.set_observation_output(ring[0])
    elif output == "ring":
        ring = aligned_ring(3, shape)
        sim.set_observation_ring(ring)

    def obs_of(k):  # where step k (counted from the redirection) wrote
        return None if ring is None else ring[k % ring.shape[0]]

    for k in range(t):
        sim.step_with_actions(acts[k])
        full.step_with_actions(acts[k])
    before = snapshot(cooked_tensors(sim, obs_of(t - 1)))
    sim.reset_worlds(mask)
    now = cooked_tensors(sim, obs_of(t - 1))  # the reset writes where the last step wrote
    same(now, cooked_tensors(full), rest, COOKED_ALL, "unmasked world changed by the reset")
    same(now, cooked_tensors(fresh), sel, COOKED_STATE, "restarted world differs from a new simulator's")
    assert int(now["timestep"][0][sel].abs().sum()) == 0
    same(now, before, sel, ["reward", "done"], "a per-step output changed")
    for k in range(t, t + K):
        for s in (sim, full, fresh):
            s.step_with_actions(acts[k])
        now = cooked_tensors(sim, obs_of(k))
        same(now, cooked_tensors(full), rest, COOKED_ALL, f"unmasked world, step {k}")
        same(now, cooked_tensors(fresh), sel, COOKED_ALL, f"restarted world, step {k}")
    for s in (sim, full, fresh):
        s.close()


@pytest.mark.parametrize("case", list(COOKED))
def test_cooked_empty_mask_changes_nothing(case, hip_lib):
    sim = cooked_sim(case)
    n = sim.num_worlds
    P = sim.action_tensor().to_torch().shape[0]
    g = torch.Generator().manual_seed(3)
    for _ in range(9):
        sim.step_with_actions(torch.randint(0, 6, (P, n, 1), dtype=torch.int32, generator=g).cuda())
    before = {k: v.clone() for k, v in cooked_exports(sim).items()}
    sim.reset_worlds(torch.zeros(n, dtype=torch.uint8))
    sim.reset_worlds(torch.zeros(n, dtype=torch.int64, device="cuda"))
    for k, v in cooked_exports(sim).items():
        assert torch.equal(v, before[k]), k
    ring = aligned_ring(2, tuple(before["observation_world_major_tensor"].shape))
    sim.set_observation_ring(ring)
    sim.rollout_random(3, seed=4)
    kept = ring.clone()
    sim.reset_worlds(torch.zeros(n, dtype=torch.bool))
    assert torch.equal(ring, kept)
    sim.close()


def test_cooked_reset_before_any_step_writes_where_the_next_step_will(hip_lib):
    sim, fresh = cooked_sim("schelling_130"), cooked_sim("schelling_130")
    n = sim.num_worlds
    P = sim.action_tensor().to_torch().shape[0]
    for _ in range(5):
        sim.step_with_actions(torch.randint(0, 6, (P, n, 1), dtype=torch.int32).cuda())
    own = sim.observation_world_major_tensor().to_torch().clone()
    slot = torch.zeros_like(own)
    sim.set_observation_output(slot)
    mask = pick(n, 0.3, 9)
    sel, rest = split(mask)
    sim.reset_worlds(mask.to(torch.int32) * 256)  # any nonzero integer restarts its world
    fresh_obs = fresh.observation_world_major_tensor().to_torch()
    assert torch.equal(slot[sel], fresh_obs[sel])
    assert int(slot[rest].abs().sum()) == 0
    assert torch.equal(sim.observation_world_major_tensor().to_torch(), own)  # the simulator's own tensor is not the output
    sim.step_with_actions(torch.zeros((P, n, 1), dtype=torch.int32, device="cuda"))
    fresh.step_with_actions(torch.zeros((P, n, 1), dtype=torch.int32, device="cuda"))
    assert torch.equal(slot[sel], fresh_obs[sel])


def test_cooked_staged_output_is_refused_and_bad_masks_raise(hip_lib):
    sim = cooked_sim("schelling_130")
    n = sim.num_worlds
    shape = tuple(sim.observation_world_major_tensor().to_torch().shape)
    nbytes = int(np.prod(shape))
    buf = torch.zeros(nbytes + 16, dtype=torch.int8, device="cuda")
    slot = buf[1:1 + nbytes].view(shape)  # off a 16-byte boundary: staged
    sim.set_observation_output(slot)
    sim.step_with_actions(torch.ones((shape[1], n, 1), dtype=torch.int32, device="cuda"))
    before = {k: v.clone() for k, v in cooked_exports(sim).items()}
    kept = buf.clone()
    with pytest.raises(MrlError, match="staged"):
        sim.reset_worlds(pick(n, 0.3, 1))
    for k, v in cooked_exports(sim).items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(buf, kept)
    sim.set_observation_output(None)
    sim.reset_worlds(pick(n, 0.3, 1))
    with pytest.raises(ValueError):
        sim.reset_worlds(torch.ones(n + 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        sim.reset_worlds(torch.ones(n, dtype=torch.float32))
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# Hanabi, Cartpole, balance beam: episode numbering
# ---------------------------------------------------------------------------------------------------------------------
def counter_sim(game, n, knobs=None):
    with debug_knobs(knobs or {}):
        if game == "hanabi":
            return HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **HANABI)
        if game == "cartpole":
            return CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
        return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)


STATE_KEYS = {"hanabi": ["obs", "state", "mask", "active", "game"], "cartpole": ["state"], "balance": ["obs", "active", "mask"]}
STEP_KEYS = ["reward", "done", "action"]


def counter_tensors(game, sim):
    if game == "hanabi":
        return {"obs": (sim.observation_tensor().to_torch(), 1), "state": (sim.agent_state_tensor().to_torch(), 1),
                "mask": (sim.action_mask_tensor().to_torch(), 1), "active": (sim.active_agent_tensor().to_torch(), 1),
                "game": (sim.game_tensor().to_torch(), 0), "reward": (sim.reward_tensor().to_torch(), 1),
                "done": (sim.done_tensor().to_torch(), 0), "action": (sim.action_tensor().to_torch(), 1)}
    if game == "cartpole":
        return {"state": (sim.observation_tensor().to_torch(), 0), "reward": (sim.reward_tensor().to_torch(), 0),
                "done": (sim.reset_tensor().to_torch(), 0), "action": (sim.action_tensor().to_torch(), 0)}
    return {"obs": (sim.observation_tensor().to_torch(), 1), "active": (sim.active_agent_tensor().to_torch(), 1),
            "mask": (sim.action_mask_tensor().to_torch(), 1), "reward": (sim.reward_tensor().to_torch(), 1),
            "done": (sim.done_tensor().to_torch(), 0), "action": (sim.action_tensor().to_torch(), 1)}


def counter_globals(game, sim):
    out = {"reset_count": sim.reset_count_tensor().to_torch(), "shard_count": sim.shard_count_tensor().to_torch()}
    if game != "balance":
        out["scan_timeout"] = sim.scan_timeout_tensor().to_torch()
    return out


def done_of(game, sim):
    d = sim.reset_tensor().to_torch()[:, 0] if game == "cartpole" else sim.done_tensor().to_torch()
    return d != 0


def reseeded(game, n, first_episode):
    """A new simulator of n worlds whose world j holds episode first_episode + j, counter first_episode + n."""
    r = counter_sim(game, n)
    r.reseed_shard(first_episode, first_episode + n)
    return r


def random_actions(game, sim, rng):
    n = sim.num_worlds
    if game == "hanabi":
        mask = sim.action_mask_tensor().to_torch().cpu().numpy()
        return torch.from_numpy((rng.random(mask.shape) * (mask != 0)).argmax(-1).astype(np.int32)).view(2, n, 1).cuda()
    if game == "cartpole":
        return torch.from_numpy(rng.integers(0, 2, (n, 1)).astype(np.int32)).cuda()
    return torch.from_numpy(rng.integers(0, 4, (2, n, 1)).astype(np.int32)).cuda()


def check_against_oracle(game, sim, sel, first, oracle_lib):
    """The worlds `sel` of `sim` hold episodes first, first + 1, ... as the CPU oracles build them."""
    m = int(sel.numel())
    if game == "hanabi":
        orc = oracle_lib.HanabiOracle(HANABI, m, num_threads=8, first_episode=first)
        no, ns = hanabi_spec.observation_size(HANABI), hanabi_spec.state_size(HANABI)
        idx = sel.cpu().numpy()
        assert np.array_equal(sim.observation_tensor().to_torch().cpu().numpy().astype(np.uint8)[:, idx, :no], orc.obs[..., :no])
        assert np.array_equal(sim.agent_state_tensor().to_torch().cpu().numpy().astype(np.uint8)[:, idx, :ns], orc.state[..., :ns])
        assert np.array_equal(sim.action_mask_tensor().to_torch().cpu().numpy()[:, idx], orc.mask)
        assert np.array_equal(sim.active_agent_tensor().to_torch().cpu().numpy()[:, idx], orc.active)
        assert np.array_equal(sim.game_tensor().to_torch().cpu().numpy()[idx], orc.dump())
        return orc
    if game == "cartpole":
        got = sim.observation_tensor().to_torch()[sel].cpu().numpy()
        orc = oracle_lib.CartpoleOracle(first + m)
        assert np.array_equal(got.view(np.uint32), orc.state[first:].view(np.uint32))
        for j in sorted({0, m // 2, m - 1}):  # the reference's reset formula on the episode's generator, sim.cpp:48-66
            want = (np.float32(-0.05) + oracle_lib.rng_stream(first + j, 4) * np.float32(0.1)).astype(np.float32)
            assert np.array_equal(got[j].view(np.uint32), want.view(np.uint32))
        return None
    orc = oracle_lib.BalanceOracle(first + m)
    assert np.array_equal(sim.observation_tensor().to_torch()[:, sel].cpu().numpy(), orc.obs[:, first:])
    return None


def warm_up(game, sim, steps, seed):
    """`steps` random-policy steps; returns the episode counter after them."""
    counter = sim.num_worlds
    for k in range(steps):
        sim.rollout_random(1, seed=seed, first_step=k)
        counter += int(sim.reset_count_tensor().to_torch().item())
    return counter


COUNTER_CASES = [("hanabi", 65536, 30), ("hanabi", 9001, 30), ("cartpole", 1 << 20, 12), ("cartpole", 1000, 12), ("cartpole", 70000, 12),
                 ("balance", 4100, 5)]


@pytest.mark.parametrize("prepared", [False, True], ids=["host_state", "after_prepare"])
@pytest.mark.parametrize("game,n,t", COUNTER_CASES, ids=[f"{g}_{n}" for g, n, _ in COUNTER_CASES])
def test_restarted_episodes_are_numbered_from_the_counter(game, n, t, prepared, hip_lib, oracle_lib):
    sim = counter_sim(game, n)
    if prepared:
        sim.prepare_graph_capture()
    c = warm_up(game, sim, t, seed=11)
    mask = pick(n, 0.3, 12)
    sel, rest = split(mask)
    m = int(sel.numel())
    before, before_g = snapshot(counter_tensors(game, sim)), {k: v.clone() for k, v in counter_globals(game, sim).items()}
    sim.reset_worlds(mask)
    now = counter_tensors(game, sim)
    same(now, before, rest, STATE_KEYS[game] + STEP_KEYS, "unmasked world changed by the reset")
    same(now, before, sel, STEP_KEYS, "a per-step output changed")
    for k, v in counter_globals(game, sim).items():
        assert torch.equal(v, before_g[k]), k
    orc = check_against_oracle(game, sim, sel, c, oracle_lib)
    twin = reseeded(game, m, c)  # a new simulator whose world j is episode c + j
    for k in STATE_KEYS[game]:
        g, axis = now[k]
        assert torch.equal(g.index_select(axis, sel), counter_tensors(game, twin)[k][0]), f"{k}: restarted world vs re-seeded simulator"
    # lock-step: the restarted worlds go on like the twin's until one of them finishes; the first natural episode ends take
    # c + M, c + M + 1, ... in ascending world order
    rng = np.random.default_rng(13)
    numbered = lockstep = False
    for step in range(60):
        a = random_actions(game, sim, rng)
        sim.step_with_actions(a)
        twin.step_with_actions(a.index_select(1 if a.dim() == 3 else 0, sel).contiguous())
        done = done_of(game, sim)
        ended = done.nonzero()[:, 0]
        assert int(sim.reset_count_tensor().to_torch().item()) == int(ended.numel())
        if not lockstep:
            if bool(done[sel].any()):
                lockstep = True  # a restarted world finished: its next episode is numbered among all worlds from here on
            else:
                got = counter_tensors(game, sim)
                want = counter_tensors(game, twin)
                for k in STATE_KEYS[game] + ["reward", "done"]:
                    g, axis = got[k]
                    w, _ = want[k]
                    assert torch.equal(g.index_select(axis, sel), w), f"{k}: restarted world vs twin, step {step}"
                if orc is not None:
                    orc.step(a.index_select(1, sel).cpu().numpy()[..., 0])
                    assert np.array_equal(sim.game_tensor().to_torch().cpu().numpy()[sel.cpu().numpy()], orc.dump()), f"step {step}"
        if not numbered and ended.numel():
            check_against_oracle(game, sim, ended, c + m, oracle_lib)
            numbered = True
        if numbered and lockstep:
            break
    assert numbered
    assert not sim.scan_timed_out
    if game != "balance":
        assert int(sim.scan_timeout_tensor().to_torch().item()) == 0
    sim.close()
    twin.close()


@pytest.mark.parametrize("game", ["hanabi", "cartpole", "balance"])
def test_empty_mask_leaves_the_counter(game, hip_lib):
    n = {"hanabi": 9001, "cartpole": 5000, "balance": 3000}[game]
    sim, twin = counter_sim(game, n), counter_sim(game, n)
    for s in (sim, twin):
        warm_up(game, s, 6, seed=2)
    before = snapshot(counter_tensors(game, sim))
    sim.reset_worlds(torch.zeros(n, dtype=torch.bool))
    same(counter_tensors(game, sim), before, torch.arange(n, device="cuda"), list(before), "empty mask changed a tensor")
    for k in range(6, 16):  # the counter too: later episodes are numbered as on the twin
        sim.rollout_random(1, seed=2, first_step=k)
        twin.rollout_random(1, seed=2, first_step=k)
        same(counter_tensors(game, sim), counter_tensors(game, twin), torch.arange(n, device="cuda"), list(before), f"step {k}")


@pytest.mark.parametrize("game,n", [("hanabi", 65536), ("cartpole", 1 << 20)])
def test_persistent_rollout_continues_from_the_reset(game, n, hip_lib):
    """The one-launch rollout after a reset equals the same draws one launch per step."""
    one = counter_sim(game, n)
    many = counter_sim(game, n, {f"{game}.no_persistent": 1})
    mask = pick(n, 0.3, 21)
    for s in (one, many):
        warm_up(game, s, 8, seed=5)
        s.reset_worlds(mask)
    assert one.rollout_kernel_name == f"mrl_{game}_rollout" and many.rollout_kernel_name != one.rollout_kernel_name
    one.rollout_random(25, seed=6, first_step=100)
    many.rollout_random(25, seed=6, first_step=100)
    a, b = counter_tensors(game, one), counter_tensors(game, many)
    same(a, b, torch.arange(n, device="cuda"), list(a), "persistent vs one launch per step")
    assert torch.equal(one.reset_count_tensor().to_torch(), many.reset_count_tensor().to_torch())
    for s in (one, many):
        s.reset_worlds(mask)  # and the counters agree: the next restarts are the same episodes
    same(counter_tensors(game, one), counter_tensors(game, many), torch.arange(n, device="cuda"), STATE_KEYS[game], "second reset")


@pytest.mark.parametrize("game,n", [("hanabi", 9001), ("cartpole", 70000), ("balance", 4100)])
def test_reset_replays_from_a_captured_graph(game, n, hip_lib):
    """[reset, K random-policy steps] captured after mrl_prepare_graph_capture and replayed three times equals the same calls
    issued one by one on a simulator that keeps its counter state on the host."""
    graphed, eager = counter_sim(game, n), counter_sim(game, n)
    graphed.prepare_graph_capture()
    for s in (graphed, eager):
        warm_up(game, s, 5, seed=8)
    mask = pick(n, 0.3, 22).cuda()
    graphed.reset_worlds(torch.zeros(n, dtype=torch.bool, device="cuda"))  # (the simulator's mask buffer exists before the capture)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            graphed.reset_worlds(mask)
            graphed.rollout_random(4, seed=9, first_step=40)
    torch.cuda.current_stream().wait_stream(side)
    for rep in range(3):
        graph.replay()
        eager.reset_worlds(mask)
        eager.rollout_random(4, seed=9, first_step=40)
        a, b = counter_tensors(game, graphed), counter_tensors(game, eager)
        same(a, b, torch.arange(n, device="cuda"), list(a), f"replay {rep}")
        assert torch.equal(graphed.reset_count_tensor().to_torch(), eager.reset_count_tensor().to_torch())


def test_refusals(hip_lib):
    sharded = counter_sim("cartpole", 1000)
    sharded.reseed_shard(1000, 2000)
    with pytest.raises(MrlError, match="shard"):
        sharded.reset_worlds()
    mailbox = counter_sim("hanabi", 700)
    mailbox.exchange_create(1, 0)
    with pytest.raises(MrlError, match="shard"):
        mailbox.reset_worlds(torch.ones(700, dtype=torch.bool))
    free = counter_sim("balance", 300)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    x = torch.zeros(4, device="cuda")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with pytest.raises(MrlError, match="mrl_prepare_graph_capture"):
            with torch.cuda.graph(graph, stream=side):
                x.add_(1)
                free.reset_worlds()
    torch.cuda.current_stream().wait_stream(side)
    for s in (sharded, mailbox, free):
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# The env wrappers
# ---------------------------------------------------------------------------------------------------------------------
def test_env_n_reset(hip_lib):
    from madrona_rl_envs_playground_amd.envs.overcooked_env import OvercookedMadrona
    n = 600
    env, fresh = OvercookedMadrona("cramped_room", n, 0, horizon=80), OvercookedMadrona("cramped_room", n, 0, horizon=80)
    P = env.num_players
    g = torch.Generator().manual_seed(31)
    for _ in range(37):
        env.n_step(torch.randint(0, 6, (P, n, 1), generator=g).cuda())
    sim = env.sim
    state = [sim.state_players_tensor().to_torch().clone(), sim.state_objects_tensor().to_torch().clone(),
             sim.state_timestep_tensor().to_torch().clone()]
    before = [o.obs.clone() for o in env.get_obs()]
    obs = env.n_reset()  # as today: the current observations, nothing restarts
    assert all(torch.equal(o.obs, b) for o, b in zip(obs, before))
    assert all(torch.equal(a, b) for a, b in zip(state, [sim.state_players_tensor().to_torch(), sim.state_objects_tensor().to_torch(),
                                                           sim.state_timestep_tensor().to_torch()]))
    mask = pick(n, 0.3, 32)
    sel, rest = split(mask)
    obs = env.n_reset(worlds=mask)
    for o, w, b in zip(obs, fresh.n_reset(), before):
        assert torch.equal(o.obs[sel], w.obs[sel]) and torch.equal(o.obs[rest], b[rest])
    env.close()
    fresh.close()


def test_tester_style_evaluation_starts_at_step_zero(hip_lib, oracle_lib):
    """train/tester.py: n_reset, then env_length steps summing rewards.  After a training run left the worlds mid-episode,
    n_reset(worlds=all) makes the sums those of whole episodes from step 0, as the oracle plays them."""
    from madrona_rl_envs_playground_amd.envs.overcooked_env import OvercookedMadrona
    n, horizon = 512, 60
    env = OvercookedMadrona("coordination_ring", n, 0, horizon=horizon)
    P = env.num_players
    g = torch.Generator().manual_seed(41)
    for _ in range(horizon + 23):
        env.n_step(torch.randint(0, 6, (P, n, 1), generator=g).cuda())
    env.n_reset(worlds=torch.ones(n, dtype=torch.bool))
    orc = oracle_lib.OvercookedOracle(layouts.get_base_layout_params("coordination_ring", horizon), n, num_threads=8)
    score, want = np.zeros((P, n), np.int64), np.zeros((P, n), np.int64)
    for k in range(horizon):
        a = torch.randint(0, 6, (P, n, 1), generator=g)
        _, rew, done, _ = env.n_step(a.cuda())
        orc.step(a.numpy())
        score += rew.cpu().numpy()
        want += orc.reward
        assert np.array_equal(done.cpu().numpy(), orc.done), f"done, step {k}"
    assert np.array_equal(score, want)
    assert bool(done.all())  # the episode that began at the reset ended at the horizon, in every world
    env.close()
