"""The Hanabi kernels on games other than full, small and very_small (tests/hanabi_configs.py): the "any configuration"
code variant with ranks != 5 -- card / R, card % R, the hint masks and every section offset computed at run time, with
more colours than ranks, fewer, and as many --, and the five-rank variant with 3, 4 and 5 colours and other token pools.
Every comparison is bit-exact: against the CPU oracle (pinned to the reference's own sim.cpp in these very games by
test_ref_hanabi.py), against the compiled reference itself where it was built, and between the kernels that must agree
(one launch per step, two, the persistent rollout, a captured graph).

World counts are small on purpose: a workgroup owns 256 worlds, so 700 are three workgroups with a ragged last one --
the smallest shape in which the look-back over lower workgroups, the ragged tail and the compaction of restarted worlds all
take part."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hanabi_configs  # noqa: E402
from hanabi_configs import BY_ID, choose, config  # noqa: E402
from madrona_rl_envs_playground_amd import hanabi_spec  # noqa: E402
from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import _DeviceBlob  # noqa: E402
from test_gpu_hanabi import compare, compare_ref, legal_random, make  # noqa: E402

N = hanabi_configs.WALK_WORLDS
NAMES = ["observation_tensor", "agent_state_tensor", "action_mask_tensor", "active_agent_tensor", "reward_tensor", "done_tensor",
         "game_tensor", "reset_count_tensor"]
AGENT_BLOCK = 896  # state row 784 | legal-move mask 80 | pad 32 (csrc/hanabi.hip: kAgentBlock)


def device_actions(a, n):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda().view(2, n, 1)


def step(sim, fused, a):
    """One step on actions `a` (2, n, 1): mrl_step, or the two-phase pair."""
    if fused == 1:
        sim.action_tensor().to_torch().copy_(a)
        sim.step()
    else:
        sim.step_phase1(a)
        sim.step_phase2(None)


def no_timeout(*sims):
    for s in sims:
        assert int(s.scan_timeout_tensor().to_torch().item()) == 0 and not s.scan_timed_out


def same_tensors(a, b, tag, names=NAMES):
    for name in names:
        assert torch.equal(getattr(a, name)().to_torch(), getattr(b, name)().to_torch()), f"{name} differs {tag}"


def blocks(sim):
    """Everything the step writes for the agents, (N, 2, 896) uint8: the rows the exported tensors are views of, with the
    bytes past state_size and the pad, which no tensor shows."""
    t = sim.agent_state_tensor()
    blob = _DeviceBlob(sim, t.ptr, (sim.num_worlds, 2, AGENT_BLOCK), (2 * AGENT_BLOCK, AGENT_BLOCK, 1), "|u1")
    return torch.as_tensor(blob, device=torch.device("cuda", t.device))


# ---------------------------------------------------------------------------------------------------------------------
# Lock-step against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 2], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("cid", hanabi_configs.IDS)
def test_lockstep_vs_oracle(cid, fused, hip_lib, oracle_lib):
    """hanabi_configs.walk: the policies that force the rare paths, driven by the oracle's mask and records.  Its CPU twin
    (test_oracle_hanabi.py:test_lockstep_walk_reaches_every_path) asserts that this very walk takes every reachable path
    and ends episodes, so the inputs here are known to contain them."""
    cfg = BY_ID[cid]
    no, ns, moves = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg), hanabi_spec.num_moves(cfg)
    with debug_knobs({"fused_step": fused}):
        sim = make(cfg, N)
    assert sim.kernel_name == ("mrl_hanabi_step_fused" if fused == 1 else "mrl_hanabi_step")
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=8)
    assert sim.observation_tensor().to_torch().shape == (2, N, no) and no <= ns <= 783
    mask = sim.action_mask_tensor().to_torch()
    compare(sim, orc, "initial", cfg)
    assert not mask[..., moves:].any()
    finished = 0
    for t, _, acts in hanabi_configs.walk(orc, cfg, hanabi_configs.WALK_STEPS[cid]):
        step(sim, fused, device_actions(acts, N))
        compare(sim, orc, f"step {t}", cfg)
        assert not mask[..., moves:].any(), f"step {t}: a legal move beyond the game's {moves}"
        assert int(sim.reset_count_tensor().to_torch().item()) == int(orc.done.sum()), f"step {t}: reset count"
        finished += int(orc.done.sum())
    assert finished > 0
    no_timeout(sim)
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# What the reference leaves undefined: the state row past state_size and the pad
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["k5r3i8l3", "k2r4i1l1", "k3r3i4l2"], ids=["more_colours_than_ranks", "fewer", "as_many"])
def test_whole_blocks_agree_between_the_kernels(cid, hip_lib):
    """The 896-byte blocks, whole, after every one of 60 steps: the one-launch step, the two-launch pair and the persistent
    rollout (which draws the moves; the two others replay them) leave the same bytes, also where no tensor shows them.
    No value is asserted there, only agreement.  A second rollout simulator takes the 60 steps in one call."""
    cfg, steps, seed = BY_ID[cid], 60, 0xB10C5
    with debug_knobs({"fused_step": 1}):
        one, roll, roll_once = make(cfg, N), make(cfg, N), make(cfg, N)
    with debug_knobs({"fused_step": 2}):
        two = make(cfg, N)
    assert (one.kernel_name, two.kernel_name) == ("mrl_hanabi_step_fused", "mrl_hanabi_step")
    assert roll.rollout_kernel_name == roll_once.rollout_kernel_name == "mrl_hanabi_rollout"
    ns = hanabi_spec.state_size(cfg)
    assert ns < 784
    finished = 0
    for t in range(steps):
        roll.rollout_random(1, seed=seed, first_step=t)
        a = roll.action_tensor().to_torch().clone()
        step(one, 1, a)
        step(two, 2, a)
        for other, name in ((two, "two launches"), (roll, "persistent rollout")):
            diff = (blocks(one) != blocks(other)).nonzero()
            assert diff.numel() == 0, f"step {t}, one launch vs {name}: first differing (world, agent, byte) {diff[0].tolist()}"
            same_tensors(one, other, f"at step {t} (one launch vs {name})")
        finished += int(one.reset_count_tensor().to_torch().item())
    roll_once.rollout_random(steps, seed=seed, first_step=0)
    diff = (blocks(one) != blocks(roll_once)).nonzero()
    assert diff.numel() == 0, f"{steps} steps in one rollout call: first differing (world, agent, byte) {diff[0].tolist()}"
    same_tensors(one, roll_once, "after one rollout call")
    assert finished > 0 and roll_once.rollout_kernel_name == "mrl_hanabi_rollout"
    no_timeout(one, two, roll, roll_once)
    for s in (one, two, roll, roll_once):
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# Against the reference's own sim.cpp (oracle/_ref)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,heal", [("k5r3i8l3", 0), ("k2r4i1l1", 0), ("k4r5i5l2", 0), ("k3r3i4l2", 0), ("k5r3i8l3", 3), ("k2r4i1l1", 3)],
                         ids=["k5r3i8l3", "k2r4i1l1", "k4r5i5l2", "k3r3i4l2", "k5r3i8l3_late_workgroups", "k2r4i1l1_late_workgroups"])
def test_step_vs_compiled_reference(cid, heal, hip_lib):
    """As test_gpu_hanabi.py:test_step_vs_compiled_reference: the single-launch step, moves from the five policies read off
    the device's own records, also with workgroups that arrive late (`fused_heal_test`)."""
    from oracle import ref
    ref.require()
    cfg, steps = BY_ID[cid], 100
    with debug_knobs({"fused_step": 1, "fused_heal_test": heal}):
        sim = make(cfg, N)
    assert sim.kernel_name == "mrl_hanabi_step_fused"
    r = ref.RefHanabi(cfg, N)
    compare_ref(sim, r, "initial", cfg)
    rng = np.random.default_rng(N + heal)
    finished = 0
    for t in range(steps):
        a = choose(rng, cfg, r.mask, sim.game_tensor().to_torch().cpu().numpy())
        r.step(a)
        step(sim, 1, device_actions(a, N))
        compare_ref(sim, r, f"step {t}", cfg)
        assert int(sim.reset_count_tensor().to_torch().item()) == int(r.done.sum())
        finished += int(r.done.sum())
    assert finished > 0 and r.episodes == N + finished
    no_timeout(sim)
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# One launch == two launches, in the short games
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heal", [0, 2], ids=["on_time", "late_workgroups"])
@pytest.mark.parametrize("cid", ["k5r2i8l3", "k3r2i1l1"])
def test_single_launch_step_equals_two_phase(cid, heal, hip_lib):
    """Two ranks: a game is a few moves, a large share of the worlds finishes in every step, and a workgroup that recounts a
    late one (`fused_heal_test`) has the most to recount."""
    cfg, n, steps = BY_ID[cid], 1500, 60
    with debug_knobs({"fused_step": 1, "fused_heal_test": heal}):
        s1 = make(cfg, n)
    with debug_knobs({"fused_step": 2}):
        s2 = make(cfg, n)
    assert s1.kernel_name == "mrl_hanabi_step_fused" and s2.kernel_name == "mrl_hanabi_step"
    gen = torch.Generator(device="cuda").manual_seed(11)
    mask = s1.action_mask_tensor().to_torch()
    total = 0
    for t in range(steps):
        a = (torch.rand(mask.shape, device="cuda", generator=gen) * mask).argmax(-1, keepdim=True).to(torch.int32)
        step(s1, 1, a)
        step(s2, 2, a)
        same_tensors(s1, s2, f"at step {t}")
        total += int(s1.reset_count_tensor().to_torch().item())
    assert total > n  # on average every world ended more than once
    no_timeout(s1, s2)
    s1.close()
    s2.close()


# ---------------------------------------------------------------------------------------------------------------------
# The persistent rollout
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4096, 1000 + 37], ids=["4096", "ragged"])
@pytest.mark.parametrize("cid", ["k5r4i8l3", "k2r3i3l1", "k4r5i5l2"])
def test_persistent_rollout_equals_stepwise(cid, n, hip_lib):
    """mrl_rollout_random with the records in LDS for all steps of a call, against a simulator that is forced to one launch
    per step and is called once per step."""
    cfg = BY_ID[cid]
    one = make(cfg, n)
    with debug_knobs({"hanabi.no_persistent": 1}):
        many = make(cfg, n)
    assert one.rollout_kernel_name == "mrl_hanabi_rollout" and many.rollout_kernel_name == many.kernel_name
    at = finished = 0
    for chunk in (1, 2, 7, 40, 1, 64):
        one.rollout_random(chunk, seed=2024, first_step=at)
        for k in range(chunk):
            many.rollout_random(1, seed=2024, first_step=at + k)
            finished += int(many.reset_count_tensor().to_torch().item())
        at += chunk
        same_tensors(one, many, f"after {at} steps", NAMES + ["action_tensor"])
        assert torch.equal(blocks(one), blocks(many)), f"whole blocks differ after {at} steps"
    mask = one.action_mask_tensor().to_torch()
    a = (torch.rand(mask.shape, device="cuda") * mask).argmax(-1, keepdim=True).to(torch.int32)
    for sim in (one, many):  # an ordinary step continues from either
        sim.step_with_actions(a)
    same_tensors(one, many, "after a step on top")
    assert finished > 0
    assert one.rollout_kernel_name == "mrl_hanabi_rollout", "the runtime refused the cooperative launch: these were launches per step"
    no_timeout(one, many)
    one.close()
    many.close()


@pytest.mark.parametrize("cid", ["k5r3i8l3", "k3r5i8l3"])
def test_device_random_policy(cid, hip_lib, oracle_lib):
    """The persistent rollout one step at a time == the oracle fed the documented stream (uniform over the mover's legal moves),
    then 90 steps in one call against that replay."""
    from madrona_rl_envs_playground_amd.simulators import random_hanabi_action
    cfg, seed, steps = BY_ID[cid], 0xC0FFEE1234, 90
    moves = hanabi_spec.num_moves(cfg)
    sim, twin = make(cfg, N), make(cfg, N)
    assert sim.rollout_kernel_name == twin.rollout_kernel_name == "mrl_hanabi_rollout"
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=8)
    world = np.arange(N)
    hist = np.zeros(20, np.int64)
    for t in range(steps):
        mover = (orc.active[1] != 0).astype(np.int64)
        legal = orc.mask[mover, world]
        want = random_hanabi_action(seed, 500 + t, world, mover, legal)
        assert (legal[world, want] != 0).all()
        sim.rollout_random(1, seed=seed, first_step=500 + t)
        got = sim.action_tensor().to_torch().cpu().numpy()[mover, world, 0]
        assert np.array_equal(got, want), f"drawn actions differ at step {t}"
        acts = np.zeros((2, N), np.int32)
        acts[mover, world] = want
        orc.step(acts)
        compare(sim, orc, f"step {t}", cfg)
        hist += np.bincount(want, minlength=20)
    assert (hist[:moves] > 0).all() and not hist[moves:].any(), f"moves drawn: {hist.tolist()}"
    twin.rollout_random(steps, seed=seed, first_step=500)
    compare(twin, orc, f"{steps} steps in one call", cfg)
    assert torch.equal(blocks(twin), blocks(sim))
    assert sim.rollout_kernel_name == twin.rollout_kernel_name == "mrl_hanabi_rollout"
    no_timeout(sim, twin)
    sim.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------------
# reset_worlds
# ---------------------------------------------------------------------------------------------------------------------
class Patchwork:
    """The oracle of a batch whose worlds restart out of step.  The oracle restarts a world only when its game ends, and numbers
    the new episodes in its own batch; so every set of worlds that restarts together -- by reset_worlds or by finishing in
    the same step -- goes on in a NEW oracle of that many worlds whose first episode is the batch's counter, which is what
    the library documents (ascending world order, numbered from the counter).  A world is followed in the last oracle that
    took it; slots nobody follows any more play on with moves of their own."""

    def __init__(self, oracle_lib, cfg, n):
        self.new = lambda m, first: oracle_lib.HanabiOracle(cfg, m, num_threads=4, first_episode=first)
        self.n, self.counter = n, n
        self.parts = [self.new(n, 0)]
        self.part, self.slot = np.zeros(n, np.int64), np.arange(n)
        self.reward, self.done = np.zeros((2, n), np.float32), np.zeros(n, np.int32)

    def _owned(self):
        for k, p in enumerate(self.parts):
            own = np.nonzero(self.part == k)[0]
            if p is not None and not len(own):
                p.close()
                self.parts[k] = p = None
            if p is not None:
                yield p, own, self.slot[own]

    def _gather(self, get, axis):
        out = None
        for p, own, slot in self._owned():
            v = get(p)
            if out is None:
                out = np.zeros(v.shape[:axis] + (self.n,) + v.shape[axis + 1:], v.dtype)
            out[(slice(None),) * axis + (own,)] = v[(slice(None),) * axis + (slot,)]
        return out

    obs = property(lambda self: self._gather(lambda p: p.obs, 1))
    state = property(lambda self: self._gather(lambda p: p.state, 1))
    mask = property(lambda self: self._gather(lambda p: p.mask, 1))
    active = property(lambda self: self._gather(lambda p: p.active, 1))

    def dump(self):
        return self._gather(lambda p: p.dump(), 0)

    def restart(self, worlds):
        """`worlds` (ascending) start the episodes counter, counter + 1, ..."""
        self.parts.append(self.new(len(worlds), self.counter))
        self.counter += len(worlds)
        self.part[worlds], self.slot[worlds] = len(self.parts) - 1, np.arange(len(worlds))

    def step(self, rng, acts):
        for p, own, slot in list(self._owned()):
            a = legal_random(rng, p.mask)
            a[:, slot] = acts[:, own]
            p.step(a)
            self.reward[:, own], self.done[own] = p.reward[:, slot], p.done[slot]
        ended = np.nonzero(self.done)[0]
        if len(ended):
            self.restart(ended)


@pytest.mark.parametrize("fused", [1, 2], ids=["one_launch", "two_launches"])
def test_reset_worlds_between_steps(fused, hip_lib, oracle_lib):
    """reset_worlds with a random mask every fourth step, all tensors against the oracle after every step and after every
    reset: the restarted worlds are the episodes counter, counter + 1, ... in ascending world order, the others and the
    per-step outputs (reward, done) stay, and the episodes that end in later steps are numbered after them."""
    cfg, steps = BY_ID["k4r4i7l2"], 40
    with debug_knobs({"fused_step": fused}):
        sim = make(cfg, N)
    pw = Patchwork(oracle_lib, cfg, N)
    compare(sim, pw, "initial", cfg)
    rng = np.random.default_rng(44)
    restarted = finished = 0
    for t in range(steps):
        acts = choose(rng, cfg, pw.mask, pw.dump())
        pw.step(rng, acts)
        sim.step_with_actions(device_actions(acts, N).contiguous())
        compare(sim, pw, f"step {t}", cfg)
        assert int(sim.reset_count_tensor().to_torch().item()) == int(pw.done.sum())
        finished += int(pw.done.sum())
        if t % 4 == 1:
            pick = rng.random(N) < (0.3 if t % 8 == 1 else 0.02)
            sim.reset_worlds(torch.from_numpy(pick))
            pw.restart(np.nonzero(pick)[0])
            compare(sim, pw, f"reset after step {t}", cfg)
            restarted += int(pick.sum())
    assert finished > 0 and restarted > N and pw.counter == N + finished + restarted
    no_timeout(sim)
    sim.close()


# ---------------------------------------------------------------------------------------------------------------------
# Graph capture
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [1, 2], ids=["one_launch", "two_launches"])
def test_steps_captured_in_a_hip_graph_after_prepare(fused, hip_lib):
    """After mrl_prepare_graph_capture three steps are captured (a linear chain of launches, moves drawn by the step kernel from
    a fixed stream) and replayed twice with an eager step in between: the same tensors as the same calls one by one."""
    cfg = BY_ID["k5r3i8l3"]
    with debug_knobs({"fused_step": fused, "hanabi.no_persistent": 1}):
        eager, graphed = make(cfg, N), make(cfg, N)
    graphed.prepare_graph_capture()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            graphed.rollout_random(3, seed=21, first_step=100)
    torch.cuda.current_stream().wait_stream(side)
    names = NAMES + ["action_tensor"]
    same_tensors(eager, graphed, "after the capture (nothing ran)", names)
    for rep in range(2):
        graph.replay()
        eager.rollout_random(3, seed=21, first_step=100)
        same_tensors(eager, graphed, f"after replay {rep}", names)
        graphed.rollout_random(1, seed=5, first_step=rep)
        eager.rollout_random(1, seed=5, first_step=rep)
        same_tensors(eager, graphed, f"after the eager step that follows replay {rep}", names)
    assert torch.equal(blocks(eager), blocks(graphed))
    assert int(eager.game_tensor().to_torch()[:, 88].ne(0xFF).sum()) > 0  # games are under way
    no_timeout(eager, graphed)
    eager.close()
    graphed.close()


# ---------------------------------------------------------------------------------------------------------------------
# The wrapper, and what the library refuses
# ---------------------------------------------------------------------------------------------------------------------
def test_env_wrapper_sizes_its_spaces_from_the_configuration(hip_lib, oracle_lib):
    from madrona_rl_envs_playground_amd.envs import HanabiMadrona
    cfg, n = dict(BY_ID["k3r3i4l2"], observation_type=1), 300
    no, ns, moves = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg), hanabi_spec.num_moves(cfg)
    # hands 45 + 2, deck 8, fireworks 9, tokens 4 + 2, discards 18, last action 35, knowledge 150; then the own hand's 45
    assert (no, ns, moves) == (273, 318, 5 + 5 + 3 + 3)
    env = HanabiMadrona(n, 0, config=cfg)
    assert env.observation_space.shape == (no,) and env.share_observation_space.shape == (ns,) and env.action_space.n == moves
    orc = oracle_lib.HanabiOracle(cfg, n)
    obs = env.n_reset()
    for agent in range(2):
        assert obs[agent].obs.shape == (n, no) and obs[agent].state.shape == (n, ns) and obs[agent].action_mask.shape == (n, moves)
        assert np.array_equal(obs[agent].obs.cpu().numpy().astype(np.uint8), orc.obs[agent, :, :no])
        assert np.array_equal(obs[agent].state.cpu().numpy().astype(np.uint8), orc.state[agent, :, :ns])
        assert np.array_equal(obs[agent].action_mask.cpu().numpy(), orc.mask[agent, :, :moves] != 0)
        assert np.array_equal(obs[agent].active.cpu().numpy(), orc.active[agent] != 0)
    assert not orc.mask[..., moves:].any()
    env.close()


def test_refusals_and_boundaries(hip_lib):
    good = BY_ID["k3r3i4l2"]
    for field, low, high in (("colors", 0, 6), ("ranks", 1, 6), ("max_information_tokens", 0, 9), ("max_life_tokens", 0, 4)):
        for v in (low, high):
            with pytest.raises(MrlError, match="need 1..5 colors, 2..5 ranks, 1..8 information tokens, 1..3 life tokens"):
                make(dict(good, **{field: v}), 8)
    for k, r in hanabi_configs.DECKLESS:
        with pytest.raises(MrlError, match="does not leave a deck after dealing two hands"):
            make(config(k, r, 3, 1), 8)
    for (k, r), deck in (((1, 5), 0), ((2, 3), 2), ((3, 2), 2), ((5, 5), 40)):
        cfg = config(k, r, 8, 3)
        sim = make(cfg, 8)
        rec = sim.game_tensor().to_torch().cpu().numpy()
        assert hanabi_configs.deck_size(cfg) == deck and (rec[:, 50] == deck).all()
        assert sim.observation_tensor().to_torch().shape == (2, 8, hanabi_spec.observation_size(cfg))
        sim.close()
