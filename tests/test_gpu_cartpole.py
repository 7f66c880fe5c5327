"""GPU parity of the Cartpole HIP step against the CPU oracle.

Float state: the bar is 1e-5 on identical action sequences (BASELINE.json
north_star); the reference's own check is one step at 1e-6
(envs/cartpole_env.py:246-288).  Tests are one-step differential like the
reference's (a 1-ulp sinf/cosf difference at a threshold flips `done`), with the
GPU state re-synchronised from the oracle after each compared step.  Reset
states come from integer RNG + exact float ops and must match bit for bit.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd.simulators import CartpoleSimulator, ExecMode  # noqa: E402

TOL = 1e-5


def make(n):
    return CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)


def test_initial_state_and_shapes(hip_lib, oracle_lib):
    n = 1024
    sim, orc = make(n), oracle_lib.CartpoleOracle(n)
    st = sim.observation_tensor().to_torch()
    assert st.shape == (n, 4) and st.dtype == torch.float32
    assert sim.action_tensor().to_torch().shape == (n, 1) and sim.action_tensor().to_torch().dtype == torch.int32
    assert sim.reward_tensor().to_torch().shape == (n, 1) and sim.reset_tensor().to_torch().shape == (n, 1)
    assert np.array_equal(st.cpu().numpy().view(np.uint32), orc.state.view(np.uint32)), "initial state not bit-equal"
    assert torch.equal(sim.world_id_tensor().to_torch()[:, 0].cpu(), torch.arange(n, dtype=torch.int32))
    assert (np.abs(orc.state) <= 0.05).all()
    sim.close()


@pytest.mark.parametrize("n,steps", [(1024, 1000), (100000, 60)])
def test_lockstep_vs_oracle(n, steps, hip_lib, oracle_lib):
    """configs[0] of BASELINE.json (1024 worlds, random actions, seed 0) and a larger batch."""
    torch.manual_seed(0)
    sim, orc = make(n), oracle_lib.CartpoleOracle(n, num_threads=8)
    st = sim.observation_tensor().to_torch()
    act = sim.action_tensor().to_torch()
    worst, flips, resets = 0.0, 0, 0
    for t in range(steps):
        a = torch.randint(0, 2, (n, 1), dtype=torch.int32)
        before = orc.state.copy()
        orc.step(a.numpy())
        act.copy_(a.cuda())
        sim.step()
        got = st.cpu().numpy()
        done_gpu = sim.reset_tensor().to_torch().cpu().numpy()[:, 0]
        done_cpu = orc.done[:, 0]
        agree = done_gpu == done_cpu
        flips += int((~agree).sum())
        keep = agree & (done_cpu == 0)
        if keep.any():
            worst = max(worst, float(np.abs(got[keep] - orc.state[keep]).max()))
        # worlds that reset on both sides must hold the same fresh state, bit for bit,
        # as long as no earlier world disagreed about resetting in this step
        if agree.all() and done_cpu.any():
            r = done_cpu == 1
            resets += int(r.sum())
            assert np.array_equal(got[r].view(np.uint32), orc.state[r].view(np.uint32)), f"reset state, step {t}"
            assert int(sim.reset_count_tensor().to_torch().item()) == int(r.sum())
        assert (sim.reward_tensor().to_torch() == 1).all()
        # a flipped done means one side re-seeded: re-synchronise everything from the oracle
        st.copy_(torch.from_numpy(orc.state).cuda())
        if not agree.all():
            sim.set_episode_counter(orc.episodes)
        del before
    assert worst <= TOL, f"max |gpu - oracle| over non-terminal steps = {worst}"
    assert flips <= max(2, n * steps // 200000), f"{flips} done flags disagree"
    assert resets > 0


VARIANTS = {1: "reference_typed", 2: "lean_f64", 3: "lean_f64_bounded_sincos", 4: "float"}


@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=[VARIANTS[v] for v in sorted(VARIANTS)])
def test_arithmetic_variants(variant, hip_lib, oracle_lib):
    """csrc/cartpole.hip evaluates the transition in one of four ways (mrl_debug_set cartpole.variant; 3 is the default).
    Each must hold the reference's own one-step bound, 1e-6 against its float64 numpy twin (envs/cartpole_env.py:277), on
    the reference-generated transitions, termination flags included (outside the band where a last-place difference
    decides), and 1e-5 against the oracle in lock-step with bit-equal fresh states."""
    import os
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cartpole_transitions.npz"))
    states, actions, next64, done = z["states"], z["actions"], z["next64"], z["done"]
    m = len(states)
    with debug_knobs({"cartpole.variant": variant}):
        g, sim = make(m), make(50000)
    g.observation_tensor().to_torch().copy_(torch.from_numpy(states).cuda())
    g.action_tensor().to_torch().copy_(torch.from_numpy(actions).cuda().view(m, 1))
    g.step_phase1(None)
    got = g.observation_tensor().to_torch().cpu().numpy().astype(np.float64)
    got_done = g.reset_tensor().to_torch().cpu().numpy()[:, 0]
    near = (np.abs(np.abs(next64[:, 0]) - 2.4) < 1e-5) | (np.abs(np.abs(next64[:, 2]) - 12 * 2 * np.pi / 360) < 1e-5)
    assert ((got_done == done) | near).all()
    assert np.abs(got - next64).max() < 1e-6, np.abs(got - next64).max()
    g.close()
    n = 50000
    orc = oracle_lib.CartpoleOracle(n, num_threads=8)
    st, act = sim.observation_tensor().to_torch(), sim.action_tensor().to_torch()
    torch.manual_seed(variant)
    worst, flips = 0.0, 0
    for t in range(60):
        a = torch.randint(0, 2, (n, 1), dtype=torch.int32)
        orc.step(a.numpy())
        act.copy_(a.cuda())
        sim.step()
        got = st.cpu().numpy()
        done_gpu, done_cpu = sim.reset_tensor().to_torch().cpu().numpy()[:, 0], orc.done[:, 0]
        agree = done_gpu == done_cpu
        flips += int((~agree).sum())
        keep = agree & (done_cpu == 0)
        worst = max(worst, float(np.abs(got[keep] - orc.state[keep]).max()))
        if agree.all() and done_cpu.any():
            r = done_cpu == 1
            assert np.array_equal(got[r].view(np.uint32), orc.state[r].view(np.uint32)), f"reset state, step {t}"
        st.copy_(torch.from_numpy(orc.state).cuda())
        if not agree.all():
            sim.set_episode_counter(orc.episodes)
    assert worst <= (1e-6 if variant != 4 else TOL), f"max |gpu - oracle| = {worst}"
    assert flips <= 15, f"{flips} done flags disagree"
    sim.close()


def test_unknown_arithmetic_variant_is_refused(hip_lib):
    from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs
    with debug_knobs({"cartpole.variant": 9}):
        with pytest.raises(MrlError, match="cartpole.variant"):
            make(64)


@pytest.mark.parametrize("n,pattern,fused_step", [
    pytest.param(300001, "all", 0, id="300001-all"),
    pytest.param(300001, "dense_block", 0, id="300001-dense_block"),
    pytest.param(1 << 20, "sparse", 0, id="1048576-sparse"),
    pytest.param(777, "all", 0, id="777-all"),
    pytest.param(777, "all", 2, id="777-all-two_launches"),
    pytest.param(300001, "all", 2, id="300001-all-two_launches"),
    pytest.param(300001, "dense_block", 2, id="300001-dense_block-two_launches"),
    pytest.param(4194305, "sparse", 0, id="4194305-sparse"),
])
def test_planted_terminations_take_episodes_in_world_order(n, pattern, fused_step, hip_lib, oracle_lib):
    """Finished worlds take consecutive episodes in ascending world order, whichever kernel re-seeds them: plant every
    world, one workgroup's whole chunk plus a sprinkle, and a sparse 3 %.

    fused_step = 0 is the library's choice: up to 4096 workgroups of 1024 worlds the single launch, which re-seeds the
    finished worlds of a wave from a list in LDS.  fused_step = 2 asks for the two-launch pair, whose second launch
    (mrl::reseed_finished, csrc/episode_scan.hpp) compacts a workgroup's finished worlds from the step's ballot words,
    64 words per trip.  4194305 worlds is the smallest batch without a single launch (4097 workgroups) and the smallest
    whose chunk per workgroup of the two-launch grid -- 17 * 256 worlds = 68 mask words -- needs a second trip."""
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    rng = np.random.default_rng(5)
    with debug_knobs({"fused_step": fused_step}):
        sim = make(n)
    if fused_step == 2 or n == 4194305:
        assert sim.kernel_name == "mrl_cartpole_step"
    orc = oracle_lib.CartpoleOracle(n, num_threads=8)
    st = sim.observation_tensor().to_torch()
    planted = orc.state.copy()
    if pattern == "all":
        hit = np.ones(n, bool)
    elif pattern == "dense_block":  # one workgroup's whole chunk, plus a sprinkle elsewhere
        hit = rng.random(n) < 0.01
        hit[1024:1600] = True
    else:
        hit = rng.random(n) < 0.03
    planted[hit, 0] = np.where(rng.random(int(hit.sum())) < 0.5, 3.0, -3.0)  # beyond X_THRESHOLD: done whatever the action
    orc.state[:] = planted
    st.copy_(torch.from_numpy(planted).cuda())
    for t in range(3):  # the re-seeded worlds keep going; later steps use the short-list path again
        a = torch.randint(0, 2, (n, 1), dtype=torch.int32)
        orc.step(a.numpy())
        sim.action_tensor().to_torch().copy_(a.cuda())
        sim.step()
        done_gpu = sim.reset_tensor().to_torch().cpu().numpy()[:, 0]
        assert np.array_equal(done_gpu, orc.done[:, 0]), f"done flags, step {t}"
        r = orc.done[:, 0] == 1
        got = st.cpu().numpy()
        assert np.array_equal(got[r].view(np.uint32), orc.state[r].view(np.uint32)), f"fresh states, step {t}"
        assert int(sim.reset_count_tensor().to_torch().item()) == int(r.sum())
        if t == 0:
            assert np.array_equal(r, hit) or pattern != "all"
        st.copy_(torch.from_numpy(orc.state).cuda())
    sim.close()


@pytest.mark.parametrize("n,steps,heal", [(5000, 120, 0), (300001, 60, 0), (1 << 20, 25, 0), (300001, 40, 3), (70000, 60, 1)],
                         ids=["5000", "300001", "1M", "300001_late_workgroups", "70000_all_late"])
def test_two_phase_equals_single_call(n, steps, heal, hip_lib):
    """mrl_step as ONE launch (every workgroup publishes its finished count, one wave looks back at the lower ones, a count
    that does not appear is recounted from that workgroup's inputs: csrc/episode_scan.hpp); the two-phase calls are two
    launches with the prefix between them.  Same numbers either way -- also when workgroups arrive late
    (`fused_heal_test` = m: workgroups whose index is a multiple of m do nothing until a higher one has recounted
    them, so the recount path runs against inputs nobody has touched yet)."""
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    with debug_knobs({"fused_step": 1, "fused_heal_test": heal}):
        s1 = make(n)
    with debug_knobs({"fused_step": 2}):
        s2 = make(n)
    assert s1.kernel_name == "mrl_cartpole_step_fused" and s2.kernel_name == "mrl_cartpole_step"
    torch.manual_seed(1)
    for _ in range(steps):
        a = torch.randint(0, 2, (n, 1), dtype=torch.int32, device="cuda")
        s1.action_tensor().to_torch().copy_(a)
        s1.step()
        s2.step_phase1(a)
        s2.step_phase2(None)
        assert torch.equal(s1.observation_tensor().to_torch(), s2.observation_tensor().to_torch())
        assert torch.equal(s1.reset_tensor().to_torch(), s2.reset_tensor().to_torch())
        assert torch.equal(s1.reset_count_tensor().to_torch(), s2.reset_count_tensor().to_torch())
    assert int(s1.scan_timeout_tensor().to_torch().item()) == 0
    s1.close()
    s2.close()


def test_sharded_episode_numbering(hip_lib):
    """Two shards driven through the two-phase step with exchanged reset counts
    reproduce one simulator of the whole batch exactly (same episode -> same seed)."""
    n, half = 6000, 3000
    whole, lo, hi = make(n), make(half), make(half)
    lo.reseed_shard(0, n)
    hi.reseed_shard(half, n)
    counter = torch.tensor([n], dtype=torch.int32, device="cuda")
    torch.manual_seed(2)
    for _ in range(150):
        a = torch.randint(0, 2, (n, 1), dtype=torch.int32, device="cuda")
        whole.action_tensor().to_torch().copy_(a)
        whole.step()
        lo.step_phase1(a[:half].contiguous())
        hi.step_phase1(a[half:].contiguous())
        # phase 1 leaves per-shard done flags; counts of the lower shard offset the upper one
        c_lo = lo.reset_tensor().to_torch().sum().to(torch.int32).reshape(1)
        c_hi = hi.reset_tensor().to_torch().sum().to(torch.int32).reshape(1)
        lo.step_phase2(counter)
        hi.step_phase2(counter + c_lo)
        counter = counter + c_lo + c_hi
        both = torch.cat([lo.observation_tensor().to_torch(), hi.observation_tensor().to_torch()])
        assert torch.equal(both, whole.observation_tensor().to_torch())
    for s in (whole, lo, hi):
        s.close()


@pytest.mark.parametrize("n,steps", [(70001, 150), (1 << 20, 40)])
def test_device_random_policy(n, steps, hip_lib):
    """mrl_rollout_random == stepping with the documented action stream (the hash's top bit); one
    persistent launch for many steps == many launches of one step."""
    from madrona_rl_envs_playground_amd.simulators import random_cartpole_action
    seed = 77
    a, b = make(n), make(n)
    world = np.arange(n)
    seen = np.zeros(2, np.int64)
    for t in range(steps):
        want = random_cartpole_action(seed, 9 + t, world)
        a.rollout_random(1, seed=seed, first_step=9 + t)
        assert np.array_equal(a.action_tensor().to_torch().cpu().numpy()[:, 0], want)
        b.action_tensor().to_torch().copy_(torch.from_numpy(want).cuda().view(n, 1))
        b.step()
        assert torch.equal(a.observation_tensor().to_torch(), b.observation_tensor().to_torch())
        assert torch.equal(a.reset_tensor().to_torch(), b.reset_tensor().to_torch())
        seen += np.bincount(want, minlength=2)
    assert abs(seen[0] / seen.sum() - 0.5) < 0.01
    c = make(n)
    c.rollout_random(steps // 3, seed=seed, first_step=9)
    c.rollout_random(steps - steps // 3, seed=seed, first_step=9 + steps // 3)
    assert torch.equal(c.observation_tensor().to_torch(), a.observation_tensor().to_torch())
    assert torch.equal(c.reset_tensor().to_torch(), a.reset_tensor().to_torch())
    assert torch.equal(c.reset_count_tensor().to_torch(), a.reset_count_tensor().to_torch())
    c.step()  # the episode counter after a rollout continues like after single steps
    a.step()
    assert torch.equal(c.observation_tensor().to_torch(), a.observation_tensor().to_torch())
    assert c.rollout_kernel_name == "mrl_cartpole_rollout", "the runtime refused the cooperative launch: these were launches per step"
    for sim in (a, b, c):
        assert int(sim.scan_timeout_tensor().to_torch().item()) == 0
        sim.close()


def test_scan_timeout_is_an_error_not_a_silent_flag(hip_lib):
    """A bounded in-kernel wait that expires leaves episode numbers unspecified: the calls after it
    must fail (MRL_ERR_DEVICE -> MrlError) and close() must say so.  The alarm is raised by a test
    hook (mrl_debug_set inject_scan_timeout) through the same device->host word a kernel would use."""
    from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs
    ok = make(2048)
    ok.step()
    assert not ok.scan_timed_out and int(ok.scan_timeout_tensor().to_torch().item()) == 0
    with debug_knobs({"inject_scan_timeout": 1}):
        bad = make(2048)
    assert bad.scan_timed_out and int(bad.scan_timeout_tensor().to_torch().item()) == 1
    for call in (bad.step, lambda: bad.step_with_actions(torch.zeros((2048, 1), dtype=torch.int32, device="cuda")),
                 lambda: bad.rollout_random(3, seed=1), lambda: bad.step_phase1()):
        with pytest.raises(MrlError, match="SCAN_TIMEOUT"):
            call()
    with pytest.raises(MrlError, match="SCAN_TIMEOUT"):
        bad.close()
    ok.step()  # other simulators are unaffected
    ok.close()


@pytest.mark.parametrize("n,fused", [(3000, 1), (300001, 1), (300001, 2)], ids=["one_launch_3000", "one_launch_300001", "two_launches_300001"])
def test_steps_captured_in_a_hip_graph_after_prepare(n, fused, hip_lib):
    """mrl_prepare_graph_capture moves the launch-to-launch state (which half of the episode counter is current, the look-back's
    epoch) into device memory; every step then advances it with a one-thread launch of its own, so a captured sequence of an
    ODD number of steps replayed several times -- and eager steps in between -- equals the same steps issued one by one on an
    ordinary simulator."""
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    with debug_knobs({"fused_step": fused}):
        eager, graphed = make(n), make(n)
    graphed.prepare_graph_capture()
    gen = torch.Generator(device="cuda").manual_seed(n)
    acts = [torch.randint(0, 2, (n, 1), dtype=torch.int32, device="cuda", generator=gen) for _ in range(3)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for a in acts:
                graphed.step_with_actions(a)
    torch.cuda.current_stream().wait_stream(side)
    finished = 0
    for rep in range(40):
        graph.replay()
        for a in acts:
            eager.step_with_actions(a)
        if rep % 3 == 0:  # an eager step on the prepared simulator between two replays
            graphed.step_with_actions(acts[1])
            eager.step_with_actions(acts[1])
        for name in ("observation_tensor", "reset_tensor", "reward_tensor", "reset_count_tensor"):
            assert torch.equal(getattr(eager, name)().to_torch(), getattr(graphed, name)().to_torch()), f"{name} differs after replay {rep}"
        finished += int(eager.reset_count_tensor().to_torch().item())
    assert finished > 0
    # the device-side policy on a prepared simulator: one launch per step, same stream of draws
    graphed.rollout_random(7, seed=3, first_step=0)
    eager.rollout_random(7, seed=3, first_step=0)
    assert torch.equal(eager.observation_tensor().to_torch(), graphed.observation_tensor().to_torch())
    eager.close()
    graphed.close()


def test_step_refuses_graph_capture(hip_lib):
    """Cartpole / Hanabi / balance launches carry host-side counter state in their arguments: a replayed
    capture would run with stale values, so -- until mrl_prepare_graph_capture has been called -- the entry points refuse a
    capturing stream (MRL_ERR_INVALID)."""
    from madrona_rl_envs_playground_amd._lib import MrlError
    sim = make(2048)
    a = torch.zeros((2048, 1), dtype=torch.int32, device="cuda")
    sim.step_with_actions(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    refused = 0
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for call in (sim.step, lambda: sim.step_with_actions(a), lambda: sim.step_phase1(a), sim.step_phase2,
                         lambda: sim.rollout_random(2, seed=3)):
                try:
                    call()
                except MrlError as e:
                    assert "captured" in str(e)
                    refused += 1
            a.add_(0)  # the capture itself stays valid: something was recorded
    assert refused == 5
    sim.step_with_actions(a)  # and the simulator is still usable outside the capture
    torch.cuda.synchronize()
    assert int(sim.scan_timeout_tensor().to_torch().item()) == 0
    sim.close()


def test_action_arrays_are_validated_on_every_entry_point(hip_lib):
    sim = make(512)
    good = torch.zeros((512, 1), dtype=torch.int32, device="cuda")
    for bad in (good.long(), good.cpu(), good[:100], torch.zeros((512, 2), dtype=torch.int32, device="cuda")[:, :1]):
        for call in (sim.step_with_actions, sim.step_phase1):
            with pytest.raises(ValueError):
                call(bad)
    sim.step_phase1(good)
    sim.step_phase2()
    sim.close()


def test_current_device_is_restored(hip_lib):
    """C-ABI calls bind the simulator's device and put the caller's back."""
    before = torch.cuda.current_device()
    sim = make(256)
    sim.step()
    assert torch.cuda.current_device() == before
    sim.close()


def _glibc_sincos():
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    for f in (libm.sinf, libm.cosf):
        f.restype, f.argtypes = ctypes.c_float, [ctypes.c_float]
    return libm.sinf, libm.cosf


@pytest.mark.parametrize("n,steps", [(1024, 300), (300001, 30), (1 << 20, 15)], ids=["1024", "300001", "1M"])
@pytest.mark.parametrize("variant", [1, 0], ids=["reference_typed", "default"])
def test_step_vs_compiled_reference(variant, n, steps, hip_lib):
    """One launch and two launches against the reference's own sim.cpp compiled unchanged against the Madrona stand-in
    (oracle/_ref: g++ -ffp-contract=off, glibc sinf / cosf), one step at a time from a common state (re-synchronised from
    the reference after every step, as test_lockstep_vs_oracle does from the oracle).

    Measured on the MI355X (300001 worlds x 30 steps): with the reference's typing (cartpole.variant=1) 0.80 % of the
    world-steps differ, and every one of them starts from a theta at which the device's sinf / cosf (ocml) and glibc's
    differ -- 2.8 % of the visited thetas; the default arithmetic differs in 8.55 % of the world-steps.  Every difference
    stayed within 2.4e-7."""
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    from oracle import ref
    ref.require()
    sims = []
    for fused in (1, 2):
        with debug_knobs({"fused_step": fused, "cartpole.variant": variant}):
            sims.append(make(n))
    assert [s.kernel_name for s in sims] == ["mrl_cartpole_step_fused", "mrl_cartpole_step"]
    r = ref.RefCartpole(n)
    for s in sims:
        assert np.array_equal(s.observation_tensor().to_torch().cpu().numpy().view(np.uint32), r.state.view(np.uint32))
    sinf, cosf = _glibc_sincos()
    rng = np.random.default_rng(n + variant)
    compared = differing = resets = 0
    for t in range(steps):
        a = rng.integers(0, 2, n).astype(np.int32)
        theta = r.state[:, 2].copy()
        r.step(a)
        ref_state, ref_done = r.state, r.done[:, 0]
        for s in sims:
            st = s.observation_tensor().to_torch()
            s.action_tensor().to_torch().copy_(torch.from_numpy(a).cuda().view(n, 1))
            s.step()
            got = st.cpu().numpy()
            done = s.reset_tensor().to_torch().cpu().numpy()[:, 0]
            assert np.array_equal(done, ref_done), f"done flags, step {t}"  # none flipped in the measurement
            if ref_done.any():
                rs = ref_done == 1
                resets += int(rs.sum())
                assert np.array_equal(got[rs].view(np.uint32), ref_state[rs].view(np.uint32)), f"reset state, step {t}"
                assert int(s.reset_count_tensor().to_torch().item()) == int(rs.sum())
            live = ref_done == 0
            diff = live & (got.view(np.uint32) != ref_state.view(np.uint32)).any(1)
            compared += int(live.sum())
            differing += int(diff.sum())
            # the reference's own one-step bound, 1e-6 (envs/cartpole_env.py:277); in ulps: at most 4 at the scale of the
            # state's magnitude (max(|value|, 1): the largest difference seen is 2 ulps of 1.0)
            scale = np.spacing(np.maximum(np.abs(ref_state[live]), np.float32(1)))
            assert (np.abs(got[live] - ref_state[live]) <= 4 * scale).all(), f"more than 4 ulps, step {t}"
            if variant == 1 and diff.any():
                # typed as the reference writes it, the device rounds every operation as the CPU does: a difference can
                # only come from the math library.  sin / cos of the pre-step theta on the device (ocml, as the kernel's
                # sinf / cosf) against glibc's, world by world
                w = np.flatnonzero(diff)
                th = torch.from_numpy(theta[w]).cuda()
                dev_s, dev_c = torch.sin(th).cpu().numpy(), torch.cos(th).cpu().numpy()
                host_s = np.array([sinf(float(x)) for x in theta[w]], np.float32)
                host_c = np.array([cosf(float(x)) for x in theta[w]], np.float32)
                unexplained = (dev_s == host_s) & (dev_c == host_c)
                assert not unexplained.any(), f"step {t}: worlds {w[unexplained][:8].tolist()} differ with sinf and cosf equal"
            st.copy_(torch.from_numpy(ref_state).cuda())
    frac = differing / compared
    print(f"cartpole variant {variant}, {n} worlds: {differing} of {compared} world-steps differ ({frac:.3%}), {resets} resets")
    # ceilings above the measured 0.80 % / 8.55 %; ADVICE's "about 9 %" for the default arithmetic
    assert frac <= (0.015 if variant == 1 else 0.10), frac
    assert resets > 0
    for s in sims:
        s.close()
