"""The Hanabi step on moves that the legal-move mask forbids (tests/hanabi_illegal_cases.py): empty hints (A), discards at a
full pool (B), actions past the move table and negative ones (E) side by side with legal moves in every wave.  The contract
(include/mrl_envs.h, ACTION) is the reference's result for every move of the table, and for a value outside it the in-table
rank hint hanabi_illegal_cases.mapped_action names, at the partner (a departure from the reference, which hints the mover's
OWN hand when u / R is odd).  So every comparison is bit for bit against the CPU oracle fed the mapped action; the oracle
is pinned to the reference's own sim.cpp on the raw actions of these walks by test_ref_hanabi.py and the fixtures of
test_oracle_hanabi.py, and test_hanabi_illegal_api.py asserts on the CPU that the walks contain every class at least 100
times within the sizes used here and shows the departure for both parities of u / R.

300 worlds are one 256-world workgroup and a ragged second one; the healing recount needs three (700)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hanabi_configs  # noqa: E402
import hanabi_illegal_cases as ic  # noqa: E402
from madrona_rl_envs_playground_amd import hanabi_spec  # noqa: E402
from madrona_rl_envs_playground_amd._lib import MrlError, debug_knobs  # noqa: E402
from test_gpu_hanabi import make  # noqa: E402
from test_gpu_hanabi_configs import blocks, device_actions, no_timeout, same_tensors  # noqa: E402

N = ic.WORLDS


def compare(sim, orc, tag, cfg, worlds=slice(None)):
    """Both agents' observation, state and mask rows, active flags, reward, done and the whole 176-byte record of `worlds`."""
    no, ns = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg)
    cpu = lambda t: t.to_torch().cpu().numpy()
    assert sim.observation_tensor().to_torch().shape[-1] == no
    assert np.array_equal(cpu(sim.observation_tensor()).astype(np.uint8)[:, worlds, :no], orc.obs[:, worlds, :no]), f"obs {tag}"
    assert np.array_equal(cpu(sim.agent_state_tensor()).astype(np.uint8)[:, worlds, :ns], orc.state[:, worlds, :ns]), f"state {tag}"
    assert np.array_equal(cpu(sim.action_mask_tensor())[:, worlds], orc.mask[:, worlds]), f"mask {tag}"
    assert np.array_equal(cpu(sim.active_agent_tensor())[:, worlds], orc.active[:, worlds]), f"active {tag}"
    assert np.array_equal(cpu(sim.reward_tensor())[:, worlds], orc.reward[:, worlds]), f"reward {tag}"
    assert np.array_equal(cpu(sim.done_tensor())[worlds], orc.done[worlds]), f"done {tag}"
    diff = np.argwhere(cpu(sim.game_tensor())[worlds] != orc.dump()[worlds])
    assert not len(diff), f"game record {tag}: first differing (world, byte) {diff[0].tolist()}"


def issue(sim, how, a):
    """One step on actions `a` (2, n, 1) int32, by each way the library takes them."""
    if how == "action_tensor":
        sim.action_tensor().to_torch().copy_(a)
        sim.step()
    elif how == "step_with_actions":
        sim.step_with_actions(a.contiguous())
    elif how == "step_sequence":
        sim.step_sequence(a.contiguous().view(1, *a.shape))
    elif how == "two_phases":
        sim.step_phase1(a)
        sim.step_phase2(None)
    else:
        raise ValueError(how)


def lockstep(sim, orc, cfg, n, how, steps=ic.STEPS, recounted=None):
    """The walk on `orc`, every step issued to `sim` and compared; returns the class counts (of worlds `recounted` if given)."""
    compare(sim, orc, "initial", cfg)
    total, episodes = {}, n
    for t, rec, acts, cls in ic.walk(orc, cfg, steps):
        issue(sim, how, device_actions(acts, n))
        compare(sim, orc, f"step {t}", cfg)
        resets = int(sim.reset_count_tensor().to_torch().item())
        assert resets == int(orc.done.sum()), f"step {t}: RESET_COUNT"
        episodes += resets
        assert episodes == orc.episodes, f"step {t}: episode counter"
        pick = slice(None) if recounted is None else recounted
        for k, v in ic.count_classes(cfg, rec[pick], acts[:, pick], cls[pick], orc.done[pick]).items():
            total[k] = total.get(k, 0) + v
    no_timeout(sim)
    return total


# (configuration, code variant): every transition copy -- 2 the full game on registers (move_world_full in both step kernels,
# apply_action_full in the recount), 1 five ranks, 0 any configuration -- on the full game, and the variants the library
# picks itself elsewhere, with token pools at both ends and games without a deck
VARIANTS = [("full", 2), ("full", 1), ("full", 0), ("k4r5i5l2", 1), ("k4r5i5l2", 0), ("small", 1), ("very_small", 1),
            ("k5r3i8l3", 0), ("k2r4i1l1", 0), ("k1r5i1l1", 0)]


@pytest.mark.parametrize("fused", [1, 2], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("name,variant", VARIANTS, ids=[f"{n}_v{v}" for n, v in VARIANTS])
def test_lockstep_vs_oracle(name, variant, fused, hip_lib, oracle_lib):
    cfg = ic.config_of(name)
    assert variant <= hanabi_configs.variant(cfg)
    with debug_knobs({"fused_step": fused, "hanabi.variant": variant}):
        sim = make(cfg, N)
    assert sim.kernel_name == ("mrl_hanabi_step_fused" if fused == 1 else "mrl_hanabi_step")
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    total = lockstep(sim, orc, cfg, N, "action_tensor" if fused == 1 else "two_phases")
    print(f"hanabi {name} variant {variant}, {'one launch' if fused == 1 else 'two launches'}: {total}")
    assert min(total[k] for k in "ABE") >= 100 and total["E at the mover's own hand"] >= 1 and total["E at the partner"] >= 1
    assert total["episodes ended"] >= 1
    sim.close()


@pytest.mark.parametrize("how", ["step_with_actions", "step_sequence"])
@pytest.mark.parametrize("name", ["full", "k2r4i1l1"])
def test_every_way_actions_arrive(name, how, hip_lib, oracle_lib):
    """step() on the ACTION tensor and the two phases are test_lockstep_vs_oracle's; here the caller's own int32 array, one
    step per call and through mrl_step_sequence."""
    cfg = ic.config_of(name)
    sim = make(cfg, N)
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    total = lockstep(sim, orc, cfg, N, how)
    print(f"hanabi {name}, {how}: {total}")
    assert min(total[k] for k in "ABE") >= 100
    sim.close()


def test_step_sequence_of_many_steps_and_int64_actions(hip_lib, oracle_lib):
    """Sixteen steps per mrl_step_sequence call (the walk's actions, worked out on the oracle first), compared after each
    call.  And int64: a Hanabi simulator refuses mrl_step_with_actions_i64 (include/mrl_envs.h) and changes nothing; what a
    caller's `.to(torch.int32)` makes of an int64 -- its low 32 bits -- is then the action, negatives included."""
    cfg, chunk = ic.FULL, 16
    sim = make(cfg, N)
    orc, twin = oracle_lib.HanabiOracle(cfg, N, num_threads=4), oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    stream = [acts for _, _, acts, _ in ic.walk(orc, cfg)]
    for at in range(0, ic.STEPS, chunk):
        sim.step_sequence(torch.stack([device_actions(a, N) for a in stream[at:at + chunk]]).contiguous())
        for a in stream[at:at + chunk]:
            twin.step(ic.mapped_action(cfg, a))
        compare(sim, twin, f"after {at + chunk} steps", cfg)
    assert twin.episodes == orc.episodes > N
    rec = twin.dump()
    acts, cls = ic.choose_with_illegal(np.random.default_rng(3), cfg, twin.mask, rec)
    assert (acts < 0).any() and (cls == ic.E).any()
    wide = torch.from_numpy(acts.astype(np.int64)).cuda().view(2, N, 1)
    wide = torch.where(wide >= 0, wide + (1 << 32) * 7, wide)  # high words that narrowing drops; the negatives stay sign-extended
    with pytest.raises(MrlError, match="mrl_step_with_actions_i64: not available"):
        sim.step_with_actions_i64(wide.contiguous())
    compare(sim, twin, "after the refused int64 step", cfg)
    narrowed = wide.to(torch.int32)
    assert torch.equal(narrowed.cpu().view(2, N), torch.from_numpy(acts))
    sim.step_with_actions(narrowed.contiguous())
    twin.step(ic.mapped_action(cfg, acts))
    compare(sim, twin, "after the narrowed int64 actions", cfg)
    no_timeout(sim)
    sim.close()


@pytest.mark.parametrize("name,variant", [("full", 2), ("k4r5i5l2", 1), ("k2r4i1l1", 0)], ids=["full_v2", "k4r5i5l2_v1", "k2r4i1l1_v0"])
def test_healing_recount_sees_illegal_moves(name, variant, hip_lib, oracle_lib):
    """Three workgroups, the first held back until a higher one has recounted it from its untouched inputs (`fused_heal_test`):
    the look-back's re-run of the transition (move_world: apply_action_full / apply_action<5> / apply_action<0>) must count
    the same finishing episodes as the real one, or every later episode number -- the dealt hands -- goes wrong."""
    cfg, n = ic.config_of(name), 700
    with debug_knobs({"fused_step": 1, "fused_heal_test": 2, "hanabi.variant": variant}):
        sim = make(cfg, n)
    assert sim.kernel_name == "mrl_hanabi_step_fused"
    orc = oracle_lib.HanabiOracle(cfg, n, num_threads=4)
    total = lockstep(sim, orc, cfg, n, "action_tensor", recounted=slice(0, 256))
    print(f"hanabi {name} variant {variant}, recounted workgroup 0: {total}")
    assert min(total[k] for k in "ABE") >= 100 and total["E at the mover's own hand"] >= 1 and total["episodes ended"] >= 1
    assert total["episodes ended by an illegal move's step"] >= 1
    sim.close()


def test_variants_agree_on_the_full_game(hip_lib, oracle_lib):
    """The same stream through variants 2 and 0 of the full game, one launch and two: every tensor and the record equal after
    every step (a copy of the transition that was changed alone shows here without the oracle).  Not the blocks' bytes that
    no tensor shows: with tokens above the maximum the last state entries move past the 783-entry row, and whether the row's
    one spare byte receives the first of them is left to each encoder."""
    cfg = ic.FULL
    sims = []
    for variant, fused in ((2, 1), (0, 1), (2, 2), (0, 2)):
        with debug_knobs({"fused_step": fused, "hanabi.variant": variant}):
            sims.append(make(cfg, N))
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    total = {}
    for t, rec, acts, cls in ic.walk(orc, cfg):
        for k, v in ic.count_classes(cfg, rec, acts, cls, orc.done).items():
            total[k] = total.get(k, 0) + v
        a = device_actions(acts, N)
        for s in sims:
            s.step_with_actions(a.contiguous())
        for s in sims[1:]:
            same_tensors(sims[0], s, f"at step {t}")
    print(f"hanabi full, variants 2 and 0 side by side: {total}")
    assert min(total[k] for k in "ABE") >= 100 and total["E at the mover's own hand"] >= 1 and total["episodes ended"] >= 1
    no_timeout(*sims)
    for s in sims:
        s.close()


@pytest.mark.parametrize("fused", [1, 2], ids=["one_launch", "two_launches"])
def test_captured_steps_with_illegal_moves(fused, hip_lib, oracle_lib):
    """After mrl_prepare_graph_capture three steps over FIXED action arrays are captured and replayed five times: a hint (half
    the worlds an out-of-table value, half an in-table one that is empty or legal as the hands fall), a discard, and a play
    of slot 0, which burns the life tokens, so episodes end inside the replays.  Tokens go 8, 7, 8, 8: never zero.  Equal to
    the same calls issued eagerly on a second simulator, and to the oracle, which also says which classes occurred."""
    cfg = ic.FULL
    w = np.arange(N)
    pool = ic.out_of_table(cfg)
    hints = np.where(w % 2 == 0, pool[(w // 2) % len(pool)], 10 + (w // 2) % 10).astype(np.int32)
    fixed = [np.stack([a, a]) for a in (hints, (w % 5).astype(np.int32), np.full(N, 5, np.int32))]
    with debug_knobs({"fused_step": fused}):
        eager, graphed = make(cfg, N), make(cfg, N)
    dev = [device_actions(a, N).contiguous() for a in fixed]
    graphed.prepare_graph_capture()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            for a in dev:
                graphed.step_with_actions(a)
    torch.cuda.current_stream().wait_stream(side)
    same_tensors(eager, graphed, "after the capture (nothing ran)")
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    empty = out = own = ended = 0
    for rep in range(5):
        graph.replay()
        for a, host in zip(dev, fixed):
            rec, mask = orc.dump(), orc.mask.copy()
            mover = rec[:, 83].astype(np.int64)
            uid = host[mover, w].astype(np.int64)
            assert ((uid >= 0) & (uid < 10) | (rec[:, 81] > 0)).all(), "a hint at zero tokens"
            in_table = (uid >= 10) & (uid < 20)
            empty += int((in_table & (mask[mover, w, np.clip(uid, 0, 19)] == 0)).sum())
            out += int(((uid >= 20) | (uid < 0)).sum())
            own += int((((uid >= 20) | (uid < 0)) & (ic.reference_hint(cfg, uid)[1] == 1)).sum())
            eager.step_with_actions(a)
            orc.step(ic.mapped_action(cfg, host))
            ended += int(orc.done.sum())
        same_tensors(eager, graphed, f"after replay {rep}")
        compare(graphed, orc, f"after replay {rep}", cfg)
    print(f"hanabi captured steps: {empty} empty hints, {out} out-of-table actions ({own} at the mover's own hand), {ended} episodes ended")
    assert empty >= 100 and own >= 100 and out - own >= 100 and ended >= 100
    assert torch.equal(blocks(eager), blocks(graphed))
    no_timeout(eager, graphed)
    eager.close()
    graphed.close()


@pytest.mark.parametrize("name", ["full", "k5r3i8l3"])
def test_hint_at_zero_tokens_stays_inside_its_world(name, hip_lib, oracle_lib):
    """Class Z, the one move outside the contract: a hint at zero tokens wraps the pool to 255 (the reference then writes far
    past its rows; the oracle is never fed it).  The last four worlds hint until their pools are empty and then once more,
    and go on hinting for twenty further steps, while the oracle's copies of them alternate a discard and a hint: neither
    side's four worlds can finish (no card is played, and twenty cards outlast ten discards), so the episode counter, which
    every world shares, stays the same on both sides -- checked, as the test's own precondition.  Every lower world stays
    bit-exact with the oracle after every step, the calls return and SCAN_TIMEOUT stays 0.  Nothing else is asserted about
    the four worlds themselves."""
    cfg = ic.config_of(name)
    assert hanabi_configs.deck_size(cfg) >= 20
    z = np.arange(N - 4, N)
    low = slice(0, N - 4)
    sim = make(cfg, N)
    orc = oracle_lib.HanabiOracle(cfg, N, num_threads=4)
    rng = np.random.default_rng(11)
    gone = False
    total = {}
    for t in range(cfg["max_information_tokens"] + 21):
        rec, mask = orc.dump(), orc.mask
        acts, cls = ic.choose_with_illegal(rng, cfg, mask, rec)
        mover = rec[z, 83].astype(np.int64)
        legal = mask[mover, z] != 0
        hint = hanabi_configs._pick(rng, legal & (np.arange(20) >= 10))
        discard = hanabi_configs._pick(rng, legal & (np.arange(20) < 5))
        for_oracle, for_device = acts.copy(), acts.copy()
        if not gone and (rec[z, 81] > 0).all():       # drain the pools: a legal hint exists while tokens are left
            assert (hint >= 0).all()
            for_oracle[:, z] = for_device[:, z] = hint
        else:                                         # the class Z move, and every step after it
            assert gone or (rec[z, 81] == 0).all()
            for_device[:, z] = ic.z_hint(rec, z) if not gone else 2 * hanabi_configs.HAND
            for_oracle[:, z] = np.where(rec[z, 81] == 0, discard, hint)  # a discard, then a hint, and so on
            assert (for_oracle[0, z] >= 0).all()
            gone = True
        orc.step(ic.mapped_action(cfg, for_oracle))
        sim.step_with_actions(device_actions(for_device, N).contiguous())
        assert not orc.done[z].any() and not sim.done_tensor().to_torch()[N - 4:].any(), "one of the four worlds finished: the episode counters part"
        compare(sim, orc, f"step {t}", cfg, low)
        assert int(sim.reset_count_tensor().to_torch().item()) == int(orc.done.sum())
        for k, v in ic.count_classes(cfg, rec[low], acts[:, low], cls[low], orc.done[low]).items():
            total[k] = total.get(k, 0) + v
    print(f"hanabi {name}, four worlds hinting at zero tokens; the {N - 4} lower worlds: {total}")
    assert gone and t >= cfg["max_information_tokens"] + 20
    no_timeout(sim)
    sim.close()
