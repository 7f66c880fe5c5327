"""GPU: what a wave of the Overcooked single step does in front of its stores -- the holder table reached through the
terrain table's pointer and requested with the state loads (and whatever else that part of the kernels is reordered
into) -- changes no byte.

Every world, every byte of observations, rewards, done flags, cells, players and clocks is compared against the CPU
oracle after each of 100 steps; horizon 40, so both resets and the urgency pass run.  The observation slab is filled with
a poison byte before every step, so a byte no store reaches shows too.  The cases walk the kernel families that share
that code (one group per wave, two groups per wave, the generic kernel with and without cell words past the register
batch), ragged and empty groups, both action types and both write-back flavours, and a caller's ring slot."""
import zlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from madrona_rl_envs_playground_amd import layouts  # noqa: E402
from madrona_rl_envs_playground_amd._lib import debug_knobs  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import ExecMode, OvercookedSimulator  # noqa: E402

POISON = 0x5A
HORIZON = 40
STEPS = 100

ALL_MODES = [("int32", 1), ("int32", 2), ("int64", 1), ("int64", 2)]  # action type, overcooked.writeback (1 = every word, 2 = changed only)
TWO_MODES = [("int32", 2), ("int64", 1)]

# name -> (layout, worlds, knobs, kernel family, modes)
CASES = {}
for n in (1, 7, 9, 33, 1003):  # eight worlds per wave: a lone world, ragged groups, workgroups with empty waves, many workgroups
    for groups, family in ((1, "step_fixed<"), (2, "step_groups_fixed<")):
        CASES[f"cramped_room_{n}_groups{groups}"] = ("cramped_room", n, {"overcooked.wpw": 8, "overcooked.groups": groups}, family,
                                                     ALL_MODES if n == 1003 else TWO_MODES)
for layout, n in (("asymmetric_advantages", 259), ("coordination_ring", 333), ("forced_coordination", 261), ("counter_circuit", 515)):
    for groups, family in ((1, "step_fixed<"), (2, "step_groups_fixed<")):
        CASES[f"{layout}_{n}_groups{groups}"] = (layout, n, {"overcooked.wpw": 4, "overcooked.groups": groups}, family, TWO_MODES)
CASES["cramped_room_generic"] = ("cramped_room", 333, {"overcooked.no_fixed": 1, "overcooked.wpw": 8}, "mrl_overcooked_step<", ALL_MODES)
# 16 worlds per wave are 320 cell words, more than the 256 a wave keeps in registers
CASES["cramped_room_generic_wide"] = ("cramped_room", 333, {"overcooked.no_fixed": 1, "overcooked.wpw": 16}, "mrl_overcooked_step<", ALL_MODES)

PARAMS = [pytest.param(case, i64, wb, id=f"{case}-{i64}-wb{wb}") for case, spec in CASES.items() for i64, wb in spec[4]]


def unpack_players(t):
    """(N,P,8) uint8 -> (N,P,6) in the oracle's dump order."""
    t = t.cpu().numpy()
    return np.stack([t[..., 0], t[..., 1], t[..., 4], t[..., 5], t[..., 6], t[..., 7]], axis=-1)


_trace = {}  # the most recent (layout, worlds): the oracle's run, shared by the cases that step the same batch


def oracle_trace(oracle_lib, layout, n):
    """Per step: actions and what the oracle holds behind them (observations, rewards, done flags, players, cells, clocks)."""
    if (layout, n) not in _trace:
        _trace.clear()
        params = layouts.get_base_layout_params(layout, HORIZON)
        P = params["num_players"]
        orc = oracle_lib.OvercookedOracle(params, n, num_threads=8)
        rng = np.random.default_rng(zlib.crc32(f"{layout} {n}".encode()))
        steps = []
        for _ in range(STEPS):
            acts = rng.integers(0, 5, size=(P, n)).astype(np.int32)
            acts[rng.random((P, n)) < 0.35] = 5  # enough interactions for pots to fill, cook and be served
            orc.step(acts)
            steps.append((acts, orc.obs.copy(), orc.reward.copy(), orc.done.copy()) + orc.dump())
        orc.close()
        assert sum(int(s[3].sum()) for s in steps) == 2 * n  # both resets
        _trace[(layout, n)] = steps
    return _trace[(layout, n)]


def run_case(oracle_lib, layout, n, knobs, kernel, i64, writeback, ring_slots=0):
    params = layouts.get_base_layout_params(layout, HORIZON)
    P, C = params["num_players"], params["height"] * params["width"]
    F = 5 * P + 16
    with debug_knobs(dict(knobs, **{"overcooked.writeback": writeback})):
        sim = OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)
    assert kernel in sim.kernel_name, sim.kernel_name
    own = sim.observation_world_major_tensor().to_torch()
    ring = None
    if ring_slots:
        ring = torch.full((ring_slots,) + tuple(own.shape), POISON, dtype=torch.int8, device="cuda")
        sim.set_observation_ring(ring)
    for t, (acts, obs, reward, done, players, objects, clock) in enumerate(oracle_trace(oracle_lib, layout, n)):
        out = ring[t % ring_slots] if ring_slots else own
        out.fill_(POISON)
        a = torch.from_numpy(acts).cuda().view(P, n, 1)
        if i64 == "int64":
            sim.step_with_actions_i64(a.to(torch.int64))
        else:
            sim.step_with_actions(a)
        assert np.array_equal(out.cpu().numpy().astype(np.uint8).reshape(n, P, C, F), obs), f"obs, step {t}"
        assert np.array_equal(sim.reward_tensor().to_torch().cpu().numpy(), reward), f"reward, step {t}"
        assert np.array_equal(sim.done_tensor().to_torch().cpu().numpy(), done), f"done, step {t}"
        assert np.array_equal(sim.state_objects_tensor().to_torch().cpu().numpy(), objects), f"objects, step {t}"
        assert np.array_equal(unpack_players(sim.state_players_tensor().to_torch()), players), f"players, step {t}"
        assert np.array_equal(sim.state_timestep_tensor().to_torch().cpu().numpy(), clock), f"timestep, step {t}"
    if ring_slots:  # the other slots keep what their own steps wrote; the simulator's own tensor was never written
        for back in range(1, ring_slots):
            want = oracle_trace(oracle_lib, layout, n)[STEPS - 1 - back][1]
            assert np.array_equal(ring[(STEPS - 1 - back) % ring_slots].cpu().numpy().astype(np.uint8).reshape(n, P, C, F), want)
    sim.close()


@pytest.mark.parametrize("case,i64,writeback", PARAMS)
def test_every_byte_after_every_step(case, i64, writeback, hip_lib, oracle_lib):
    layout, n, knobs, kernel, _ = CASES[case]
    run_case(oracle_lib, layout, n, knobs, kernel, i64, writeback)


def test_into_a_ring_slot(hip_lib, oracle_lib):
    """The step writes a caller's rollout buffer, slot after slot, instead of the simulator's own tensor."""
    layout, n, knobs, kernel, _ = CASES["cramped_room_1003_groups1"]
    run_case(oracle_lib, layout, n, knobs, kernel, "int32", 2, ring_slots=3)
