"""GPU: the Cartpole step (csrc/cartpole.hip) from pole angles beyond pi / 4 (tests/golden/cartpole_wide.npz, written by
tests/golden/make_cartpole_wide_golden.py and checked on the CPU by tests/test_cartpole_wide_fixture.py).  The default
arithmetic (cartpole.variant 3) and the float one (4) evaluate their sin / cos polynomials unconditionally and take the
library's sincosf under ONE branch per thread, with a select per world, where |theta| > pi / 4; a live pole stays within
12 degrees, so only a caller who writes STATE gets there -- and variants 1 and 2 call sincosf with arguments no other test
reaches.

The kernels use 256 threads and four rounds per thread: worlds i0 + 256 u.

Tolerances: `survive` -- the fixture's, 4 x the oracle's largest distance from the reference's float64 step per component
(the oracle itself is up to 2.9 float spacings from it on x_dot: neither "4 spacings of the oracle" nor an absolute 1e-6
is a bound the reference supports at these rates), 10 x that for the float variant, the ratio test_arithmetic_variants
grants it (1e-5 against 1e-6).  `finish` -- the reference's own one-step bound of 1e-6 on the rates
(envs/cartpole_env.py:277; they stay below 4.5, where float rounding is at most 2.4e-7) and one float spacing on position and
angle, which are one multiply-add of the old state (the float variant's constant is float(0.02): test_finish_set adds what
that is off, times the rate).

Measured on the MI355X, device over tolerance per component (x, x_dot, theta, theta_dot): survive, variants 1 to 3
(0, 0.42, 0, 0.26), float (0.5, 0.64, 2.6, 0.51) of an allowed 10; finish, rates 2.2e-7 from the float64 step for all four,
position and angle half a spacing."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN, load_golden  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import CartpoleSimulator, ExecMode  # noqa: E402
from test_gpu_cartpole import VARIANTS  # noqa: E402

WIDE = load_golden("cartpole_wide.npz")
FUSED = [1, 2]
FUSED_IDS = ["one_launch", "two_launches"]
VARIANT_IDS = [VARIANTS[v] for v in sorted(VARIANTS)]


def make(n, variant, fused):
    from madrona_rl_envs_playground_amd._lib import debug_knobs
    with debug_knobs({"cartpole.variant": variant, "fused_step": fused}):
        sim = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    assert sim.kernel_name == ("mrl_cartpole_step_fused" if fused == 1 else "mrl_cartpole_step")
    return sim


def cpu(t):
    return t.to_torch().cpu().numpy()


def plant(sim, state, action):
    sim.observation_tensor().to_torch().copy_(torch.from_numpy(np.ascontiguousarray(state, dtype=np.float32)).cuda())
    sim.action_tensor().to_torch().copy_(torch.from_numpy(np.ascontiguousarray(action, dtype=np.int32)[:, None].copy()).cuda())


@pytest.mark.parametrize("fused", FUSED, ids=FUSED_IDS)
@pytest.mark.parametrize("n", [512, 1025])
@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=VARIANT_IDS)
def test_survive_set(variant, n, fused, hip_lib):
    """one step from the `survive` states, world w taking transition w mod 512: nobody finishes, and the new state --
    rates from the library's sin / cos -- is the reference's within the fixture's tolerance"""
    idx = np.arange(n) % 512
    tol = WIDE["survive_tol"] * (10.0 if variant == 4 else 1.0)
    sim = make(n, variant, fused)
    plant(sim, WIDE["survive_state"][idx], WIDE["survive_action"][idx])
    sim.step()
    got = cpu(sim.observation_tensor()).astype(np.float64)
    assert not cpu(sim.reset_tensor()).any(), "a world of the survive set finished"
    assert int(cpu(sim.reset_count_tensor())[0]) == 0 and (cpu(sim.reward_tensor()) == 1).all()
    err = np.abs(got - WIDE["survive_next"][idx].astype(np.float64))
    print(f"cartpole wide survive variant={variant} n={n} fused={fused}: largest distance from the oracle over the fixture's "
          f"tolerance {err.max(axis=0) / WIDE['survive_tol']} (allowed {tol / WIDE['survive_tol']}), from the float64 reference "
          f"{np.abs(got - WIDE['survive_next64'][idx]).max(axis=0) / WIDE['survive_tol']}")
    assert (err <= tol).all(), err.max(axis=0) / tol
    sim.close()


@pytest.mark.parametrize("variant", sorted(VARIANTS), ids=VARIANT_IDS)
def test_finish_set(variant, hip_lib, oracle_lib):
    """phase 1 of the two-launch step stores every world's post-transition state: all finish, the rates within the
    reference's 1e-6 of its float64 step, position and angle within one float spacing.  Then the one-launch step: every
    world holds its next episode, in world order, bit for bit the oracle's."""
    n = 512
    state, action, next64 = WIDE["finish_state"], WIDE["finish_action"], WIDE["finish_next64"]
    sim = make(n, variant, 2)
    plant(sim, state, action)
    sim.step_phase1(None)
    got = cpu(sim.observation_tensor()).astype(np.float64)
    assert cpu(sim.reset_tensor()).all(), "a world of the finish set lives"
    sim.close()
    err = np.abs(got - next64)
    spacing = np.spacing(np.abs(next64).astype(np.float32)).astype(np.float64)
    print(f"cartpole wide finish variant={variant}: rates {err[:, [1, 3]].max(axis=0)} from the float64 reference (bound 1e-6), "
          f"position and angle {(err / spacing)[:, [0, 2]].max(axis=0)} float spacings (bound 1)")
    assert (err[:, [1, 3]] <= 1e-6).all(), err[:, [1, 3]].max(axis=0)
    # The float variant multiplies by float(0.02), which is 4.5e-10 below the reference's 0.02: its x + tau * x_dot is the
    # exact multiply-add of THAT constant, so it may lie |float(0.02) - 0.02| * |rate| further off -- more than a spacing
    # where |x| < 0.016 (measured: 4.3 spacings at x = 0.004, x_dot = 4).  The other variants take the double constant.
    tau_error = abs(float(np.float32(0.02)) - 0.02) if variant == 4 else 0.0
    bound = spacing[:, [0, 2]] + tau_error * np.abs(state[:, [1, 3]].astype(np.float64))
    assert (err[:, [0, 2]] <= bound).all(), (err[:, [0, 2]] / bound).max(axis=0)
    orc = oracle_lib.CartpoleOracle(n)
    orc.state[:] = state
    orc.step(action)
    assert orc.done.all() and orc.episodes == 2 * n
    sim = make(n, variant, 1)
    plant(sim, state, action)
    sim.step()
    assert cpu(sim.reset_tensor()).all() and int(cpu(sim.reset_count_tensor())[0]) == n
    assert np.array_equal(cpu(sim.observation_tensor()).view(np.uint32), orc.state.view(np.uint32)), "fresh states, in world order"
    assert int(cpu(sim.scan_timeout_tensor())[0]) == 0
    sim.close()


# ---- independence: 2049 in-range worlds, wide states in chosen rounds ----
N = 2049
ROTATE = 256 + 1  # another round of another thread


def _wide_worlds():
    """(world, row of `survive`): the four rounds of thread t of workgroup 0 (worlds 256 u + t) carry the pattern of the
    four bits of t mod 16 -- every subset, none and all included; a sprinkle in workgroup 1 and the one world of the third"""
    out = [256 * u + t for t in range(256) for u in range(4) if (t % 16) >> u & 1]
    out += [1024 + 256 * u + t for t in (0, 63, 64, 255) for u in (t % 4, 3)] + [2048]
    out = sorted(set(out))
    return [(w, k % 512) for k, w in enumerate(out)]


PLANTED = _wide_worlds()


def batch(shift=None):
    """in-range transition 1000 + w mod 1500 of cartpole_transitions.npz (the reset range: nobody finishes) in world w; with
    `shift` the wide states of PLANTED, `shift` worlds further on (mod N)"""
    z = np.load(os.path.join(GOLDEN, "cartpole_transitions.npz"))
    idx = 1000 + np.arange(N) % 1500
    state, action = z["states"][idx].copy(), z["actions"][idx].copy()
    assert (np.abs(state) <= 0.05).all()
    where = np.array([(w + (shift or 0)) % N for w, _ in PLANTED])
    if shift is not None:
        rows = [r for _, r in PLANTED]
        state[where], action[where] = WIDE["survive_state"][rows], WIDE["survive_action"][rows]
    return state, action, where


@pytest.mark.parametrize("variant", [3, 4], ids=[VARIANTS[3], VARIANTS[4]])
def test_a_world_depends_on_neither_its_thread_mates_nor_its_round(variant, hip_lib):
    """the `wide` branch is per thread and its selects per world: an in-range world next to wide ones keeps the result it
    has among in-range worlds, a wide world's result is the same in another round of another thread, and the one-launch and
    the two-launch step agree -- all bit for bit"""
    rows = [r for _, r in PLANTED]
    tol = WIDE["survive_tol"] * (10.0 if variant == 4 else 1.0)
    results = {}
    for fused in FUSED:
        for shift in (None, 0, ROTATE):
            state, action, where = batch(shift)
            sim = make(N, variant, fused)
            plant(sim, state, action)
            sim.step()
            assert not cpu(sim.reset_tensor()).any() and int(cpu(sim.scan_timeout_tensor())[0]) == 0
            results[fused, shift] = cpu(sim.observation_tensor()).copy()
            sim.close()
    for shift in (None, 0, ROTATE):
        assert results[1, shift].tobytes() == results[2, shift].tobytes(), f"shift {shift}: one launch and two launches differ"
    base = results[1, None]
    for shift in (0, ROTATE):
        where = batch(shift)[2]
        in_range = np.ones(N, bool)
        in_range[where] = False
        assert in_range.sum() == N - len(PLANTED)
        assert results[1, shift][in_range].tobytes() == base[in_range].tobytes(), f"shift {shift}: an in-range world depends on its thread-mates"
        err = np.abs(results[1, shift][where].astype(np.float64) - WIDE["survive_next"][rows].astype(np.float64))
        assert (err <= tol).all(), err.max(axis=0) / tol
    assert results[1, 0][batch(0)[2]].tobytes() == results[1, ROTATE][batch(ROTATE)[2]].tobytes(), \
        "a wide world's result depends on its round or its thread-mates"
