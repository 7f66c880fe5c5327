"""GPU: the RECURRENT CNN kernels (``mrl_cnn_gru_act``, ``mrl_mappo_cnn_gru_grad`` and the rollouts that call them) on the kitchens
of tests/kitchen_shape_cases.py (cases: tests/cnn_gru_shape_cases.py), against the float64 twin of tests/cnn_gru_twin.py.  Both
LDS images are maxima of two layouts; the cases sit on either side of each crossover, nearest to it, and run P = 3, npos 12, 13
and 25 and last slabs 23 and 4 wide through the update's forward sweep, row reload and conv phase for the first time.  The three
kitchens past the LDS limit are refused with ``MRL_CNN_RECURRENT`` as without.

The assertions are tests/test_gpu_cnn_gru.py's own, called on these cases: the device within 8 x d, d the float32 CPU
computation's distance from the twin on the same inputs (the scalar stats: pooled per kitchen, ``cnn_gru_shape_cases.stat_margins``).
tests/test_cnn_gru_shapes_api.py asserts the cases' conditions.  Each test prints its ratios."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_gru_shape_cases as cases  # noqa: E402
import kitchen_shape_cases as table  # noqa: E402
import test_gpu_cnn_gru as base  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import CnnGruPolicy, CnnGruRecord, ExecMode, MappoOptimizer, OvercookedSimulator  # noqa: E402
from test_gpu_cnn_gru import DEV, cpu, same_bits  # noqa: E402  (``base.Device`` and ``base.run_act`` run every case)


@pytest.mark.parametrize("key, seats", cases.ACT_CASES)
def test_act_matches_the_twin(hip_lib, key, seats):
    """values, log-probs, logits and both new states within 8 d; h0 written with the incoming state; the other seats' state rows
    and everything outside the act's cells untouched; the same bits on a second run"""
    base.test_act_matches_the_twin(hip_lib, key, cases.N, seats, "nonzero")


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_stats_and_step_match_the_twin(hip_lib, case):
    base.gradient_stats_and_step_match_the_twin(case, cases.twin_rows(case), cases.stat_margins(case[0]))


@pytest.mark.parametrize("key, chunk", cases.UNCHANGED_CASES)
def test_unchanged_parameters_give_the_records_values_and_log_probs(hip_lib, key, chunk):
    """on either side of the update's crossover the forward sweep has the act's bits: ratio exactly 1, value loss and the critic's
    gradient exactly 0"""
    base.test_unchanged_parameters_give_the_records_values_and_log_probs(hip_lib, key, chunk)


@pytest.mark.parametrize("key", table.REFUSED_KEYS)
def test_kitchens_past_the_lds_limit_are_refused_with_the_recurrent_bit(hip_lib, key):
    """``mrl_cnn_act``, ``mrl_rollout_cnn``, ``mrl_mappo_workspace_bytes`` and ``mrl_mappo_update`` refuse the shape; the marked
    record, the states, ACTION, the ring, the parameters and the moments keep every bit"""
    L, n, t, chunk = _lib.lib(), 3, 4, 2
    w, h, p, act_bytes, _ = table.REFUSED[key]
    f = 5 * p + 16
    sim = OvercookedSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **table.layout_params(key))
    assert tuple(sim.observation_world_major_tensor().shape) == (n, p, h, w, f)
    policy = CnnGruPolicy(w, h, f, device=DEV)
    policy.params.normal_(generator=torch.Generator(device=DEV).manual_seed(2))
    state = policy.state(n, p)
    state.actor.fill_(0.5)
    state.critic.fill_(0.25)
    params_before = cpu(policy.params)
    record = base.marked_record(t, n, p, chunk)
    sim.action_tensor().to_torch().fill_(-7)
    space = torch.zeros(int(max(L.mrl_cnn_workspace_bytes(n, p), L.mrl_cnn_bank_workspace_bytes(n, p, 1))) + 256, dtype=torch.uint8, device=DEV)
    ring = torch.zeros((t + 1, n, p, h, w, f), dtype=torch.int8, device=DEV)
    desc, rec, every_seat = policy.desc(), record.struct, (1 << p) - 1
    assert desc.base.flags & _lib.CNN_RECURRENT
    needs = f"a {w} x {h} kitchen with {f} channels needs an LDS image of {act_bytes} bytes per workgroup, the limit is {table.LDS_LIMIT}"
    rc = L.mrl_cnn_act(sim._handle, every_seat, _lib.base_ref(desc), _lib.base_ref(rec), 0, 1, 0, 0, space.data_ptr(), space.numel(), None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_cnn_act: {needs}"
    rc = L.mrl_rollout_cnn(sim._handle, every_seat, _lib.base_ref(desc), _lib.base_ref(rec), ring.data_ptr(), 1, 0, None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_rollout_cnn: {needs}"

    # the update: every array is there, so that the shape is what refuses it
    size = ctypes.c_uint64(0)
    assert L.mrl_mappo_workspace_bytes(w, h, f, 64 | _lib.CNN_GRU_HIDDEN, cases.BC, 1, ctypes.byref(size)) == _lib.MRL_ERR_INVALID
    assert "LDS image does not fit" in L.mrl_last_error().decode() and size.value == 0
    optimizer = MappoOptimizer(policy)
    optimizer.exp_avg.fill_(0.25)
    optimizer.exp_avg_sq.fill_(0.5)
    with pytest.raises(_lib.MrlError, match="LDS image does not fit"):
        optimizer.workspace_bytes(cases.BC, 1)
    count, width = t * n * p, t // chunk * n * p
    plain_record = CnnGruRecord(t, n, p, DEV, chunk_length=chunk)
    (entry, _), shape, make_batch, obs = policy._mappo_batch(plain_record, ring, count)
    advantages, returns = torch.ones((t, n, p), device=DEV), torch.ones((t, n, p), device=DEV)
    batch = make_batch(obs.data_ptr(), plain_record.actions.data_ptr(), plain_record.logprobs.data_ptr(), plain_record.values.data_ptr(),
                       returns.data_ptr(), advantages.data_ptr(), count)
    opt = _lib.MappoOptimizerDesc(policy.params.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), 0)
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1.0 - 0.99999, 1e-5, 0)
    indices = torch.arange(width, dtype=torch.int32, device=DEV).view(1, width)
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    stats = torch.full((1, len(_lib.MAPPO_STATS)), -3.0, device=DEV)
    rc = entry(_lib.base_ref(shape), ctypes.byref(opt), _lib.base_ref(batch), indices.data_ptr(), 1, width, ctypes.byref(cfg), None,
               scratch.data_ptr(), scratch.numel(), stats.data_ptr(), None, 0, None)
    assert rc == _lib.MRL_ERR_INVALID
    assert L.mrl_last_error().decode().startswith("mrl_mappo_update: the kitchen's LDS image does not fit one workgroup's 160 KiB "
                                                  f"(width {w}, height {h}, channels {f}, hidden 64")

    torch.cuda.synchronize()
    for name in base.BUFFERS:
        assert (cpu(getattr(record, name)) == -3).all(), name
    assert (cpu(state.actor) == 0.5).all() and (cpu(state.critic) == 0.25).all()
    assert (cpu(sim.action_tensor()) == -7).all() and not cpu(ring).any() and not cpu(scratch).any() and (cpu(stats) == -3).all()
    same_bits(cpu(policy.params), params_before, "the parameters")
    assert (cpu(optimizer.exp_avg) == 0.25).all() and (cpu(optimizer.exp_avg_sq) == 0.5).all()
    sim.step()  # and the simulator still steps
    torch.cuda.synchronize()
    sim.close()
