"""No GPU: the recurrent CNN actor-critic's constants, struct layouts and parameter count, ``CnnGruActorCritic``'s names against the
flat tensor, and the conditions of the cases that tests/test_gpu_cnn_gru.py relies on, checked with the twin alone."""
import ctypes

import numpy as np
import pytest
import torch

import cnn_gru_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import CnnGruActorCritic, GruState, MlpBaseGruState


def test_constants_structs_and_parameter_count(hip_lib):
    assert (_lib.CNN_RECURRENT, _lib.CNN_GRU_HIDDEN, _lib.CNN_GRU_MAX_CHUNK) == (16, 0x100, 16) and GruState is MlpBaseGruState
    header = open(_lib.HEADER).read()
    for line in ("enum { MRL_CNN_RECURRENT = 16 };", "enum { MRL_CNN_GRU_HIDDEN = 0x100 };", "enum { MRL_CNN_GRU_MAX_CHUNK = 16 };"):
        assert line in header
    p, r, b = _lib.CnnGruPolicyDesc, _lib.CnnGruRecordDesc, _lib.MappoGruBatch
    assert p.base.offset == 0 and p.h_actor.offset == ctypes.sizeof(_lib.CnnPolicyDesc) == 16 and ctypes.sizeof(p) == 32
    assert r.base.offset == 0 and r.h0_actor.offset == ctypes.sizeof(_lib.CnnRecordDesc) == 64 and ctypes.sizeof(r) == 88
    assert b.base.offset == 0 and b.h0_actor.offset == ctypes.sizeof(_lib.MappoBatch) == 56 and ctypes.sizeof(b) == 96
    assert ctypes.sizeof(_lib.MappoGruPolicyDesc) == ctypes.sizeof(_lib.MappoPolicyDesc)
    L = _lib.lib()
    for key in twin.KITCHENS:
        w, h, _, f = twin.shape(key)
        plain = L.mrl_cnn_policy_num_params(w, h, f, 64, 6)
        assert L.mrl_cnn_policy_num_params(w, h, f, 64 | _lib.CNN_GRU_HIDDEN, 6) == plain + 2 * twin.GRU == len(twin.params_of(key))
        assert 2 * twin.actor_size(key) - 5 * 65 == plain + 2 * twin.GRU
        small, large = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert L.mrl_mappo_workspace_bytes(w, h, f, 64, 33, 2, ctypes.byref(small)) == _lib.MRL_OK
        assert L.mrl_mappo_workspace_bytes(w, h, f, 64 | _lib.CNN_GRU_HIDDEN, 33, 2, ctypes.byref(large)) == _lib.MRL_OK
        assert large.value > small.value + 2 * 2 * 16 * 2 * 32 * 64 * 4  # two workgroups' slices for the longest chunk, per net
    assert L.mrl_cnn_policy_num_params(5, 4, 26, 32 | _lib.CNN_GRU_HIDDEN, 6) == 0


def test_reference_names_load_into_and_out_of_the_flat_tensor():
    w, h, _, f = twin.shape("cramped_room")
    params = twin.params_of("cramped_room")
    module = twin.module_from(params, "cramped_room", torch.float32)
    names = [n for n, _ in module.actor.named_parameters()]
    assert names == ["base.cnn.cnn.0.weight", "base.cnn.cnn.0.bias", "base.cnn.cnn.3.weight", "base.cnn.cnn.3.bias", "base.cnn.cnn.5.weight",
                     "base.cnn.cnn.5.bias", "rnn.rnn.weight_ih_l0", "rnn.rnn.weight_hh_l0", "rnn.rnn.bias_ih_l0", "rnn.rnn.bias_hh_l0",
                     "rnn.norm.weight", "rnn.norm.bias", "act.action_out.linear.weight", "act.action_out.linear.bias"]
    assert [n for n, _ in module.critic.named_parameters()][-2:] == ["v_out.weight", "v_out.bias"]
    other = CnnGruActorCritic(w, h, f)
    other.actor.load_state_dict(module.actor.state_dict())
    other.critic.load_state_dict(module.critic.state_dict())
    assert np.array_equal(torch.nn.utils.parameters_to_vector(other.parameters()).detach().numpy(), params)
    sl = twin.whh_slices("cramped_room")[0]
    assert np.array_equal(params[sl], module.actor.rnn.rnn.weight_hh_l0.detach().numpy().reshape(-1))


@pytest.mark.parametrize("key, n", [("k3x3p1", 65), ("cramped_room", 33), ("simple/1p", 65), ("k8x5p4", 33)])
def test_act_cases_decide_their_draws(key, n):
    p = twin.shape(key)[2]
    inputs = twin.act_inputs(key, n, "nonzero")
    assert inputs["done"].any() and not inputs["done"].all() and inputs["h_actor"].any()
    rows = twin.rows_of(inputs["obs"])
    u = twin.draws(17, 5, n, p)
    exact = twin.act(twin.params_of(key), key, rows, inputs["h_actor"].reshape(-1, 64), inputs["h_critic"].reshape(-1, 64),
                     np.repeat(1.0 - (inputs["done"] != 0), p), u)
    assert (~twin.near_boundary(exact["cdf"], u)).mean() >= 0.9
    assert len(np.unique(exact["actions"])) > 2


@pytest.mark.parametrize("key, L", [("k3x3p1", 2), ("cramped_room", 10), ("k8x5p4", 16)])
def test_update_cases_clip_some_samples_and_not_others(key, L):
    params, batch, ids = twin.update_case(key, L, 33)
    clipfrac = twin.row(params, key, batch, ids[0], twin.Config())["stats"]["clipfrac"]
    assert 0.05 < clipfrac < 0.95
    assert batch.dones.any() and not batch.dones.all() and batch.h0_actor.any() and batch.h0_critic.any()
