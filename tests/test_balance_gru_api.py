"""CPU: the recurrent balance-beam binding without a GPU -- ``MlpBaseGruActorCritic`` / ``MlpBaseGruPolicy`` and the twin of
tests/mlpbase_gru_twin.py against the reference's own ``R_Actor`` / ``R_Critic`` with ``use_recurrent_policy`` through
tests/golden/mlpbase_gru_ref.npz (names, order and count of the flat tensor; one step and one chunk batch with zero masks), the
header's and the binding's constants, the extended ctypes structs, the Python refusals, ``chunk_indices``, and the input conditions
of every case of tests/test_gpu_balance_gru.py -- properties of the twin, not of the device."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import balance_gru_cases as cases
import mlpbase_gru_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd import simulators
from madrona_rl_envs_playground_amd.simulators import (MappoOptimizer, MlpBaseGruActorCritic, MlpBaseGruPolicy, MlpBaseGruRecord,
                                                         MlpBaseGruState, MlpBasePolicy, MlpBasePolicyBank, MlpBaseRecord, chunk_indices,
                                                         mappo_update, mlpbase_act)

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
HEADER = os.path.join(os.path.dirname(HERE), "include", "mrl_envs.h")
BOUND = 2.0 ** -40  # x the largest magnitude of the compared array: float64 dot products of at most 192 terms through about a
#                     dozen layers and steps leave more than 100 x headroom (derived, not measured)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "mlpbase_gru_ref.npz"))


def load_generator():
    spec = importlib.util.spec_from_file_location("make_mlpbase_gru_golden", os.path.join(GOLDEN, "make_mlpbase_gru_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    off, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    print(f"{what}: distance {off:.3e}, bound {BOUND * scale:.3e}")
    assert off <= BOUND * scale, what


# ---------------------------------------------------------------- the C surface

def test_header_and_binding_constants_agree(hip_lib):
    text = open(HEADER).read()
    for name, value in (("MRL_MLPBASE_RECURRENT", _lib.MLPBASE_RECURRENT), ("MRL_MLPBASE_GRU_LAYERS", _lib.MLPBASE_GRU_LAYERS),
                        ("MRL_MLPBASE_GRU_MAX_CHUNK", _lib.MLPBASE_GRU_MAX_CHUNK)):
        found = re.search(rf"enum \{{ {name} = (\w+) \}}", text)
        assert found and int(found.group(1), 0) == value, name
    assert (_lib.MLPBASE_RECURRENT, _lib.MLPBASE_GRU_LAYERS) == (16, 0x100) and _lib.MLPBASE_GRU_MAX_CHUNK >= 16
    assert _lib.MLPBASE_RECURRENT & (_lib.POLICY_GREEDY | _lib.MLPBASE_VALUE_ONLY) == 0
    assert "MRL_ABI_VERSION 4" in text.replace("  ", " ") or re.search(r"MRL_ABI_VERSION\s+4\b", text)


def test_extended_structs_begin_with_the_unchanged_base_structs():
    for extended, base, size, own in ((_lib.MlpBaseGruPolicyDesc, _lib.MlpBasePolicyDesc, 24, ("h_actor", "h_critic")),
                                      (_lib.MlpBaseGruRecordDesc, _lib.MlpBaseRecordDesc, 72, ("h0_actor", "h0_critic", "chunk_length")),
                                      (_lib.MappoMlpGruBatch, _lib.MappoMlpBatch, 56, ("h0_actor", "h0_critic", "dones", "chunk_length",
                                                                                       "num_worlds", "num_seats"))):
        assert ctypes.sizeof(base) == size
        assert extended._fields_[0] == ("base", base) and extended.base.offset == 0 and extended._extends_ is base
        assert tuple(name for name, _ in extended._fields_[1:]) == own
        assert getattr(extended, own[0]).offset == size
    assert (ctypes.sizeof(_lib.MlpBaseGruPolicyDesc), ctypes.sizeof(_lib.MlpBaseGruRecordDesc), ctypes.sizeof(_lib.MappoMlpGruBatch)) == (40, 96, 96)
    plain = _lib.MlpBasePolicyDesc(1, 64, 2, 0)
    assert isinstance(_lib.base_ref(plain), type(ctypes.byref(plain)))
    pointer = _lib.base_ref(_lib.MlpBaseGruPolicyDesc(_lib.MlpBasePolicyDesc(5, 64, 2, 16), 7, 9))
    assert isinstance(pointer, ctypes.POINTER(_lib.MlpBasePolicyDesc)) and pointer.contents.params_dev == 5 and pointer.contents.flags == 16


def test_size_queries(hip_lib):
    L = _lib.lib()
    gru = _lib.MLPBASE_GRU_LAYERS
    assert L.mrl_mlpbase_policy_num_params(7, 64, 2 + gru, 4) == 77537 and L.mrl_mlpbase_policy_num_params(7, 64, 1 + gru, 4) == 68961
    assert L.mrl_mlpbase_policy_num_params(7, 64, 2, 4) == 27361 and L.mrl_mlpbase_policy_num_params(7, 64, 1, 4) == 18785
    for shape in ((7, 64, gru, 4), (7, 64, 3 + gru, 4), (7, 32, 2 + gru, 4), (8, 64, 2 + gru, 4), (7, 64, 2 + gru, 6), (7, 64, 2 + 2 * gru, 4),
                  (7, 64, 0, 4), (7, 64, 3, 4)):
        assert L.mrl_mlpbase_policy_num_params(*shape) == 0, shape
    out = ctypes.c_uint64(0)
    assert L.mrl_mappo_mlp_workspace_bytes(7, 64, 2, 4, 33, 2, ctypes.byref(out)) == 0
    plain = out.value
    assert L.mrl_mappo_mlp_workspace_bytes(7, 64, 2 + gru, 4, 33, 2, ctypes.byref(out)) == 0 and out.value > plain
    for shape in ((7, 64, gru, 4, 33, 2), (7, 64, 3 + gru, 4, 33, 2), (7, 64, 2 + gru, 4, 0, 2), (7, 32, 2 + gru, 4, 33, 2)):
        assert L.mrl_mappo_mlp_workspace_bytes(*shape, ctypes.byref(out)) == _lib.MRL_ERR_INVALID, shape
    assert L.mrl_mappo_mlp_workspace_bytes(7, 64, 2 + gru, 4, 33, 2, None) == _lib.MRL_ERR_INVALID
    for layer_N in (1, 2):
        assert twin.num_params(layer_N) == L.mrl_mlpbase_policy_num_params(7, 64, layer_N + gru, 4)
        assert MlpBaseGruPolicy(layer_N, device="cpu").num_params == twin.num_params(layer_N)


# ---------------------------------------------------------------- the network against the reference

@pytest.mark.parametrize("layer_N", (1, 2))
def test_parameter_names_and_order_are_the_references(golden, layer_N):
    module = MlpBaseGruActorCritic(layer_N=layer_N)
    for which, net in (("actor", module.actor), ("critic", module.critic)):
        assert [name for name, _ in net.named_parameters()] == list(golden[f"n{layer_N}/{which}/parameter_names"])
        assert [p.numel() for p in net.parameters()] == list(golden[f"n{layer_N}/{which}/parameter_sizes"])
    names = [name for name, _ in module.actor.named_parameters()]
    assert names[-8:-2] == ["rnn.rnn.weight_ih_l0", "rnn.rnn.weight_hh_l0", "rnn.rnn.bias_ih_l0", "rnn.rnn.bias_hh_l0", "rnn.norm.weight",
                            "rnn.norm.bias"]
    assert "base.mlp.fc_h.0.weight" in names and names.index("base.mlp.fc_h.0.weight") < names.index("rnn.rnn.weight_ih_l0")
    # the flat tensor is parameters_to_vector of the actor, then of the critic, and module() aliases it
    policy = MlpBaseGruPolicy.from_module(module, device="cpu")
    want = torch.cat([torch.nn.utils.parameters_to_vector(net.parameters()) for net in (module.actor, module.critic)])
    assert torch.equal(policy.params, want.detach())
    alias = policy.module()
    assert isinstance(alias, MlpBaseGruActorCritic) and alias is policy.module()
    with torch.no_grad():
        alias.actor.rnn.rnn.weight_hh_l0[0, 0] = 42.0
    assert policy.params[twin.whh_slices(layer_N)[0]][0] == 42.0
    # the reference's initialisation of the GRU: orthogonal weights, zero biases (rnn.py:14-21)
    for net in (module.actor, module.critic):
        w = net.rnn.rnn.weight_hh_l0.detach().double()
        assert torch.allclose(w.T @ w, torch.eye(64, dtype=torch.float64), atol=1e-5)
        assert not net.rnn.rnn.bias_ih_l0.any() and not net.rnn.rnn.bias_hh_l0.any()


def compare_with(golden_like):
    g, layer_N = golden_like, 2
    params = np.asarray(g["n2/params"], np.float64)
    assert params.shape == (77537,)
    step = twin.act(params, g["rows"], g["h_actor"], g["h_critic"], g["masks"], np.zeros(len(g["rows"])), layer_N)
    close(step["logits"], g["n2/logits"], "one step: logits")
    close(step["values"], g["n2/values"], "one step: values")
    close(step["h_actor"], g["n2/new_h_actor"], "one step: the actor's new state")
    close(step["h_critic"], g["n2/new_h_critic"], "one step: the critic's new state")
    # the chunk batch through the twin's evaluation: L = 3 rows of N = 5 worlds and one seat, chunk n = column n
    L, N = g["chunk_masks"].shape
    zeros = np.zeros((L, N, 1), np.float32)
    batch = twin.Batch(g["chunk_rows"][:, :, None, :], g["chunk_actions"][:, :, None].astype(np.int32), zeros, zeros, zeros, zeros,
                       (1.0 - g["chunk_masks"])[:, :, None].astype(np.float32), g["chunk_h_actor"][None, :, None, :],
                       g["chunk_h_critic"][None, :, None, :], L)
    assert (g["chunk_masks"][1] == 0).any() and (g["chunk_masks"][0] == 0).any()
    module = twin.module_from(params, layer_N)
    with torch.no_grad():
        values, logits, ha, hc, _, _ = twin.evaluate(module, batch, np.arange(N))
        logp = torch.log_softmax(logits, dim=-1)
        taken = logp.gather(-1, torch.from_numpy(np.asarray(g["chunk_actions"])).long().unsqueeze(-1)).squeeze(-1)
        entropy = -(logp.exp() * logp).sum(dim=-1).mean()
    close(taken.numpy(), g["n2/chunk_logp"], "the chunk batch: log-probabilities")
    close(values.numpy(), g["n2/chunk_values"], "the chunk batch: values")
    close(np.array(entropy.item()), g["n2/chunk_entropy"], "the chunk batch: entropy")
    close(ha.numpy(), g["n2/chunk_h_actor_out"], "the chunk batch: the actor's final state")
    close(hc.numpy(), g["n2/chunk_h_critic_out"], "the chunk batch: the critic's final state")
    # MlpBaseGruActorCritic itself, step by step through actor(obs, h, mask) / critic(obs, h, mask)
    h_a, h_c = torch.from_numpy(np.asarray(g["chunk_h_actor"])), torch.from_numpy(np.asarray(g["chunk_h_critic"]))
    with torch.no_grad():
        for i in range(L):
            x, m = torch.from_numpy(np.asarray(g["chunk_rows"][i])).double(), torch.from_numpy(np.asarray(g["chunk_masks"][i]))
            step_logits, h_a = module.actor(x, h_a, m)
            step_values, h_c = module.critic(x, h_c, m)
            close(step_values[:, 0].numpy(), g["n2/chunk_values"][i], f"step {i} of the chunk batch: values")
    close(h_a.numpy(), g["n2/chunk_h_actor_out"], "step by step: the actor's final state")


def test_twin_and_module_match_the_references_numbers(golden):
    compare_with(golden)


def test_golden_is_what_the_reference_gives_today(golden):
    gen = load_generator()
    if not gen.reference_present():
        pytest.skip("no reference tree on this machine: tests/golden/mlpbase_gru_ref.npz is not regenerated (it is still compared against)")
    fresh = gen.generate()
    assert sorted(fresh) == sorted(golden.files)
    for name in golden.files:
        a, b = np.asarray(fresh[name]), golden[name]
        if a.dtype.kind in "fc":
            close(a, b, name)
        else:
            assert np.array_equal(a, b), name


# ---------------------------------------------------------------- Python objects and refusals

def test_state_record_and_chunk_indices():
    policy = MlpBaseGruPolicy(2, device="cpu")
    assert policy.running is None
    state = policy.state(5)
    assert isinstance(state, MlpBaseGruState) and policy.running is state
    assert state.actor.shape == state.critic.shape == (5, 2, 64) and not state.actor.any() and state.actor.dtype == torch.float32
    state.actor.fill_(1.0), state.critic.fill_(2.0)
    state.zero_(worlds=[1, 3])
    assert not state.actor[[1, 3]].any() and state.actor[[0, 2, 4]].all() and not state.critic[[1, 3]].any()
    assert not state.zero_().critic.any() and not state.actor.any()
    other = MlpBaseGruState(5, "cpu")
    assert policy.bind(other) is other and policy.running is other
    with pytest.raises(ValueError, match="state must be an MlpBaseGruState"):
        policy.bind(object())
    record = MlpBaseGruRecord(20, 3, 2, "cpu")
    assert record.chunk_length == 10 and record.h0_actor.shape == record.h0_critic.shape == (2, 3, 2, 64) and record.num_chunks == 12
    assert isinstance(record, MlpBaseRecord) and record.obs.shape == (21, 3, 2, 7)
    assert record.struct.chunk_length == 10 and record.struct.base.num_steps == 20 and record.struct.h0_actor == record.h0_actor.data_ptr()
    assert record.struct.base.obs == record.obs.data_ptr()
    for steps, chunk in ((20, 0), (20, 3), (5, 10)):
        with pytest.raises(ValueError, match="chunk_length"):
            MlpBaseGruRecord(steps, 3, 2, "cpu", chunk_length=chunk)
    generator = torch.Generator().manual_seed(3)
    indices = chunk_indices(record, 3, 4, generator)
    assert indices.shape == (12, 4) and indices.dtype == torch.int32
    for epoch in indices.view(4, 12):
        assert sorted(epoch.tolist()) == list(range(12))
    assert len({tuple(epoch.tolist()) for epoch in indices.view(4, 12)}) > 1
    with pytest.raises(ValueError, match="record must be an MlpBaseGruRecord"):
        chunk_indices(MlpBaseRecord(20, 3, 2, "cpu"), 3, 4)
    with pytest.raises(ValueError):
        chunk_indices(record, 5, 1)  # 12 chunks do not divide into 5 rows


class _Beam(simulators.BalanceBeamSimulator):
    pass


def test_python_refusals(hip_lib):
    with pytest.raises(ValueError, match="layer_N 1 or 2"):
        MlpBaseGruPolicy(3, device="cpu")
    with pytest.raises(ValueError, match="module must be an MlpBaseGruActorCritic"):
        MlpBaseGruPolicy.from_module(simulators.MlpBaseActorCritic())
    with pytest.raises(ValueError, match="module must be an MlpBaseActorCritic"):
        MlpBasePolicy.from_module(MlpBaseGruActorCritic())
    policy = MlpBaseGruPolicy(2, device="cpu")
    with pytest.raises(ValueError, match="bound state"):
        policy.desc()
    # a recurrent policy is an MlpBasePolicy to the type checks, and is refused as one on the wrong simulator
    sim = _Beam.__new__(_Beam)
    sim.gpu_id = 0
    with pytest.raises(ValueError, match=r"^policy\.params must be a contiguous float32 tensor .* on cuda:0$"):
        mlpbase_act(sim, policy)
    with pytest.raises(ValueError, match="policy must be an MlpBasePolicy"):
        mlpbase_act(sim, object())
    # the update: the record's kind, no ring, no bank
    optimizer = MappoOptimizer(policy)
    with pytest.raises(ValueError, match="record must be an MlpBaseGruRecord"):
        mappo_update(policy, optimizer, MlpBaseRecord(2, 3, 2, "cpu"), None, None, None, None)
    with pytest.raises(ValueError, match="ring must be None"):
        mappo_update(policy, optimizer, MlpBaseGruRecord(2, 3, 2, "cpu", chunk_length=1), object(), None, None, None)
    with pytest.raises(ValueError, match="does not take a recurrent policy"):
        policy._mappo_workspace_bytes(4, 1, None, members=2)
    assert optimizer.workspace_bytes(33, 2) > MappoOptimizer(MlpBasePolicy(device="cpu")).workspace_bytes(33, 2)
    assert MlpBasePolicyBank._member_class is MlpBasePolicy


# ---------------------------------------------------------------- the conditions the GPU tests rely on

@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
@pytest.mark.parametrize("weights", cases.WEIGHTS)
def test_act_cases_are_decided(oracle_lib, layer_N, weights):
    params = cases.params_of(layer_N, weights)
    assert params.shape == (twin.num_params(layer_N),)
    for n in cases.ACT_WORLDS:
        for states in cases.STATES:
            inputs = cases.act_inputs(n, states)
            assert inputs["done"].any() and not inputs["done"].all() and (states == "zero") != bool(inputs["h_actor"].any())
            for seats in cases.ACT_SEATS:
                rows, h_actor, h_critic, mask = cases.act_twin_inputs(inputs, seats)
                u = cases.draws(17, 5, n, seats)
                exact = twin.act(params, rows, h_actor, h_critic, mask, u, layer_N)
                assert (~twin.near_boundary(exact["cdf"], u)).mean() > 0.9, (n, states, seats)
                # the mask matters: a masked world's new state is what a zero state would have led to, and is not the unmasked one
                if states == "nonzero":
                    unmasked = twin.act(params, rows, h_actor, h_critic, np.ones_like(mask), u, layer_N)
                    zeroed = twin.act(params, rows, np.zeros_like(h_actor), np.zeros_like(h_critic), mask, u, layer_N)
                    gone = mask == 0
                    assert np.array_equal(exact["h_actor"][gone], zeroed["h_actor"][gone])
                    assert np.abs(exact["h_actor"][gone] - unmasked["h_actor"][gone]).max() > 1e-3
    d = cases.act_margins(layer_N, weights)
    assert all(0 < d[k] < 1e-4 for k in twin.ACT_KINDS), d
    if weights == "trained":
        module = cases.make_module(layer_N, weights)
        assert module.actor.rnn.rnn.bias_hh_l0.abs().max() > 0.1 and module.critic.rnn.norm.bias.abs().max() > 0.1


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_update_cases_hold_their_conditions(oracle_lib, case):
    fixed = cases.fixed_case(case)
    layer_N, _, width, length, _ = case
    batch, indices = fixed["batch"], fixed["indices"]
    assert indices.shape == (1, width) and len(set(indices[0].tolist())) == width and indices.max() < 2 * cases.N * cases.P
    assert twin.conditions_hold(fixed), (fixed["twin"]["kink"], twin.relu_margin(fixed))
    masked = cases.masked_steps(batch, indices[0])
    assert masked.shape == (length, width)
    # the row's first chunk has its mask zero at its first, its middle and its last step; some step of the row is unmasked
    assert masked[[0, length // 2, length - 1], 0].all() and (width * length <= 2 or not masked.all())
    d = twin.row_margins(fixed["twin"], fixed["f32"])
    assert 0 < d["grad"] < 1e-4
    grad = fixed["twin"]["grad"]
    assert not any(grad[sl].any() for sl in twin.fc_h_slices(layer_N))
    if not masked.all():  # (a state that is never masked out reaches weight_hh_l0)
        assert all(np.abs(grad[sl]).max() > 1e-6 for sl in twin.whh_slices(layer_N))
    if width >= 33:  # more than one workgroup's share per net
        assert -(-width // 32) >= 2
