"""CPU: the balance beam's MAPPO binding without a GPU -- ``MlpBaseActorCritic`` / ``MlpBasePolicy`` against the reference's own
``R_Actor`` / ``R_Critic`` through tests/golden/balance_mlpbase_ref.npz (names, shapes, order and count of the flat tensor; the
twin's logits and values), the views of ``module()``, ``fc_h``, the ctypes structs and symbols, the Python refusals, and the input
conditions of every parity case of tests/test_gpu_balance_mappo.py -- properties of the twin, not of the device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

import balance_mappo_cases as cases
import mlpbase_twin as twin
from conftest import GOLDEN
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnPolicyBank, CnnRecord, MappoOptimizer, MlpBaseActorCritic, MlpBasePolicy, MlpBaseRecord,
                                                         mappo_advantages, mappo_update)

CPU = torch.device("cpu")
SIZES = {1: (9490, 9295), 2: (13778, 13583)}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "balance_mlpbase_ref.npz"))


def load_generator():
    spec = importlib.util.spec_from_file_location("make_balance_mlpbase_golden", os.path.join(GOLDEN, "make_balance_mlpbase_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def golden_module(golden, layer_N, dtype=torch.float64):
    """``MlpBaseActorCritic`` holding the golden state dicts, loaded by name (strict: the keys are the reference's)"""
    module = MlpBaseActorCritic(layer_N=layer_N).to(dtype)
    for which, net in (("actor", module.actor), ("critic", module.critic)):
        state = {str(name): torch.from_numpy(golden[f"n{layer_N}/{which}/{name}"]).to(dtype) for name in golden[f"n{layer_N}/{which}/names"]}
        net.load_state_dict(state, strict=True)
    return module


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_flat_tensor_is_the_references_names_shapes_order_and_count(hip_lib, golden, layer_N):
    module = MlpBaseActorCritic(layer_N=layer_N)
    for which, net, size in (("actor", module.actor, SIZES[layer_N][0]), ("critic", module.critic, SIZES[layer_N][1])):
        names = [name for name, _ in net.named_parameters()]
        assert names == [str(n) for n in golden[f"n{layer_N}/{which}/parameter_names"]]
        assert list(net.state_dict()) == [str(n) for n in golden[f"n{layer_N}/{which}/names"]]
        for name, p in net.named_parameters():
            assert tuple(p.shape) == golden[f"n{layer_N}/{which}/{name}"].shape, name
        assert sum(p.numel() for p in net.parameters()) == size == (twin.actor_size(layer_N) if which == "actor" else twin.actor_size(layer_N) - 195)
    assert hip_lib.mrl_mlpbase_policy_num_params(7, 64, layer_N, 4) == sum(SIZES[layer_N])
    policy = MlpBasePolicy.from_module(golden_module(golden, layer_N, torch.float32), device=CPU)
    assert policy.params.numel() == sum(SIZES[layer_N])
    # the flat order: actor then critic, parameters_to_vector's
    at = 0
    for which in ("actor", "critic"):
        for name in golden[f"n{layer_N}/{which}/parameter_names"]:
            want = golden[f"n{layer_N}/{which}/{name}"].astype(np.float32).reshape(-1)
            assert np.array_equal(policy.params[at:at + want.size].numpy(), want), (which, name)
            if str(name) == "base.mlp.fc_h.0.weight":
                assert at == (0 if which == "actor" else SIZES[layer_N][0]) + 654
            at += want.size
    assert at == policy.params.numel()


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_module_views_alias_the_flat_tensor(hip_lib, layer_N):
    policy = MlpBasePolicy(layer_N=layer_N, device=CPU)
    module = policy.module()
    assert policy.module() is module
    at = 0
    for p in module.parameters():
        assert p.data_ptr() == policy.params.data_ptr() + 4 * at
        at += p.numel()
    policy.params.fill_(0.5)
    assert all((p == 0.5).all() for p in module.parameters())
    with torch.no_grad():
        module.critic.v_out.bias.fill_(3.0)
    assert policy.params[-1] == 3.0
    desc = policy.desc()
    assert (desc.params_dev, desc.hidden, desc.layer_N, desc.flags) == (policy.params.data_ptr(), 64, layer_N, 0)


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_fc2_clones_equal_fc_h_at_construction(layer_N):
    torch.manual_seed(layer_N)
    module = MlpBaseActorCritic(layer_N=layer_N)
    for net in (module.actor, module.critic):
        mlp = net.base.mlp
        assert len(mlp.fc2) == layer_N
        for clone in mlp.fc2:
            assert clone is not mlp.fc_h
            for a, b in zip(clone.parameters(), mlp.fc_h.parameters()):
                assert torch.equal(a, b) and a.data_ptr() != b.data_ptr()
        assert (mlp.fc1[2].weight == 1).all() and (mlp.fc1[0].bias == 0).all() and (net.base.feature_norm.bias == 0).all()
    head, v_out = module.actor.act.action_out.linear.weight, module.critic.v_out.weight
    assert torch.allclose(head @ head.T, 1e-4 * torch.eye(4), atol=1e-7) and torch.allclose(v_out @ v_out.T, torch.eye(1), atol=1e-6)
    # fc_h takes no part in the forward pass
    x = torch.randn(5, 7)
    before = module.actor(x)
    with torch.no_grad():
        module.actor.base.mlp.fc_h[0].weight.add_(1.0)
    assert torch.equal(module.actor(x), before)


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_twin_reproduces_the_golden_logits_and_values(golden, layer_N):
    params = twin.flat(golden_module(golden, layer_N))
    rows = golden["rows"]
    assert (rows[0] == rows[0][0]).all()  # the row of variance 0
    got = twin.act(params, rows, np.zeros(len(rows)), layer_N)
    tag = f"n{layer_N}"
    assert np.abs(got["logits"] - golden[f"{tag}/logits"]).max() < 1e-12
    assert np.abs(got["logp"] - golden[f"{tag}/logp"]).max() < 1e-12
    assert np.abs(got["values"] - golden[f"{tag}/values"]).max() < 1e-12
    assert np.array_equal(got["greedy"], golden[f"{tag}/greedy"])
    # the module's own forward, as a user calls it
    module = golden_module(golden, layer_N)
    with torch.no_grad():
        action, logp, _, value = module.get_action_and_value(torch.from_numpy(rows).double(), deterministic=True)
    assert np.array_equal(action.numpy(), golden[f"{tag}/greedy"]) and np.abs(value[:, 0].numpy() - golden[f"{tag}/values"]).max() < 1e-12


def test_golden_file_is_what_the_reference_writes(golden):
    gen = load_generator()
    if not gen.reference_present():
        pytest.skip("no reference tree (%s): the committed fixture cannot be regenerated here" % gen.reference_dir())
    fresh = gen.generate()
    assert sorted(fresh) == sorted(golden.files)
    for name, value in fresh.items():
        assert np.array_equal(np.asarray(value), golden[name]), name


def test_ctypes_structs_and_symbols(hip_lib):
    for symbol in ("mrl_mlpbase_policy_num_params", "mrl_mlpbase_act", "mrl_rollout_mlpbase", "mrl_mappo_mlp_workspace_bytes",
                   "mrl_mappo_mlp_update"):
        assert symbol in _lib.SYMBOLS and hasattr(hip_lib, symbol)
    header = open(_lib.HEADER).read()
    assert "MRL_MLPBASE_VALUE_ONLY = 4" in header and _lib.MLPBASE_VALUE_ONLY == 4
    assert ctypes.sizeof(_lib.MlpBasePolicyDesc) == 24 and _lib.MlpBasePolicyDesc.layer_N.offset == 12
    assert ctypes.sizeof(_lib.MlpBaseRecordDesc) == 72 and _lib.MlpBaseRecordDesc.obs.offset == 56 and _lib.MlpBaseRecordDesc.num_steps.offset == 64
    assert ctypes.sizeof(_lib.MappoMlpBatch) == ctypes.sizeof(_lib.MappoBatch) == 56
    assert hip_lib.mrl_abi_version() == 4
    out = ctypes.c_uint64(0)
    assert hip_lib.mrl_mappo_mlp_workspace_bytes(7, 64, 2, 4, 65, 1, ctypes.byref(out)) == 0
    one_tile = out.value
    assert hip_lib.mrl_mappo_mlp_workspace_bytes(7, 64, 2, 4, 1, 1, ctypes.byref(out)) == 0 and out.value < one_tile
    # at most 256 partial vectors per net: the workspace stops growing
    assert hip_lib.mrl_mappo_mlp_workspace_bytes(7, 64, 2, 4, 256 * 32, 1, ctypes.byref(out)) == 0
    cap = out.value
    assert hip_lib.mrl_mappo_mlp_workspace_bytes(7, 64, 2, 4, 1 << 20, 1, ctypes.byref(out)) == 0 and out.value == cap
    for bad in ((7, 64, 3, 4), (7, 512, 2, 4), (6, 64, 2, 4), (7, 64, 2, 6), (7, 64, 0, 4)):
        assert hip_lib.mrl_mlpbase_policy_num_params(*bad) == 0
        assert hip_lib.mrl_mappo_mlp_workspace_bytes(*bad, 65, 1, ctypes.byref(out)) == _lib.MRL_ERR_INVALID


def test_python_refusals(hip_lib):
    with pytest.raises(ValueError):
        MlpBasePolicy(hidden=512, device=CPU)
    with pytest.raises(ValueError):
        MlpBasePolicy(layer_N=3, device=CPU)
    with pytest.raises(ValueError):
        MlpBasePolicy.from_module(torch.nn.Linear(2, 2))
    policy = MlpBasePolicy(device=CPU)
    record = MlpBaseRecord(2, 3, 2, CPU, logits=True)
    assert record.obs.shape == (3, 3, 2, 7) and record.obs.dtype == torch.int32 and record.logits.shape == (2, 3, 2, 4)
    rollout = record.rollout()
    assert rollout.values.shape == (2, 6) and rollout.next_value.shape == (6,)
    optimizer = MappoOptimizer(policy)
    assert optimizer.exp_avg.shape == policy.params.shape and optimizer.workspace_bytes(65, 1) > 0
    with pytest.raises(ValueError):
        MappoOptimizer(object())
    with pytest.raises(ValueError):
        mappo_advantages(object())
    z = torch.zeros((2, 3, 2))
    indices = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="ring must be None"):
        mappo_update(policy, optimizer, record, torch.zeros(4, dtype=torch.int8), z, z, indices)
    with pytest.raises(ValueError, match="MlpBaseRecord"):
        mappo_update(policy, optimizer, CnnRecord(2, 3, 2, CPU), None, z, z, indices)
    with pytest.raises(ValueError):
        mappo_update(policy, MappoOptimizer(MlpBasePolicy(device=CPU)), record, None, z, z, indices)  # another policy's optimizer
    with pytest.raises(ValueError, match="GPU"):
        mappo_update(policy, optimizer, record, None, z, z, indices)  # the parameters are not on a GPU
    # the kitchens' errors are what they were
    cnn = CnnPolicy(5, 4, 26, device=CPU)
    with pytest.raises(ValueError, match="CnnRecord"):
        mappo_update(cnn, MappoOptimizer(cnn), record, None, z, z, indices)
    member = CnnPolicyBank(5, 4, 26, 2, device=CPU).policy(1)  # a bank's member is a CnnPolicy like any other
    with pytest.raises(ValueError, match="CnnRecord"):
        mappo_update(member, MappoOptimizer(member), record, None, z, z, indices)
    assert MappoOptimizer(member).workspace_bytes(65, 1) == MappoOptimizer(cnn).workspace_bytes(65, 1) > 0
    with pytest.raises(ValueError, match="CnnPolicy"):
        mappo_update(object(), optimizer, record, None, z, z, indices)


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_input_conditions_of_the_update_cases(oracle_lib, case):
    """no pre-activation closer to 0 than 8 x its float32 error (one exactly 0 in both computations decides nothing), no sample
    within KINK of a kink of the loss; and the case is worth running: both branches of every clamp are taken where B allows"""
    fixed = cases.fixed_case(case)
    closest, worst = twin.relu_margin(fixed)
    assert fixed["twin"]["kink"] > twin.KINK, fixed["twin"]["kink"]
    assert closest > twin.FACTOR * worst, (closest, worst)
    assert twin.row_margins(fixed["twin"], fixed["f32"])["grad"] > 0
    if case[3] >= 31:
        b = fixed["twin"]["branches"]
        assert 0 < b["ratio_clipped"] < 1
        if fixed["cfg"].clipped_value:
            assert 0 < b["value_clipped"] < 1
        if fixed["cfg"].huber:
            assert b["huber_above"] > 0 and b["huber_below"] > 0
    # the twin's gradient has no fc_h component, and every other tensor has one
    grad = fixed["twin"]["grad"]
    for sl in twin.fc_h_slices(case[0]):
        assert not grad[sl].any()
    if case[3] >= 31:
        assert np.abs(grad[twin.used(case[0])]).max() > 0


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
@pytest.mark.parametrize("weights", cases.WEIGHTS)
def test_input_conditions_of_the_act_cases(oracle_lib, layer_N, weights):
    params = cases.params_of(layer_N, weights)
    start = twin.flat(MlpBaseActorCritic(layer_N=layer_N))
    if weights == "trained":  # no tensor at its initial value: LayerNorm off (1, 0), biases off 0
        module = cases.make_module(layer_N, weights)
        for name, p in module.named_parameters():
            if p.dim() == 1:
                target = 1.0 if name.endswith(("2.weight", "feature_norm.weight")) else 0.0
                assert (p != target).all(), name
    assert params.size == start.size
    d_value, d_logp, d_logits = cases.act_margins(layer_N, weights)
    assert d_value > 0 and d_logp > 0 and d_logits > 0
    for n in cases.ACT_WORLDS:
        for inputs in cases.INPUTS:
            obs = cases.act_inputs(n, inputs)
            assert obs.shape == (2, n, 7) and obs[:, :, :6].min() >= 0 and obs[:, :, :6].max() <= 8 and obs[:, :, 6].max() <= 2
            rows = cases.rows_of(obs)
            if inputs == "synthetic":
                assert (rows[cases.CONSTANT_ROW] == 2).all()
            exact = twin.act(params, rows, np.zeros(len(rows)), layer_N)
            single = twin.act(params, rows, np.zeros(len(rows)), layer_N, torch.float32)
            assert np.isfinite(exact["values"]).all() and np.isfinite(single["logp"]).all()
            # pre-activations: none closer to 0 than 8 x its float32 error, unless exactly 0 in both
            with torch.no_grad():
                pre64 = [z.numpy() for z in twin.forward(twin.module_from(params, layer_N), rows)[2]]
                pre32 = [z.double().numpy() for z in twin.forward(twin.module_from(params, layer_N, torch.float32), rows)[2]]
            closest, worst = twin.relu_margin({"twin": {"pre": pre64}, "f32": {"pre": pre32}})
            assert closest > twin.FACTOR * worst, (n, inputs, closest, worst)
