"""CPU: the surface of the device-side CNN actor-critic (``mrl_cnn_act``, ``mrl_rollout_cnn``) that needs no GPU -- symbols,
parameter counts and order, the module's aliasing and state-dict keys -- and the conditions the GPU tests rest on: the float64
twin against torch float32 on every GPU case's inputs, how many draws lie near a boundary, the integer construction's bound,
the edge draws' exact u."""
import re

import numpy as np
import pytest
import torch

import cnn_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnPolicy, CnnRecord

ALL_CASES = [(layout, n, weights, inputs) for layout, n in twin.CASES for weights in twin.WEIGHTS for inputs in twin.INPUTS]


def test_symbols_and_struct_layouts(hip_lib):
    header = open(_lib.HEADER).read()
    for name in ("mrl_cnn_policy_num_params", "mrl_cnn_workspace_bytes", "mrl_cnn_act", "mrl_rollout_cnn"):
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header)
        getattr(hip_lib, name)
    assert re.search(r"enum \{ MRL_CNN_VALUE_ONLY = 4 \}", header) and _lib.CNN_VALUE_ONLY == 4
    assert [f[0] for f in _lib.CnnRecordDesc._fields_] == ["actions", "logprobs", "values", "rewards", "dones", "next_done", "logits", "num_steps"]
    assert [f[0] for f in _lib.CnnPolicyDesc._fields_] == ["params_dev", "hidden", "flags"]
    assert re.search(r"#define MRL_ABI_VERSION 4\b", header)


@pytest.mark.parametrize("layout", ["cramped_room", "asymmetric_advantages", "coordination_ring", "counter_circuit"])
def test_num_params_is_the_modules(layout, hip_lib):
    w, h, _, f = twin.shape(layout)
    module = CnnActorCritic(w, h, f)
    count = sum(p.numel() for p in module.parameters())
    assert int(hip_lib.mrl_cnn_policy_num_params(w, h, f, 64, 6)) == count
    npos = (w - 2) * (h - 2)
    per_net = 32 * f * 9 + 32 + 64 * 32 * npos + 64 + 64 * 64 + 64
    assert count == 2 * per_net + (6 * 64 + 6) + (64 + 1)
    for bad in ((w, h, f, 128, 6), (w, h, f, 64, 5), (2, h, f, 64, 6), (w, 2, f, 64, 6)):
        assert int(hip_lib.mrl_cnn_policy_num_params(*bad)) == 0
    assert int(hip_lib.mrl_cnn_workspace_bytes(33, 2)) % 16 == 0


def test_parameter_order_is_parameters_to_vector(hip_lib):
    w, h, _, f = twin.shape("cramped_room")
    module = twin.make_module("cramped_room", "trained")
    names = [name for name, _ in module.named_parameters()]
    assert names == [f"actor.base.cnn.cnn.{i}.{kind}" for i in (0, 3, 5) for kind in ("weight", "bias")] + \
        ["actor.act.action_out.linear.weight", "actor.act.action_out.linear.bias"] + \
        [f"critic.base.cnn.cnn.{i}.{kind}" for i in (0, 3, 5) for kind in ("weight", "bias")] + ["critic.v_out.weight", "critic.v_out.bias"]
    policy = CnnPolicy.from_module(module, device="cpu")
    flat = torch.nn.utils.parameters_to_vector(module.parameters()).detach()
    assert torch.equal(policy.params, flat)
    # the twin's split reads the same order
    nets = twin.split(flat.numpy(), w, h, f)
    assert np.array_equal(nets["actor"][0][0], module.actor.base.cnn.cnn[0].weight.detach().double().numpy())
    assert np.array_equal(nets["critic"][3][0], module.critic.v_out.weight.detach().double().numpy())
    assert np.array_equal(nets["critic"][1][1], module.critic.base.cnn.cnn[3].bias.detach().double().numpy())


def test_module_aliases_the_flat_tensor(hip_lib):
    w, h, _, f = twin.shape("cramped_room")
    policy = CnnPolicy.from_module(twin.make_module("cramped_room", "reference"), device="cpu")
    module = policy.module()
    assert module is policy.module() and not hasattr(policy, "load_")
    start, end = policy.params.data_ptr(), policy.params.data_ptr() + 4 * policy.params.numel()
    at = start
    for p in module.parameters():
        assert p.data_ptr() == at
        at += 4 * p.numel()
    assert at == end
    with torch.no_grad():
        module.critic.v_out.bias.add_(1.5)
    assert float(policy.params[-1]) == 1.5  # the reference's biases start at zero
    optimizer = torch.optim.SGD(module.parameters(), lr=0.5)
    before = policy.params.clone()
    module.actor(torch.zeros(2, w, h, f)).sum().backward()
    optimizer.step()
    assert not torch.equal(before, policy.params)


def test_reference_initialisation_and_state_dict_keys(hip_lib):
    w, h, _, f = twin.shape("coordination_ring")
    torch.manual_seed(0)
    module = CnnActorCritic(w, h, f)
    assert sorted(module.actor.state_dict()) == sorted([f"base.cnn.cnn.{i}.{k}" for i in (0, 3, 5) for k in ("weight", "bias")] +
                                                        ["act.action_out.linear.weight", "act.action_out.linear.bias"])
    assert sorted(module.critic.state_dict()) == sorted([f"base.cnn.cnn.{i}.{k}" for i in (0, 3, 5) for k in ("weight", "bias")] +
                                                         ["v_out.weight", "v_out.bias"])
    for name, p in module.named_parameters():
        if name.endswith("bias"):
            assert not p.any(), name
    fc2 = module.actor.base.cnn.cnn[5].weight.detach()
    assert torch.allclose(fc2 @ fc2.T, 2.0 * torch.eye(64), atol=1e-4)  # orthogonal with the ReLU gain
    head = module.actor.act.action_out.linear.weight.detach()
    assert torch.allclose(head @ head.T, 1e-4 * torch.eye(6), atol=1e-7)  # gain 0.01
    # a reference checkpoint is two state dicts under those keys: they load, and change the module
    torch.manual_seed(1)
    donor = CnnActorCritic(w, h, f)
    module.actor.load_state_dict({k: v.clone() for k, v in donor.actor.state_dict().items()})
    module.critic.load_state_dict({k: v.clone() for k, v in donor.critic.state_dict().items()})
    assert torch.equal(torch.nn.utils.parameters_to_vector(module.parameters()), torch.nn.utils.parameters_to_vector(donor.parameters()))


def test_record_shapes_and_rollout_views():
    record = CnnRecord(3, 5, 2, torch.device("cpu"), logits=True)
    assert record.values.shape == (4, 5, 2) and record.logits.shape == (3, 5, 2, 6) and record.next_done.shape == (5, 2)
    r = record.rollout()
    assert r.rewards.shape == (3, 10) and r.next_value.shape == (10,) and r.values.data_ptr() == record.values.data_ptr()
    assert r.next_value.data_ptr() == record.values[3].data_ptr() and r.next_done.data_ptr() == record.next_done.data_ptr()


@pytest.mark.parametrize("layout,n,weights,inputs", ALL_CASES)
def test_twin_against_torch_float32_and_the_boundary_condition(layout, n, weights, inputs, oracle_lib):
    module = twin.make_module(layout, weights)
    obs = twin.case_inputs(layout, n, weights, inputs)["obs"]
    rows = twin.rows_of(obs)
    d_value, d_logp = twin.case_margins(layout, n, weights, inputs)
    # float32 against float64 over K <= 672 products of O(1): a few 1e-6 at most; a twin with a wrong index map is off by O(1)
    assert d_value <= 2e-5 and d_logp <= 5e-5, (d_value, d_logp)
    cap_value, cap_logp = twin.layout_margins(layout, weights)
    assert 0 < d_value <= cap_value and 0 < d_logp <= cap_logp
    # a condition of the GPU test, not a measurement: at most 1 % of the rows have their draw within 1e-5 of a boundary
    u = twin.draws(twin.case_seed(layout, n, weights, inputs), 0, n, obs.shape[1])
    want = twin.act(twin.flat(module), rows, u)
    assert twin.near_boundary(want["cdf"], u).sum() <= 0.01 * len(rows)
    assert ((want["actions"] >= 0) & (want["actions"] <= 5)).all()


@pytest.mark.parametrize("layout", twin.INTEGER_LAYOUTS)
def test_integer_construction_stays_exact_in_float32(layout):
    layers = twin.integer_layers(layout)
    obs = twin.integer_observations(layout)
    values, logits, bound = twin.integer_forward(layers, twin.rows_of(obs))
    assert bound < 2 ** 24
    assert np.abs(twin.integer_params(layers)).max() < 2 ** 24 and (twin.integer_params(layers) == np.round(twin.integer_params(layers))).all()
    # the float64 twin on the same parameters is the integer computation
    v64, l64 = twin.forward(twin.integer_params(layers), twin.rows_of(obs))
    assert np.array_equal(v64, values) and np.array_equal(l64, logits)
    # it tells the maps apart: the H / W swap and the other flatten order give other logits
    lo, hi = twin.TIE
    assert (logits[:, lo] == logits[:, hi]).all() and (logits.argmax(axis=1) == lo).all()
    assert len(np.unique(values)) > len(values) // 2 and (values != 0).any()
    conv = layers["actor"][0][0]
    assert not np.array_equal(conv, conv.transpose(0, 1, 3, 2))  # not symmetric in (i, j)


def test_edge_draws_have_the_exact_u():
    for kind, rows in twin.EDGE_DRAWS.items():
        for seed, seat, world in rows:
            u = twin.draws(seed, 0, twin.EDGE_N, 2)
            assert u[world * 2 + seat] == twin.EDGE_U[kind], (kind, seed, seat, world)
    assert np.float32(twin.EDGE_U["top"]) == twin.EDGE_U["top"] < 1.0
