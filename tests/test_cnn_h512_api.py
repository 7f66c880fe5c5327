"""CPU: the surface of the hidden-512 CNN act (``mrl_cnn_act`` / ``mrl_rollout_cnn`` with ``hidden`` = 512) that needs no GPU --
parameter counts and order, the module's aliasing, what stays refused -- and the conditions the GPU tests rest on: how many draws
of each forward case lie near a boundary, and the integer construction's bound."""
import numpy as np
import pytest
import torch

import cnn_h512_cases as cases
import cnn_twin as twin
from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, CnnGruPolicy, CnnPolicy, CnnPolicyBank, MappoOptimizer

@pytest.mark.parametrize("key", ["cramped_room", "k3x3p1"])
def test_num_params_is_the_modules(key, hip_lib):
    w, h, _, f = cases.KITCHENS[key][2]
    npos = (w - 2) * (h - 2)
    count = sum(p.numel() for p in CnnActorCritic(w, h, f, hidden=512).parameters())
    assert int(hip_lib.mrl_cnn_policy_num_params(w, h, f, 512, 6)) == count
    assert count == 2 * (256 * 9 * f + 256 + 512 * 256 * npos + 512 + 512 ** 2 + 512) + (6 * 512 + 6) + (512 + 1)
    for bad in ((w, h, f, 128, 6), (w, h, f, 256, 6), (w, h, f, 512 | 0x100, 6), (w, h, f, 512, 5), (2, h, f, 512, 6)):
        assert int(hip_lib.mrl_cnn_policy_num_params(*bad)) == 0

def test_parameter_order_and_aliasing(hip_lib):
    module = cases.make_module("cramped_room", "trained")
    policy = CnnPolicy.from_module(module, device="cpu")
    assert policy.hidden == 512 and policy.desc().hidden == 512
    assert torch.equal(policy.params, torch.nn.utils.parameters_to_vector(module.parameters()).detach())
    aliased, at = policy.module(), policy.params.data_ptr()
    assert aliased is policy.module() and aliased.hidden == 512
    for p in aliased.parameters():
        assert p.data_ptr() == at
        at += 4 * p.numel()
    assert at == policy.params.data_ptr() + 4 * policy.params.numel()
    # the learning phase at 512: torch autograd on the module moves the flat tensor the kernel reads
    before = policy.params.clone()
    aliased.actor(torch.ones(2, 5, 4, 26)).sum().backward()
    torch.optim.SGD(aliased.parameters(), lr=0.5).step()
    assert not torch.equal(before, policy.params)

def test_what_runs_64_only_says_so(hip_lib):
    policy = CnnPolicy(5, 4, 26, hidden=512, device="cpu")
    for refused in (lambda: CnnPolicyBank(5, 4, 26, 2, hidden=512, device="cpu"), lambda: CnnGruPolicy(5, 4, 26, hidden=512, device="cpu"),
                    lambda: MappoOptimizer(policy)):
        with pytest.raises(ValueError, match="device update.*64 only"):
            refused()
    with pytest.raises(ValueError, match="64 or 512"):
        CnnPolicy(5, 4, 26, hidden=128, device="cpu")

@pytest.mark.parametrize("key,n,weights", sorted({case[:3] for case in cases.FORWARD}))
def test_reference_draws_and_margins(key, n, weights):
    ref = cases.reference(key, n, weights)
    assert ref["near"].sum() <= 1  # at most one row whose action a float32 evaluation may decide otherwise
    # float32 against float64 over K <= 5376 products of O(1); a wrong view (H and W swapped) is off by O(1)
    assert 0 < ref["d_value"] <= 1e-4 and 0 < ref["d_logp"] <= 1e-4, (ref["d_value"], ref["d_logp"])

@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_integer_construction_stays_exact_in_float32(key):
    layers, obs = cases.integer_case(key)
    values, logits, bound = twin.integer_forward(layers, twin.rows_of(obs))
    params = twin.integer_params(layers)
    assert bound < 2 ** 24 and np.abs(params).max() < 2 ** 24
    w, h, _, f = cases.KITCHENS[key][2]
    assert params.size == sum(p.numel() for p in CnnActorCritic(w, h, f, hidden=512).parameters())
    # the outputs tell samples and columns apart
    assert len(np.unique(values)) > len(values) // 2 and len(np.unique(logits)) > logits.size // 4
