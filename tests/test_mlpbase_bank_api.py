"""CPU: the surface of the balance beam's policy bank (``mrl_mlpbase_act_bank``, ``mrl_mlpbase_bank_resample``,
``mrl_rollout_mlpbase_bank``) that needs no GPU -- symbols, struct layout, the workspace size, the refusals that are raised before
any launch, and the aliasing of a bank's members."""
import ctypes
import re

import pytest
import torch

from madrona_rl_envs_playground_amd import _lib, simulators
from madrona_rl_envs_playground_amd.pantheonrl_extension import MlpBasePopulationAgent
from madrona_rl_envs_playground_amd.simulators import (BankResample, CnnPolicyBank, CnnResample, MappoOptimizer, MlpBaseActorCritic,
                                                         MlpBasePolicy, MlpBasePolicyBank, cross_play, mlpbase_act_bank, mlpbase_resample)

NEW = ("mrl_mlpbase_bank_workspace_bytes", "mrl_mlpbase_act_bank", "mrl_mlpbase_bank_resample", "mrl_rollout_mlpbase_bank")


def test_symbols_abi_and_struct_layout(hip_lib):
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header)
        getattr(hip_lib, name)
    assert re.search(r"#define MRL_ABI_VERSION 4\b", header) and int(hip_lib.mrl_abi_version()) == 4  # additive: the version stays
    assert re.search(r"typedef struct mrl_mlpbase_bank \{", header)
    # mrl_mlpbase_bank { const float *; uint32_t; uint64_t; uint32_t, uint32_t, uint32_t }: 8 + 4 (+ 4) + 8 + 12 (+ 4)
    assert [f[0] for f in _lib.MlpBaseBankDesc._fields_] == ["params_dev", "num_policies", "stride", "hidden", "layer_N", "flags"]
    assert ctypes.sizeof(_lib.MlpBaseBankDesc) == 40 and _lib.MlpBaseBankDesc.stride.offset == 16
    assert (_lib.MlpBaseBankDesc.hidden.offset, _lib.MlpBaseBankDesc.layer_N.offset, _lib.MlpBaseBankDesc.flags.offset) == (24, 28, 32)
    assert BankResample is CnnResample


@pytest.mark.parametrize("n,k", [(1, 1), (17, 1), (70, 5), (300, 256), (1024, 3), (1025, 3), (32768, 4)])
def test_workspace_is_the_cnn_banks_for_two_seats(n, k, hip_lib):
    got = int(hip_lib.mrl_mlpbase_bank_workspace_bytes(n, k))
    assert got == int(hip_lib.mrl_cnn_bank_workspace_bytes(n, 2, k)) > 0 and got % 16 == 0


def test_refusals_without_a_device(hip_lib):
    assert int(hip_lib.mrl_mlpbase_bank_workspace_bytes(33, 0)) == 0
    assert int(hip_lib.mrl_mlpbase_bank_workspace_bytes(33, 257)) == 0
    # no simulator: every call is refused before it looks at anything else
    bank = _lib.MlpBaseBankDesc(None, 1, 0, 64, 2, 0)
    first, num = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(1, 1)
    resample = _lib.CnnResampleDesc(1, first, num, 0)
    assert hip_lib.mrl_mlpbase_act_bank(None, 3, ctypes.byref(bank), None, None, None, 0, 0, 0, 0, None, 0, None) != 0
    assert hip_lib.mrl_mlpbase_bank_resample(None, 3, ctypes.byref(resample), None, None, None) != 0
    assert hip_lib.mrl_rollout_mlpbase_bank(None, 3, ctypes.byref(bank), None, None, None, None, None, 0, 0, None, 0, None) != 0
    for k in (0, 257, -1):
        with pytest.raises(ValueError):
            MlpBasePolicyBank(k, device="cpu")
    with pytest.raises(ValueError):
        MlpBasePolicyBank(2, layer_N=3, device="cpu")
    with pytest.raises(ValueError):
        MlpBasePolicyBank(2, hidden=512, device="cpu")
    with pytest.raises(ValueError):
        MlpBasePolicyBank.from_policies([])
    with pytest.raises(ValueError):
        MlpBasePolicyBank.from_policies([MlpBasePolicy(layer_N=1, device="cpu"), MlpBasePolicy(layer_N=2, device="cpu")])
    with pytest.raises(ValueError):
        MlpBasePolicyBank.from_policies([object()])
    bank = MlpBasePolicyBank(3, device="cpu")
    for k in (-1, 3):
        with pytest.raises(IndexError):
            bank.policy(k)
    with pytest.raises(TypeError):
        MlpBasePopulationAgent(object(), bank)  # not the balance-beam env: no torch fallback
    with pytest.raises(TypeError):
        MlpBasePopulationAgent(object(), object())
    w, h, f = 5, 4, 26
    with pytest.raises(TypeError):
        MlpBasePopulationAgent(object(), CnnPolicyBank(w, h, f, 2, device="cpu"))  # the other network's bank

    class NotTheBeam:
        gpu_id = 0

    ids = torch.zeros((3, 2), dtype=torch.int32)
    with pytest.raises(ValueError, match="BalanceBeamSimulator"):
        mlpbase_act_bank(NotTheBeam(), bank, ids)
    with pytest.raises(ValueError, match="MlpBasePolicyBank"):
        mlpbase_act_bank(NotTheBeam(), bank.policy(0), ids)
    with pytest.raises(ValueError, match="BalanceBeamSimulator"):
        mlpbase_resample(NotTheBeam(), ids, torch.zeros(3, dtype=torch.int32), "robin", 0, 3)

    class FakeEnv:
        sim = NotTheBeam()

    with pytest.raises(ValueError, match="BalanceBeamSimulator"):
        cross_play(FakeEnv(), bank)  # dispatched on the bank's type, refused on the env's


def test_members_are_views_of_the_bank(hip_lib):
    sources = []
    for seed in (1, 2, 3):
        torch.manual_seed(seed)
        sources.append(MlpBasePolicy.from_module(MlpBaseActorCritic(layer_N=1), device="cpu"))
    bank = MlpBasePolicyBank.from_policies(sources)
    assert bank.layer_N == 1 and bank.params.shape == (3, sources[0].num_params) and bank.params.is_contiguous() and len(bank) == 3
    assert bank.num_params == int(hip_lib.mrl_mlpbase_policy_num_params(7, 64, 1, 4)) == 18785
    assert MlpBasePolicyBank(2, device="cpu").num_params == 27361  # layer_N defaults to 2
    desc = bank.desc()
    assert desc.params_dev == bank.params.data_ptr() and desc.num_policies == 3 and desc.stride == bank.num_params
    assert (desc.hidden, desc.layer_N, desc.flags) == (64, 1, 0)
    for k in range(3):
        member = bank.policy(k)
        assert member is bank.policy(k) and isinstance(member, MlpBasePolicy)
        assert member.params.data_ptr() == bank.params[k].data_ptr() == bank.params.data_ptr() + 4 * k * bank.num_params
        assert member.params.is_contiguous() and member.num_params == bank.num_params == member.params.numel() and member.layer_N == 1
        assert torch.equal(member.params, sources[k].params) and member.params.data_ptr() != sources[k].params.data_ptr()
        assert member.desc().params_dev == member.params.data_ptr() and member.desc().layer_N == 1
    # a member's module and optimizer are the stand-alone policy's: parameters alias the row, a step on them moves the bank
    module = bank.policy(1).module()
    assert isinstance(module, MlpBaseActorCritic) and module is bank.policy(1).module()
    at = bank.params[1].data_ptr()
    for p in module.parameters():
        assert p.data_ptr() == at
        at += 4 * p.numel()
    assert at == bank.params[2].data_ptr()
    with torch.no_grad():
        list(module.parameters())[-1].add_(2.5)  # the critic head's bias: the row's last float
    assert float(bank.params[1, -1]) == float(sources[1].params[-1]) + 2.5
    assert torch.equal(bank.params[0], sources[0].params) and torch.equal(bank.params[2], sources[2].params)
    assert MappoOptimizer(bank.policy(1)).policy is bank.policy(1)
    assert simulators.BEAM_TIME == 3
