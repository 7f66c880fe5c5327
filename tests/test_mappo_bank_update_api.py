"""CPU: the surface of the bank update (``mrl_mappo_bank_update``, ``mrl_mappo_mlp_bank_update`` and their workspace functions;
DESIGN.md section 22) that needs no GPU -- symbols, struct layout, the workspace sizes, ``member_samples``, the views of
``ValueNormBank`` and ``MappoBankOptimizer``, and the refusals that are raised before any launch."""
import ctypes
import re

import pytest
import torch

from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import (CnnPolicyBank, MappoBankOptimizer, MappoOptimizer, MlpBasePolicy, MlpBasePolicyBank,
                                                         MlpBaseRecord, ValueNorm, ValueNormBank, mappo_advantages_bank, mappo_update_bank,
                                                         member_samples)

NEW = ("mrl_mappo_bank_workspace_bytes", "mrl_mappo_bank_update", "mrl_mappo_mlp_bank_workspace_bytes", "mrl_mappo_mlp_bank_update")
INVALID = _lib.MRL_ERR_INVALID


def test_symbols_abi_and_struct_layout(hip_lib):
    header = open(_lib.HEADER).read()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header)
        getattr(hip_lib, name)
    assert re.search(r"#define MRL_ABI_VERSION 4\b", header) and int(hip_lib.mrl_abi_version()) == 4 == _lib.ABI_VERSION  # additive
    assert re.search(r"typedef struct mrl_mappo_bank_optimizer \{", header)
    # mrl_mappo_bank_optimizer { float *, *, *; uint64_t; uint32_t x 4 }: 24 + 8 + 16
    desc = _lib.MappoBankOptimizerDesc
    assert [f[0] for f in desc._fields_] == ["params_dev", "exp_avg", "exp_avg_sq", "row_bytes", "num_policies", "first_member",
                                             "num_members", "step"]
    assert ctypes.sizeof(desc) == 48 and desc.row_bytes.offset == 24
    assert (desc.num_policies.offset, desc.first_member.offset, desc.num_members.offset, desc.step.offset) == (32, 36, 40, 44)


@pytest.mark.parametrize("width, rows", [(1, 1), (33, 3), (8225, 1), (2 ** 30, 2)])
@pytest.mark.parametrize("members", [1, 2, 16, 256])
def test_workspace_is_the_plain_one_per_member(hip_lib, width, rows, members):
    plain, bank = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for layer_N in (1, 2):
        assert hip_lib.mrl_mappo_mlp_workspace_bytes(7, 64, layer_N, 4, width, rows, ctypes.byref(plain)) == 0
        assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, layer_N, 4, width, rows, members, ctypes.byref(bank)) == 0
        assert bank.value == members * plain.value and plain.value % 16 == 0
    assert hip_lib.mrl_mappo_workspace_bytes(5, 4, 26, 64, width, rows, ctypes.byref(plain)) == 0
    assert hip_lib.mrl_mappo_bank_workspace_bytes(5, 4, 26, 64, width, rows, members, ctypes.byref(bank)) == 0
    assert bank.value == members * plain.value and plain.value % 16 == 0


def test_workspace_stops_growing_at_the_cap_on_partial_vectors(hip_lib):
    at_cap, far = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 2, 4, 256 * 32 + 33, 1, 2, ctypes.byref(at_cap)) == 0
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 2, 4, 2 ** 30, 1, 2, ctypes.byref(far)) == 0
    assert at_cap.value == far.value > 0


def test_workspace_refusals(hip_lib):
    out = ctypes.c_uint64(0)
    for members in (0, 257):
        assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 2, 4, 33, 1, members, ctypes.byref(out)) == INVALID
        assert hip_lib.mrl_mappo_bank_workspace_bytes(5, 4, 26, 64, 33, 1, members, ctypes.byref(out)) == INVALID
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 3, 4, 33, 1, 2, ctypes.byref(out)) == INVALID  # the plain one's shapes
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 2, 4, 0, 1, 2, ctypes.byref(out)) == INVALID
    assert hip_lib.mrl_mappo_bank_workspace_bytes(5, 4, 26, 512, 33, 1, 2, ctypes.byref(out)) == INVALID
    assert hip_lib.mrl_mappo_bank_workspace_bytes(2, 4, 26, 64, 33, 1, 2, ctypes.byref(out)) == INVALID
    assert hip_lib.mrl_mappo_mlp_bank_workspace_bytes(7, 64, 2, 4, 33, 1, 2, None) == INVALID
    assert hip_lib.mrl_mappo_bank_workspace_bytes(5, 4, 26, 64, 33, 1, 2, None) == INVALID


def test_bank_refusals_that_need_no_device(hip_lib):
    """the bank's own description is checked before anything is dereferenced or enqueued: host arrays stand in for the device's"""
    p = int(hip_lib.mrl_mlpbase_policy_num_params(7, 64, 2, 4))
    host = (ctypes.c_float * 16)()
    at = ctypes.addressof(host)
    policy = _lib.MlpBasePolicyDesc(at, 64, 2, 0)
    batch = _lib.MappoMlpBatch(at, at, at, at, at, at, 4)
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 0)

    def update(policy=policy, opt=None, **changes):
        fields = dict(params_dev=at, exp_avg=at, exp_avg_sq=at, row_bytes=4 * p, num_policies=4, first_member=1, num_members=2, step=0)
        fields.update(changes)
        opt = _lib.MappoBankOptimizerDesc(**fields) if opt is None else opt
        return hip_lib.mrl_mappo_mlp_bank_update(ctypes.byref(policy) if policy else None, ctypes.byref(opt) if opt else None,
                                                 ctypes.byref(batch), at, 1, 4, ctypes.byref(cfg), None, at, 1 << 30, None, None, 0, None)

    assert update(opt=False) == INVALID and b"null optimizer" in hip_lib.mrl_last_error()
    assert update(num_members=0) == INVALID and b"members" in hip_lib.mrl_last_error()
    assert update(first_member=3, num_members=2) == INVALID
    assert update(first_member=0xFFFFFFFF, num_members=2) == INVALID  # no wrap-around
    assert update(num_policies=0) == INVALID and update(num_policies=257, first_member=0, num_members=1) == INVALID
    assert update(row_bytes=4 * p - 4) == INVALID and b"row_bytes" in hip_lib.mrl_last_error()
    assert update(row_bytes=4 * p + 2) == INVALID and b"row_bytes" in hip_lib.mrl_last_error()
    assert update(policy=False) == INVALID
    assert update(policy=_lib.MlpBasePolicyDesc(at + 4, 64, 2, 0)) == INVALID  # not the bank's first row
    assert update(policy=_lib.MlpBasePolicyDesc(at, 64, 3, 0)) == INVALID
    # the kitchens' call checks the same description
    kitchen = _lib.MappoPolicyDesc(at, 64, 0, 5, 4, 26)
    pk = int(hip_lib.mrl_cnn_policy_num_params(5, 4, 26, 64, 6))
    for changes in (dict(num_members=0), dict(first_member=3), dict(num_policies=300), dict(row_bytes=4 * pk - 4), dict(row_bytes=4 * pk + 1)):
        fields = dict(params_dev=at, exp_avg=at, exp_avg_sq=at, row_bytes=4 * pk, num_policies=4, first_member=1, num_members=2, step=0)
        fields.update(changes)
        opt = _lib.MappoBankOptimizerDesc(**fields)
        kbatch = _lib.MappoBatch(at, at, at, at, at, at, 4)
        assert hip_lib.mrl_mappo_bank_update(ctypes.byref(kitchen), ctypes.byref(opt), ctypes.byref(kbatch), at, 1, 4, ctypes.byref(cfg), None, at,
                                             1 << 30, None, None, 0, None) == INVALID, changes


def test_member_samples_on_a_hand_made_owner_table():
    #        world 0  1       2        3       4
    owner = torch.tensor([[0, 0], [1, 1], [2, -1], [0, 1], [1, 0]], dtype=torch.int32)
    got = member_samples(owner, [0, 1], 2)
    assert got.dtype == torch.int32 and got.device == owner.device and tuple(got.shape) == (2, 8)
    # cells (n P + p) of member 0: 0, 1, 6, 9; of member 1: 2, 3, 7, 8; row t adds 10 t
    assert got.tolist() == [[0, 1, 6, 9, 10, 11, 16, 19], [2, 3, 7, 8, 12, 13, 17, 18]]
    assert member_samples(owner, [1], 1).tolist() == [[2, 3, 7, 8]]
    assert member_samples(owner, (k for k in [1, 0]), 1).tolist() == [[2, 3, 7, 8], [0, 1, 6, 9]]  # in the order asked for
    with pytest.raises(ValueError, match="same number"):
        member_samples(owner, [0, 2], 2)  # four cells against one
    with pytest.raises(ValueError, match="same number"):
        member_samples(owner, [3], 2)  # nobody's
    with pytest.raises(ValueError):
        member_samples(owner, [], 2)
    with pytest.raises(ValueError):
        member_samples(owner, [0], 0)
    with pytest.raises(ValueError):
        member_samples(owner.long(), [0], 2)
    with pytest.raises(ValueError):
        member_samples(owner.view(-1), [0], 2)
    # the self-play table of the training tool: world n under member n mod K
    table = (torch.arange(6) % 3).view(6, 1).expand(6, 2).to(torch.int32)
    rows = member_samples(table, range(3), 3)
    assert rows[1].tolist() == [2, 3, 8, 9, 14, 15, 20, 21, 26, 27, 32, 33]
    assert sorted(rows.view(-1).tolist()) == list(range(36))  # every sample is exactly one member's


def test_value_norm_bank_members_are_views():
    bank = ValueNormBank(3, "cpu", beta=0.9, epsilon=1e-3)
    assert tuple(bank.state.shape) == (3, 3) and bank.state.dtype == torch.float32 and len(bank) == 3
    member = bank.member(1)
    assert isinstance(member, ValueNorm) and (member.beta, member.epsilon) == (0.9, 1e-3)
    assert member.state.data_ptr() == bank.state[1].data_ptr() and tuple(member.state.shape) == (3,)
    member.update(torch.tensor([1.0, 3.0]))  # the reference's update, through the view
    assert bank.state[1].tolist() == pytest.approx([0.2, 0.5, 0.1]) and not bank.state[0].any() and not bank.state[2].any()
    bank.state[2, 0] = 7.0
    assert bank.member(2).state[0] == 7.0
    for k in (-1, 3):
        with pytest.raises(IndexError):
            bank.member(k)
    for k in (0, 257):
        with pytest.raises(ValueError):
            ValueNormBank(k, "cpu")


@pytest.mark.parametrize("kind", ["beam", "kitchen"])
def test_bank_optimizer_members_are_views(hip_lib, kind):
    bank = MlpBasePolicyBank(3, layer_N=1, device="cpu") if kind == "beam" else CnnPolicyBank(5, 4, 26, 3, device="cpu")
    optimizer = MappoBankOptimizer(bank, lr=1e-3, critic_lr=2e-3, betas=(0.8, 0.9), eps=1e-6)
    assert tuple(optimizer.exp_avg.shape) == tuple(optimizer.exp_avg_sq.shape) == tuple(bank.params.shape) == (3, bank.num_params)
    assert optimizer.step == 0 and (optimizer.lr, optimizer.critic_lr) == (1e-3, 2e-3)
    optimizer.lr, optimizer.step = 5e-4, 7  # assignable
    member = optimizer.member(2)
    assert isinstance(member, MappoOptimizer) and member.policy is bank.policy(2)
    assert (member.lr, member.critic_lr, member.betas, member.eps, member.step) == (5e-4, 2e-3, (0.8, 0.9), 1e-6, 7)
    assert member.exp_avg.data_ptr() == optimizer.exp_avg[2].data_ptr() and member.exp_avg_sq.data_ptr() == optimizer.exp_avg_sq[2].data_ptr()
    assert member.exp_avg.is_contiguous() and member.exp_avg.numel() == bank.num_params == member.policy.params.numel()
    member.exp_avg.fill_(3.0)
    assert (optimizer.exp_avg[2] == 3.0).all() and not optimizer.exp_avg[:2].any()
    plain, banked = member.workspace_bytes(33, 3), optimizer.workspace_bytes(33, 3, 2)
    assert banked == 2 * plain and optimizer.workspace_bytes(33, 3) == plain
    with pytest.raises(ValueError):
        MappoBankOptimizer(MlpBasePolicy(device="cpu"))
    with pytest.raises(IndexError):
        optimizer.member(3)


def test_python_value_errors_without_a_gpu(hip_lib):
    bank = MlpBasePolicyBank(3, layer_N=1, device="cpu")
    optimizer = MappoBankOptimizer(bank)
    record = MlpBaseRecord(2, 3, 2, "cpu")
    flat = torch.zeros((2, 3, 2))
    indices = torch.zeros((2, 1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="MappoBankOptimizer made for it"):
        mappo_update_bank(bank, MappoBankOptimizer(MlpBasePolicyBank(3, layer_N=1, device="cpu")), record, None, flat, flat, indices)
    with pytest.raises(ValueError, match="MappoBankOptimizer made for it"):
        mappo_update_bank(bank.policy(0), optimizer, record, None, flat, flat, indices)
    with pytest.raises(ValueError, match="ring must be None"):
        mappo_update_bank(bank, optimizer, record, flat, flat, flat, indices)
    with pytest.raises(ValueError, match="ValueNormBank of the bank's size"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices, value_norms=ValueNormBank(2, "cpu"))
    with pytest.raises(ValueError, match="ValueNormBank of the bank's size"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices, value_norms=ValueNorm("cpu"))
    with pytest.raises(ValueError, match="members, rows, minibatch_size"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices[0])
    with pytest.raises(ValueError, match="not rows of a bank"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices, first_member=2)
    with pytest.raises(ValueError, match="not rows of a bank"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices, first_member=-1)
    with pytest.raises(ValueError, match="GPU"):
        mappo_update_bank(bank, optimizer, record, None, flat, flat, indices)
    assert optimizer.step == 0
    cells = member_samples(torch.tensor([[0, 0], [1, 1], [2, 2]], dtype=torch.int32), [0, 1, 2], 2)
    with pytest.raises(ValueError, match="ValueNormBank or None"):
        mappo_advantages_bank(record, cells, ValueNorm("cpu"))
    with pytest.raises(ValueError, match="member_samples"):
        mappo_advantages_bank(record, cells.long())
    with pytest.raises(ValueError, match="member_samples"):
        mappo_advantages_bank(record, cells[:, :3])  # not a whole number of rows
    with pytest.raises(ValueError, match="record must be"):
        mappo_advantages_bank(object(), cells)
