"""No GPU: the surface of ``mrl_ppo_update`` -- symbols, refusals, the workspace size --, the float64 twin of tests/ppo_twin.py
against torch's own lines, ``clip_grad_norm_`` and ``Adam``, the branch conditions of every case the GPU tests run, and the
Python layer (``minibatch_indices``, ``PpoOptimizer``, the ValueErrors of ``ppo_update``)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ppo_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import MlpPolicy, PpoOptimizer, Rollout, minibatch_indices, ppo_update

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mrl_ppo_workspace_bytes", "mrl_ppo_update")


def workspace_bytes(lib, width, rows=1, shape=(4, 64, 2)):
    out = ctypes.c_uint64(0)
    rc = lib.mrl_ppo_workspace_bytes(shape[0], shape[1], shape[2], width, rows, ctypes.byref(out))
    return rc, out.value


def test_symbols(hip_lib):
    header = open(os.path.join(REPO, "include", "mrl_envs.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.mrl_abi_version() == 4 == _lib.ABI_VERSION
    assert "#define MRL_ABI_VERSION 4" in header


class Call:
    """A well-formed argument list of mrl_ppo_update over dummy non-NULL addresses (nothing is dereferenced before the
    refusals under test), one piece of which a test breaks."""

    def __init__(self, lib):
        self.lib = lib
        self.shape = _lib.MlpPolicyDesc(0, 4, 64, 2, 0, 0)
        self.opt = _lib.PpoOptimizerDesc(4096, 4096, 4096, 0)
        self.batch = _lib.PpoBatch(4096, 4096, 4096, 4096, 4096, 4096, 128)
        self.cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, _lib.PPO_NORM_ADV | _lib.PPO_CLIP_VLOSS)
        self.indices, self.rows, self.width, self.workspace, self.workspace_bytes = 4096, 1, 64, 4096, 1 << 40

    def refused(self, **null):
        ref = lambda name, value: None if null.get(name) else ctypes.byref(value)  # noqa: E731
        rc = self.lib.mrl_ppo_update(ref("shape", self.shape), ref("opt", self.opt), ref("batch", self.batch),
                                     None if null.get("indices") else self.indices, self.rows, self.width, ref("cfg", self.cfg),
                                     None if null.get("workspace") else self.workspace, self.workspace_bytes, None, None, 0, None)
        message = self.lib.mrl_last_error().decode()
        assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_update" in message, (rc, message)
        return message


def test_refusals(hip_lib):
    for name in ("shape", "opt", "batch", "indices", "cfg", "workspace"):
        Call(hip_lib).refused(**{name: True})
    for field in ("params_dev", "exp_avg", "exp_avg_sq"):
        call = Call(hip_lib)
        setattr(call.opt, field, None)
        call.refused()
    for field in ("obs", "actions", "logprobs", "advantages", "returns", "values"):
        call = Call(hip_lib)
        setattr(call.batch, field, None)
        call.refused()
    call = Call(hip_lib)
    call.shape.hidden = 32
    assert "hidden" in call.refused()
    call = Call(hip_lib)
    call.shape.obs_dim = 5
    call.refused()
    call = Call(hip_lib)
    call.shape.obs_dim, call.shape.num_actions = 6, 2
    call.refused()
    call = Call(hip_lib)
    call.width = 1
    assert "minibatch_size" in call.refused()
    call = Call(hip_lib)
    call.width = 0
    call.refused()
    call = Call(hip_lib)
    call.batch.size = 0
    call.refused()
    call = Call(hip_lib)
    call.workspace_bytes = workspace_bytes(hip_lib, call.width)[1] - 1
    assert "workspace" in call.refused()
    call = Call(hip_lib)
    call.batch.obs = 4096 + 8
    assert "boundary" in call.refused()
    # B = 1 is a shape the call accepts without MRL_PPO_NORM_ADV: with these dummy addresses it must get past the checks
    # only as far as the next one that fails
    call = Call(hip_lib)
    call.width, call.cfg.flags, call.workspace_bytes = 1, 0, 0
    assert "workspace" in call.refused()


def test_workspace_bytes(hip_lib):
    sizes = [1, 2, 63, 64, 65, 257, 2049, 1 << 16, 1 << 20, 1 << 24, 1 << 28, (1 << 31) - 1, (1 << 31), (1 << 32) - 1]
    got = []
    for width in sizes:
        rc, value = workspace_bytes(hip_lib, width)
        assert rc == _lib.MRL_OK and value > 0
        got.append(value)
    assert got == sorted(got)
    assert got[sizes.index(1 << 28)] == got[-1] < 64 << 20, "the number of partial vectors must not grow with B beyond a cap"
    assert workspace_bytes(hip_lib, 257, 16)[1] >= workspace_bytes(hip_lib, 257, 1)[1]
    for shape in ((4, 32, 2), (5, 64, 2), (6, 64, 2), (4, 64, 4)):
        assert workspace_bytes(hip_lib, 64, 1, shape)[0] == _lib.MRL_ERR_INVALID
        assert "mrl_ppo_workspace_bytes" in hip_lib.mrl_last_error().decode()
    assert workspace_bytes(hip_lib, 0)[0] == _lib.MRL_ERR_INVALID
    assert hip_lib.mrl_ppo_workspace_bytes(4, 64, 2, 64, 1, None) == _lib.MRL_ERR_INVALID
    tile = twin.tile_size(lambda width: workspace_bytes(hip_lib, width)[1])
    assert 2 <= tile <= 1024
    # non-decreasing also where the workgroups start to take several tiles each and their number drops below the cap
    saturation = twin.saturation(lambda width: workspace_bytes(hip_lib, width)[1])
    assert saturation % tile == 0
    dense = [workspace_bytes(hip_lib, width)[1] for width in range(saturation - 2 * tile, 3 * saturation + 2 * tile, tile // 2 + 1)]
    assert dense == sorted(dense) and dense[-1] == got[-1]


def all_cases(hip_lib):
    size = lambda width: workspace_bytes(hip_lib, width)[1]  # noqa: E731
    tile = twin.tile_size(size)
    return twin.gpu_cases(tile) + twin.large_cases(tile, twin.saturation(size))


def test_branch_conditions_of_every_gpu_case(hip_lib):
    """Every parity case: no sample within 1e-5 of a kink in the twin, and (B >= 63) at least 10 % of the samples on each of
    the three branches and on each complement."""
    for case in all_cases(hip_lib) + twin.ADAM_CASES:
        fixed = twin.fixed_case(case)
        assert fixed["twin"]["kink"] > twin.KINK, (case, fixed["twin"]["kink"])
        if case[3] >= 63:
            for name, share in fixed["twin"]["branches"].items():
                assert 0.1 <= share <= 0.9, (case, name, share)


def test_twin_against_the_trainers_lines_in_float32(hip_lib):
    """d of every case and kind is small against the numbers themselves, and the float64 twin is the same computation as the
    float32 one (their clipfrac is the same count)."""
    worst = 0.0
    for case in all_cases(hip_lib):
        fixed = twin.fixed_case(case)
        d = twin.row_margins(fixed["twin"], fixed["f32"])
        largest = float(np.abs(fixed["twin"]["grad"]).max())
        assert 0.0 < d["grad"] < 1e-5 * largest, (case, d["grad"], largest)
        assert d["clipfrac"] == 0.0
        for name in twin.STATS:
            assert d[name] <= 1e-5 * max(1.0, abs(fixed["twin"]["stats"][name])), (case, name, d[name])
        worst = max(worst, d["grad"] / largest)
    print(f"largest d(grad) / largest component: {worst:.2e}")


@pytest.mark.parametrize("step", [0, 999])
@pytest.mark.parametrize("max_grad_norm", [0.5, 1e6, 0.0])
def test_twin_clip_and_adam_against_torch(step, max_grad_norm):
    fixed = twin.fixed_case(twin.ADAM_CASES[0])
    cfg = twin.Config(max_grad_norm=max_grad_norm, norm_adv=False)
    grad = fixed["twin"]["grad"]
    m, v = twin.moments(grad.size, 5) if step else (np.zeros(grad.size), np.zeros(grad.size))
    mine = twin.clip_adam(fixed["params"], m, v, grad, step, cfg)
    theirs = twin.clip_adam_torch(fixed["params"], m, v, grad, step, cfg, torch.float64)
    assert (mine[0] > 0.5) and abs(mine[0] - theirs[0]) < 1e-12
    for a, b, what in zip(mine[1:], theirs[1:], ("params", "exp_avg", "exp_avg_sq")):
        assert twin.distance(a, b) < 1e-12, what
    # d of the Adam parity test exists and is of float32's size
    single = twin.clip_adam_torch(fixed["params"], m, v, grad.astype(np.float32), step, cfg, torch.float32)
    assert 0.0 < twin.distance(single[1], mine[1]) < 1e-6


def test_minibatch_indices():
    g = torch.Generator().manual_seed(11)
    rows = minibatch_indices(4096, 4, 3, generator=g)
    assert rows.dtype == torch.int32 and tuple(rows.shape) == (12, 1024) and rows.device.type == "cpu"
    for epoch in range(3):
        assert sorted(rows[4 * epoch:4 * epoch + 4].reshape(-1).tolist()) == list(range(4096))
    assert not torch.equal(rows[:4], rows[4:8])
    again = minibatch_indices(4096, 4, 3, generator=torch.Generator().manual_seed(11))
    assert torch.equal(rows, again)
    assert tuple(minibatch_indices(8, 2, 0).shape) == (0, 4)
    with pytest.raises(ValueError):
        minibatch_indices(10, 4, 1)


def test_optimizer_and_value_errors(hip_lib):
    policy = MlpPolicy(4, 2, device="cpu")
    optimizer = PpoOptimizer(policy)
    assert optimizer.step == 0 and optimizer.lr == 2.5e-4 and optimizer.betas == (0.9, 0.999) and optimizer.eps == 1e-5
    assert optimizer.exp_avg.shape == policy.params.shape == optimizer.exp_avg_sq.shape
    assert optimizer.exp_avg.device == policy.params.device and not optimizer.exp_avg.any()
    optimizer.lr = 1e-4
    assert optimizer.lr == 1e-4
    assert optimizer.workspace_bytes(257, 16) == workspace_bytes(hip_lib, 257, 16)[1]
    first = optimizer.workspace(257, 16)
    assert first.numel() >= optimizer.workspace_bytes(257, 16) and optimizer.workspace(63, 1) is first
    with pytest.raises(ValueError):
        PpoOptimizer(object())
    n = 8
    rollout = Rollout(torch.zeros(1, n, 4), torch.zeros(1, n, dtype=torch.int32), *[torch.zeros(1, n) for _ in range(4)],
                      torch.zeros(n, 4), torch.zeros(n), torch.zeros(n))
    indices = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="policy.params"):
        ppo_update(policy, optimizer, rollout, torch.zeros(1, n), torch.zeros(1, n), indices)
    with pytest.raises(ValueError):
        ppo_update(policy, PpoOptimizer(MlpPolicy(4, 2, device="cpu")), rollout, torch.zeros(1, n), torch.zeros(1, n), indices)
    assert optimizer.step == 0


def chain_cases():
    return [(d, a, 1.0, width, "default") for d, a in twin.SHAPES for width in twin.CHAIN_SIZES]


def test_rehearsal_of_the_chained_rows():
    """The chained GPU test with torch's float32 lines, clip_grad_norm_ and Adam in the device's place: over the six rows of
    every chain case the twin, fed the pre-row parameters, finds at most one row with a sample within 1e-5 of a kink, and the
    float32 gradient of every other row is within float32's reach of the twin's."""
    for case in chain_cases():
        fixed = twin.fixed_case(case, twin.CHAIN_ROWS)
        cfg = fixed["cfg"]
        params = fixed["params"].astype(np.float32)
        m, v = np.zeros_like(params), np.zeros_like(params)
        skipped = 0
        for k in range(twin.CHAIN_ROWS):
            exact = twin.row(params, fixed["batch"], fixed["indices"][k], cfg)
            single = twin.row(params, fixed["batch"], fixed["indices"][k], cfg, torch.float32)
            if exact["kink"] <= twin.KINK:
                skipped += 1
            else:
                assert twin.distance(exact["grad"], single["grad"]) < 1e-5 * np.abs(exact["grad"]).max(), (case, k)
            _, p, m, v = twin.clip_adam_torch(params, m, v, single["grad"].astype(np.float32), k, cfg, torch.float32)
            params, m, v = p.astype(np.float32), m.astype(np.float32), v.astype(np.float32)
        print(f"{case}: {skipped} of {twin.CHAIN_ROWS} rows skipped")
        assert skipped <= twin.CHAIN_MAX_SKIPPED, case
