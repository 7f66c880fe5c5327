"""No GPU: the surface of ``mrl_mappo_update`` -- symbols, struct sizes, refusals, the workspace size --, ``ValueNorm`` against the
reference's formulas, the float64 twin of tests/mappo_twin.py against torch's own float64, ``huber_loss``'s one-sided quirk, the
input conditions of every case the GPU tests run, and the Python layer's ValueErrors that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import cnn_twin
import mappo_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnRecord, MappoOptimizer, MlpPolicy, ValueNorm, mappo_advantages,
                                                         mappo_update)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mrl_mappo_workspace_bytes", "mrl_mappo_update")


def workspace_bytes(lib, width, rows=1, shape=(5, 4, 26, 64)):
    out = ctypes.c_uint64(0)
    rc = lib.mrl_mappo_workspace_bytes(shape[0], shape[1], shape[2], shape[3], width, rows, ctypes.byref(out))
    return rc, out.value


def test_symbols_and_struct_sizes(hip_lib):
    header = open(os.path.join(REPO, "include", "mrl_envs.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.mrl_abi_version() == 4 == _lib.ABI_VERSION
    assert "#define MRL_ABI_VERSION 4" in header
    # as a C compiler lays them out: 13 floats and a word; a pointer, five words and padding; six pointers and a word; three and a word
    assert ctypes.sizeof(_lib.MappoConfig) == 56 and ctypes.sizeof(_lib.MappoPolicyDesc) == 32
    assert ctypes.sizeof(_lib.MappoBatch) == 56 and ctypes.sizeof(_lib.MappoOptimizerDesc) == 32
    assert (_lib.MAPPO_VALUENORM, _lib.MAPPO_HUBER_LOSS, _lib.MAPPO_CLIPPED_VALUE_LOSS, _lib.MAPPO_MAX_GRAD_NORM) == (1, 2, 4, 8)
    for name, value in (("VALUENORM", 1), ("HUBER_LOSS", 2), ("CLIPPED_VALUE_LOSS", 4), ("MAX_GRAD_NORM", 8)):
        assert re.search(r"MRL_MAPPO_%s = %d\b" % (name, value), header)
    assert len(_lib.MAPPO_STATS) == 8


class Call:
    """A well-formed argument list of mrl_mappo_update over dummy non-NULL addresses (nothing is dereferenced before the
    refusals under test), one piece of which a test breaks."""

    def __init__(self, lib):
        self.lib = lib
        self.policy = _lib.MappoPolicyDesc(4096, 64, 0, 5, 4, 26)
        self.opt = _lib.MappoOptimizerDesc(4096, 8192, 8192, 0)
        self.batch = _lib.MappoBatch(4096, 4096, 4096, 4096, 4096, 4096, 128)
        self.cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 15)
        self.indices, self.rows, self.width, self.state, self.workspace, self.workspace_bytes = 4096, 1, 64, 4096, 4096, 1 << 40

    def refused(self, **null):
        ref = lambda name, value: None if null.get(name) else ctypes.byref(value)  # noqa: E731
        rc = self.lib.mrl_mappo_update(ref("policy", self.policy), ref("opt", self.opt), ref("batch", self.batch),
                                       None if null.get("indices") else self.indices, self.rows, self.width, ref("cfg", self.cfg),
                                       None if null.get("state") else self.state, None if null.get("workspace") else self.workspace,
                                       self.workspace_bytes, None, None, 0, None)
        message = self.lib.mrl_last_error().decode()
        assert rc == _lib.MRL_ERR_INVALID and "mrl_mappo_update" in message, (rc, message)
        return message


def test_refusals(hip_lib):
    for name in ("policy", "opt", "batch", "indices", "cfg", "workspace"):
        Call(hip_lib).refused(**{name: True})
    assert "value_norm_state" in Call(hip_lib).refused(state=True)
    for field in ("params_dev", "exp_avg", "exp_avg_sq"):
        call = Call(hip_lib)
        setattr(call.opt, field, None)
        call.refused()
    for field in ("obs", "actions", "logprobs", "value_preds", "returns", "advantages"):
        call = Call(hip_lib)
        setattr(call.batch, field, None)
        call.refused()
    call = Call(hip_lib)
    call.policy.params_dev = 8192
    assert "same array" in call.refused()
    call = Call(hip_lib)
    call.policy.hidden = 32
    assert "hidden" in call.refused()
    call = Call(hip_lib)
    call.policy.width = 2
    assert "3 x 3" in call.refused()
    call = Call(hip_lib)
    call.policy.width, call.policy.height = 12, 5  # the LDS image of a 12 x 5 kitchen does not fit
    assert "LDS" in call.refused()
    call = Call(hip_lib)
    call.width = 0
    assert "minibatch_size" in call.refused()
    call = Call(hip_lib)
    call.batch.size = 0
    assert "sample" in call.refused()
    call = Call(hip_lib)
    call.cfg.flags = 16
    assert "flags" in call.refused()
    call = Call(hip_lib)
    call.workspace_bytes = workspace_bytes(hip_lib, call.width)[1] - 1
    assert "workspace" in call.refused()
    call = Call(hip_lib)
    call.workspace = 4096 + 8
    assert "boundar" in call.refused()
    call = Call(hip_lib)
    call.batch.returns = 4096 + 2
    assert "boundar" in call.refused()
    # an observation block may start anywhere: with these dummy addresses the call must get as far as the next check that fails
    call = Call(hip_lib)
    call.batch.obs, call.workspace_bytes = 4096 + 1, 0
    assert "workspace" in call.refused()


def test_workspace_bytes(hip_lib):
    sizes = [1, 2, 31, 32, 33, 65, 257, 2049, 1 << 13, 1 << 16, 1 << 20, 1 << 28, (1 << 31) - 1, (1 << 32) - 1]
    got = []
    for width in sizes:
        rc, value = workspace_bytes(hip_lib, width)
        assert rc == _lib.MRL_OK and value > 0
        got.append(value)
    assert got == sorted(got)
    assert got[sizes.index(1)] == got[sizes.index(32)] < got[sizes.index(33)], "one partial vector per net up to a tile of 32"
    assert got[sizes.index(1 << 13)] == got[-1] < 64 << 20, "the number of partial vectors must not grow with B beyond a cap"
    assert twin.saturation(lambda width: workspace_bytes(hip_lib, width)[1]) == (32, 256 * 32)
    assert workspace_bytes(hip_lib, 257, 16)[1] >= workspace_bytes(hip_lib, 257, 1)[1]
    assert workspace_bytes(hip_lib, 257, 1, (9, 5, 26, 64))[1] > workspace_bytes(hip_lib, 257, 1)[1]
    for shape in ((5, 4, 26, 32), (2, 4, 26, 64), (5, 2, 26, 64), (5, 4, 0, 64), (12, 5, 26, 64)):
        assert workspace_bytes(hip_lib, 64, 1, shape)[0] == _lib.MRL_ERR_INVALID, shape
    assert workspace_bytes(hip_lib, 0)[0] == _lib.MRL_ERR_INVALID
    assert hip_lib.mrl_mappo_workspace_bytes(5, 4, 26, 64, 64, 1, None) == _lib.MRL_ERR_INVALID
    # every standard layout fits
    for layout in ("cramped_room", "asymmetric_advantages", "coordination_ring", "forced_coordination", "counter_circuit"):
        w, h, _, f = twin.shape_of(layout)
        assert workspace_bytes(hip_lib, 64, 1, (w, h, f, 64))[0] == _lib.MRL_OK, layout


def test_python_value_errors_without_a_gpu(hip_lib):
    policy = CnnPolicy(5, 4, 26, device="cpu")
    optimizer = MappoOptimizer(policy)
    assert optimizer.step == 0 and optimizer.lr == optimizer.critic_lr == 5e-4 and optimizer.exp_avg.shape == policy.params.shape
    optimizer.lr, optimizer.critic_lr = 1e-4, 2e-4  # assignable, for lr_decay
    assert optimizer.workspace_bytes(64, 2) == workspace_bytes(hip_lib, 64, 2)[1]
    with pytest.raises(ValueError):
        MappoOptimizer(MlpPolicy(4, 2, device="cpu"))
    record = CnnRecord(2, 3, 2, "cpu")
    ring = torch.zeros((3, 3, 2, 4, 5, 26), dtype=torch.int8)
    zeros = torch.zeros(2, 3, 2)
    indices = torch.zeros((1, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        mappo_update(policy, optimizer, record, ring, zeros, zeros, indices)  # CPU parameters
    with pytest.raises(ValueError, match="MappoOptimizer"):
        mappo_update(policy, MappoOptimizer(CnnPolicy(5, 4, 26, device="cpu")), record, ring, zeros, zeros, indices)
    with pytest.raises(ValueError, match="CnnRecord"):
        mappo_update(policy, optimizer, object(), ring, zeros, zeros, indices)
    with pytest.raises(ValueError, match="ValueNorm"):
        mappo_update(policy, optimizer, record, ring, zeros, zeros, indices, value_norm=3)
    with pytest.raises(ValueError, match="CnnRecord"):
        mappo_advantages(object())
    assert optimizer.step == 0


def test_value_norm_is_the_references_over_ten_chained_updates():
    """utils/valuenorm.py:34-87 restated with torch float32 tensors, as the reference holds them"""
    rng = np.random.default_rng(7)
    ours = ValueNorm("cpu")
    mean, mean_sq, debias, beta, eps = torch.zeros(()), torch.zeros(()), torch.tensor(0.0), 0.99999, 1e-5
    x = torch.from_numpy(rng.normal(3.0, 2.0, size=50).astype(np.float32))
    for k in range(10):
        batch = torch.from_numpy(rng.normal(3.0 + k, 2.0, size=(64, 1)).astype(np.float32))
        mean.mul_(beta).add_(batch.mean(dim=0)[0] * (1.0 - beta))
        mean_sq.mul_(beta).add_((batch ** 2).mean(dim=0)[0] * (1.0 - beta))
        debias.mul_(beta).add_(1.0 * (1.0 - beta))
        ours.update(batch)
        assert torch.equal(ours.state, torch.stack([mean, mean_sq, debias]))
        m = mean / debias.clamp(min=eps)
        var = (mean_sq / debias.clamp(min=eps) - m ** 2).clamp(min=1e-2)
        got_mean, got_var = ours.running_mean_var()
        assert torch.equal(got_mean, m) and torch.equal(got_var, var)
        assert torch.equal(ours.normalize(x), (x - m) / torch.sqrt(var))
        assert torch.equal(ours.denormalize(x), x * torch.sqrt(var) + m)
        # and the twin's float32 recurrence, which is the device's: the same numbers
        cfg = twin.Config()
        state = np.zeros(3, np.float32) if k == 0 else state  # noqa: F821
        state, tm, ts = twin.value_norm_update(state, batch.numpy().reshape(-1), cfg, np.float32)
        assert np.allclose(state, ours.state.numpy(), rtol=3e-6, atol=0)
        assert abs(tm - float(m)) <= 4e-6 * abs(float(m)) and abs(ts - float(torch.sqrt(var))) <= 4e-6 * float(torch.sqrt(var))
    fresh = ValueNorm("cpu")
    assert fresh.running_mean_var()[1] == 1e-2 and torch.equal(fresh.denormalize(x), x * 0.1)


def test_huber_loss_is_the_references_below_minus_delta():
    e = torch.tensor([-3.0, -1.0 - 1e-6, -1.0, -0.5, 0.0, 0.5, 1.0, 1.0 + 1e-6, 3.0], dtype=torch.float64, requires_grad=True)
    loss = twin.huber_loss(e, 1.0)
    want = torch.tensor([0.0, 0.0, 0.5, 0.125, 0.0, 0.125, 0.5, 1.0 * (1.0 + 1e-6 - 0.5), 2.5], dtype=torch.float64)
    assert torch.allclose(loss, want, rtol=0, atol=1e-15)
    loss.sum().backward()
    assert torch.equal(e.grad, torch.tensor([0.0, 0.0, -1.0, -0.5, 0.0, 0.5, 1.0, 1.0, 1.0], dtype=torch.float64))
    # the reference's own lines
    ref = lambda e, d: (abs(e) <= d).float() * e ** 2 / 2 + (e > d).float() * d * (abs(e) - d / 2)  # noqa: E731
    x = torch.linspace(-4, 4, 101)
    assert torch.equal(twin.huber_loss(x, 1.5), ref(x, 1.5))


def reference_row(module, x, actions, old_logp, adv, old_v, target, cfg):
    """r_mappo.py:124-155 and :62-87 written out again with torch.distributions, on a module, in the module's dtype"""
    dist = torch.distributions.Categorical(logits=module.actor(x))
    action_log_probs, dist_entropy = dist.log_prob(actions), dist.entropy().mean()
    imp_weights = torch.exp(action_log_probs - old_logp)
    surr1 = imp_weights * adv
    surr2 = torch.clamp(imp_weights, 1.0 - cfg.clip_param, 1.0 + cfg.clip_param) * adv
    policy_loss = -torch.min(surr1, surr2).mean()
    values = module.critic(x).squeeze(1)
    value_pred_clipped = old_v + (values - old_v).clamp(-cfg.clip_param, cfg.clip_param)
    error_clipped, error_original = target - value_pred_clipped, target - values
    value_loss = torch.max(twin.huber_loss(error_original, cfg.huber_delta), twin.huber_loss(error_clipped, cfg.huber_delta)).mean()
    return policy_loss - dist_entropy * cfg.entropy_coef, value_loss * cfg.value_loss_coef


def test_the_twin_is_torchs_float64(hip_lib):
    case = ("cramped_room", twin.N, "trained", "synthetic", 65, "default")
    fixed = twin.fixed_case(case)
    cfg, batch, inds = fixed["cfg"], fixed["batch"], fixed["indices"][0].astype(np.int64)
    module = twin.module_from(fixed["params"], fixed["layout"], torch.float64)
    x = torch.from_numpy(np.array(batch.ring[inds])).transpose(1, 2).double()
    as64 = lambda a: torch.from_numpy(np.asarray(a)[inds]).double()  # noqa: E731
    _, mean, std = twin.value_norm_update(twin.STATE0, batch.returns[inds], cfg)
    actor_loss, critic_loss = reference_row(module, x, torch.from_numpy(batch.actions[inds]).long(), as64(batch.logprobs), as64(batch.advantages),
                                            as64(batch.values), (as64(batch.returns) - mean) / std, cfg)
    actor_loss.backward()
    critic_loss.backward()
    assert twin.distance(twin.flat_grad(module), fixed["twin"]["grad"]) <= 1e-12
    # clip_grad_norm_ and Adam, per net
    grad, params = fixed["twin"]["grad"], fixed["params"]
    m, v = twin.moments(params.size, 5)
    na = twin.actor_size(fixed["layout"])
    for limit in (1e-3, 1e3, None):
        for sl, lr in ((slice(0, na), 3e-4), (slice(na, None), 7e-4)):
            ours = twin.clip_adam(params[sl], m[sl], v[sl], grad[sl], 4, limit, lr, cfg)
            theirs = twin.clip_adam_torch(params[sl], m[sl], v[sl], grad[sl], 4, limit, lr, cfg)
            for a, b in zip(ours, theirs):
                assert twin.distance(a, b) <= 1e-12
    # the pre-activations the conditions read are the module's own
    with torch.no_grad():
        assert twin.distance(np.maximum(fixed["twin"]["pre"][5], 0) @ module.critic.v_out.weight.numpy().T + module.critic.v_out.bias.numpy(),
                             module.critic(x).numpy()) <= 1e-12


def all_cases(hip_lib):
    tile, size = twin.saturation(lambda width: workspace_bytes(hip_lib, width)[1])
    return list(twin.CASES) + twin.large_cases(tile, size)


def test_input_conditions_of_every_gpu_case(hip_lib):
    """conditions, not measurements: in the twin no sample lies within 1e-5 of a kink of the loss, no pre-activation is closer to
    0 than 8 x the largest float32-vs-twin pre-activation distance unless it is exactly 0 in both, and the batches put their
    samples on every branch"""
    for case in all_cases(hip_lib):
        fixed = twin.fixed_case(case)
        exact, width = fixed["twin"], case[4]
        assert exact["kink"] > twin.KINK, (case, exact["kink"])
        closest, worst = twin.relu_margin(fixed)
        assert closest > twin.FACTOR * worst, (case, closest, worst)
        assert (fixed["indices"] >= 0).all() and (fixed["indices"] < len(fixed["batch"].ring)).all()
        if width > len(fixed["batch"].ring):
            assert len(np.unique(fixed["indices"])) <= twin.DISTINCT
        if width < 24:
            continue
        b = exact["branches"]
        assert b["ratio_clipped"] >= 0.25 and b["value_clipped"] >= 0.25 and min(b["clipped_high"], b["clipped_low"]) >= 0.1, (case, b)
        assert min(b["huber_above"], b["huber_below"]) >= 0.05, (case, b)
    # rows that start off 4-byte boundaries: coordination_ring's are 650 bytes
    w, h, _, f = twin.shape_of("coordination_ring")
    assert (w * h * f) % 4 == 2


def test_integer_construction_is_exact():
    for layout in cnn_twin.INTEGER_LAYOUTS:
        case = twin.integer_case(layout)
        assert case["bound"] < 2 ** 24 and case["indices"].shape[1] == 64
        for name, matrix in case["matrices"].items():
            assert len(np.unique(matrix)) > 8 and (matrix.shape[0] != matrix.shape[1] or (matrix != matrix.T).sum() > 8), name
        # the integer gradient is the twin's float64 one
        cfg, batch, layout_params = case["cfg"], case["batch"], case["params"]
        exact = twin.row(layout_params, layout, batch, case["indices"][0], cfg)
        assert np.array_equal(exact["grad"][twin.actor_size(layout):], case["grad"].astype(np.float64))


def test_compute_returns_is_the_references_and_is_gae():
    """the twin's compute_returns against the reference's own lines (utils/shared_buffer.py:216-228 with a ValueNorm, written out
    again on torch float64 buffers whose masks[t + 1] is 1 - done after step t) and r_mappo.py:174-182; and mrl_gae's recurrence
    (``cnn_twin.gae32``) on the denormalised values is the same function"""
    rng = np.random.default_rng(3)
    t, cols, gamma, lam = 7, 5, 0.99, 0.95
    rewards = rng.integers(0, 3, size=(t, cols)).astype(np.float64) * 20
    value_preds = rng.normal(size=(t + 1, cols))
    done_after = (rng.uniform(size=(t + 1, cols)) < 0.3).astype(np.float64)  # done_after[k]: the flag in front of step k
    dones, next_done = done_after[:t], done_after[t]
    cfg = twin.Config()
    for state in (None, twin.STATE0, (0.0, 0.0, 0.0)):
        adv, ret = twin.compute_returns(rewards, value_preds, dones, next_done, gamma, lam, cfg, state)
        if state is None:
            denorm = lambda x: x  # noqa: E731
        else:
            mean, var = twin.running_mean_var(state, cfg)
            denorm = lambda x: x * np.sqrt(var) + mean  # noqa: E731
        masks = torch.ones(t + 1, cols, dtype=torch.float64)
        masks[1:] = torch.from_numpy(1.0 - done_after[1:])  # buffer.insert stores the masks of step k at k + 1
        r, vp = torch.from_numpy(rewards), torch.from_numpy(value_preds)
        returns, gae = torch.zeros(t + 1, cols, dtype=torch.float64), 0
        for step in reversed(range(t)):
            delta = r[step] + gamma * denorm(vp[step + 1]) * masks[step + 1] - denorm(vp[step])
            gae = delta + gamma * lam * masks[step + 1] * gae
            returns[step] = gae + denorm(vp[step])
        advantages = returns[:-1] - denorm(vp[:-1])
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-5)
        assert twin.distance(ret, returns[:-1].numpy()) <= 1e-12 and twin.distance(adv, advantages.numpy()) <= 1e-12
        # mrl_gae's recurrence (float32) on the denormalised values
        dv = denorm(value_preds)
        a32, r32 = cnn_twin.gae32(rewards, dv[:t], dones, dv[t], next_done, gamma, lam)
        assert twin.distance(r32, ret) <= 1e-4 * max(1.0, float(np.abs(ret).max()))
        raw = ret - dv[:t]
        assert twin.distance(a32, raw) <= 1e-4 * max(1.0, float(np.abs(raw).max()))
    # a finished world takes nothing across the boundary: with done in front of step k + 1, row k's return is its reward alone
    k, c = np.argwhere(done_after[1:] == 1)[0]
    _, ret = twin.compute_returns(rewards, value_preds, dones, next_done, gamma, lam, cfg, None)
    assert abs(ret[k, c] - rewards[k, c]) <= 1e-12
