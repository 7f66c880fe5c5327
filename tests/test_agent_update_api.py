"""No GPU: the surface of ``mrl_agent_update`` -- symbols, struct sizes, refusals, the workspace formula --, the float64 twin of
tests/wide_update_twin.py against ``torch.optim.Adam`` and ``clip_grad_norm_`` on a ``WideAgent``, the input conditions of every
batch the GPU tests run, and the exact-integer construction's bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import wide_twin
import wide_update_twin as twin
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent
from madrona_rl_envs_playground_amd.simulators import WideOptimizer, WidePolicy, agent_update

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mrl_agent_update_workspace_bytes", "mrl_agent_update")


def workspace_bytes(lib, capacity, shape=(187, 212, 16)):
    out = ctypes.c_uint64(0)
    rc = lib.mrl_agent_update_workspace_bytes(shape[0], shape[1], shape[2], capacity, ctypes.byref(out))
    return rc, out.value


def test_symbols_structs_and_abi(hip_lib):
    header = open(os.path.join(REPO, "include", "mrl_envs.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
        assert name in _lib.SYMBOLS
        assert hasattr(hip_lib, name)
    assert hip_lib.mrl_abi_version() == 4 == _lib.ABI_VERSION
    assert "#define MRL_ABI_VERSION 4" in header
    # the structs the call takes keep their layouts
    assert ctypes.sizeof(_lib.AgentRecord) == 18 * 8 + 8 and ctypes.sizeof(_lib.WidePolicyDesc) == 24
    assert ctypes.sizeof(_lib.PpoConfig) == 36 and ctypes.sizeof(_lib.PpoOptimizerDesc) == 32
    assert _lib.AGENT_UPDATE_STATS == _lib.PPO_STATS + ("samples", "status")


class Call:
    """A well-formed argument list of mrl_agent_update over dummy non-NULL addresses (nothing is dereferenced before the
    refusals under test), one piece of which a test breaks.  The workspace is a byte short, so that a call that gets past every
    other check is still refused."""

    def __init__(self, lib):
        self.lib = lib
        self.policy = _lib.WidePolicyDesc(4096, 187, 212, 16)
        self.opt = _lib.PpoOptimizerDesc(4096, 4096, 4096, 0)
        self.record = _lib.AgentRecord(*([4096] * 18), 8, 33)
        self.cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, _lib.PPO_NORM_ADV | _lib.PPO_CLIP_VLOSS)
        self.types = [_lib.MRL_INT8, _lib.MRL_INT8]
        self.advantages, self.returns, self.stats, self.grads = 4096, 4096, 4096, 4096
        self.epochs, self.capacity, self.workspace = 1, 8 * 33, 4096
        self.workspace_bytes = None

    def refused(self, **null):
        ref = lambda name, value: None if null.get(name) else ctypes.byref(value)  # noqa: E731
        val = lambda name, value: None if null.get(name) else value  # noqa: E731
        size = self.workspace_bytes
        if size is None:
            size = workspace_bytes(self.lib, max(self.capacity, 1), (self.policy.obs_dim or 1, self.policy.state_dim or 1, 16))[1] - 1
        rc = self.lib.mrl_agent_update(ref("policy", self.policy), ref("opt", self.opt), ref("record", self.record), self.types[0],
                                       self.types[1], val("advantages", self.advantages), val("returns", self.returns), self.epochs,
                                       ref("cfg", self.cfg), self.capacity, val("workspace", self.workspace), size, self.stats,
                                       self.grads, 0, None)
        message = self.lib.mrl_last_error().decode()
        assert rc == _lib.MRL_ERR_INVALID and message.startswith("mrl_agent_update:"), (rc, message)
        return message


def test_refusals(hip_lib):
    assert "workspace of" in Call(hip_lib).refused()  # the well-formed list gets as far as the short workspace
    for name in ("policy", "opt", "record", "cfg", "advantages", "returns", "workspace"):
        assert "null" in Call(hip_lib).refused(**{name: True})
    for field in ("params_dev", "exp_avg", "exp_avg_sq"):
        call = Call(hip_lib)
        setattr(call.opt, field, None)
        assert "null" in call.refused()
    for field in ("obs", "states", "action_masks", "active", "actions", "logprobs", "values"):
        call = Call(hip_lib)
        setattr(call.record, field, None)
        assert "null" in call.refused()
    for field in ("dones", "rewards", "totals", "logits", "next_value"):  # what the update does not read may be absent
        call = Call(hip_lib)
        setattr(call.record, field, None)
        assert "workspace of" in call.refused()
    for field, value in (("num_actions", 0), ("num_actions", 65), ("obs_dim", 0), ("state_dim", 0)):
        call = Call(hip_lib)
        setattr(call.policy, field, value)
        assert "num_actions" in call.refused()
    for capacity in (0, 8 * 33 + 1):
        call = Call(hip_lib)
        call.capacity = capacity
        assert "capacity" in call.refused()
    call = Call(hip_lib)
    call.capacity = 1  # anything from 1 to T N is a capacity
    assert "workspace of" in call.refused()
    call = Call(hip_lib)
    call.record.num_steps, call.record.num_worlds, call.capacity = 1 << 12, 1 << 12, 64
    assert "2^24" in call.refused()
    call = Call(hip_lib)
    call.workspace, call.workspace_bytes = 4096 + 8, 1 << 40
    assert "16-byte" in call.refused()
    for name in ("advantages", "returns", "stats", "grads"):
        call = Call(hip_lib)
        setattr(call, name, 4096 + 2)
        call.workspace_bytes = 1 << 40
        assert "4-byte" in call.refused()
    for field in ("logprobs", "values", "actions"):
        call = Call(hip_lib)
        setattr(call.record, field, 4096 + 2)
        call.workspace_bytes = 1 << 40
        assert "4-byte" in call.refused()
    call = Call(hip_lib)
    call.record.obs, call.workspace_bytes = 4096 + 1, None  # int8 rows start anywhere ...
    assert "workspace of" in call.refused()
    call.types[0], call.workspace_bytes = _lib.MRL_INT32, 1 << 40  # ... int32 rows on a 4-byte boundary
    assert "4-byte" in call.refused()
    call = Call(hip_lib)
    call.cfg.flags |= 4
    assert "flag" in call.refused()
    for types in ([5, _lib.MRL_INT8], [_lib.MRL_INT8, 7]):
        call = Call(hip_lib)
        call.types = types
        assert "element types" in call.refused()
    # epochs == 0 is refused like any other call where its arguments are wrong
    call = Call(hip_lib)
    call.epochs = 0
    assert "workspace of" in call.refused()


def test_workspace_formula(hip_lib):
    pad = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for shape in ((7, 7, 4), (187, 212, 16), (658, 783, 20)):
        d, s, a = shape
        params = int(hip_lib.mrl_wide_policy_num_params(d, s, a))
        for n in (1, 2, 33, 64, 65, 256, 257, 1285, 65536):
            want = (pad(4 * n) + 256) + 2 * 6 * 2048 * n + 2 * 256 * n + 2 * pad(4 * n) + 256 + pad(64 * ((n + 255) // 256)) + \
                2 * pad(4 * params) + pad(4 * ((params + 255) // 256))
            assert workspace_bytes(hip_lib, n, shape) == (_lib.MRL_OK, want)
    assert 24000 < (workspace_bytes(hip_lib, 65536)[1] - workspace_bytes(hip_lib, 32768)[1]) / 32768 < 26000  # about 25 KB a sample
    for shape in ((0, 7, 4), (7, 0, 4), (7, 7, 0), (7, 7, 65)):
        assert workspace_bytes(hip_lib, 64, shape)[0] == _lib.MRL_ERR_INVALID
        assert hip_lib.mrl_last_error().decode().startswith("mrl_agent_update_workspace_bytes:")
    assert workspace_bytes(hip_lib, 0)[0] == _lib.MRL_ERR_INVALID and workspace_bytes(hip_lib, 1 << 24)[0] == _lib.MRL_ERR_INVALID
    assert hip_lib.mrl_agent_update_workspace_bytes(7, 7, 4, 64, None) == _lib.MRL_ERR_INVALID


def test_twin_against_torch_adam_over_three_epochs():
    """The twin's float64 epoch, ``update_twin.clip_adam`` between epochs, against ``loss.backward()``, ``clip_grad_norm_`` and
    ``torch.optim.Adam`` on a float64 ``WideAgent``, to 1e-12."""
    game, weights, size = "hanabi_very_small", "peaked", 65
    batch = twin.make_batch(game, weights, size)
    cfg = twin.config(lr=1e-3)
    d, s, a = wide_twin.dims(game)
    agent = twin.agent_from(batch["params"], d, s, a, torch.float64)
    optimizer = torch.optim.Adam(agent.parameters(), lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).double()  # noqa: E731
    p, m, v = batch["params"].astype(np.float64), np.zeros(len(batch["params"])), np.zeros(len(batch["params"]))
    for k in range(3):
        _, newlogprob, entropy, newvalue = agent.get_action_and_value(t(batch["obs"]), t(batch["state"]), torch.from_numpy(batch["mask"] != 0),
                                                                      torch.from_numpy(batch["actions"]).long())
        ratio = (newlogprob - t(batch["logprobs"])).exp()
        adv = t(batch["advantages"])
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
        pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - cfg.clip_coef, 1 + cfg.clip_coef)).mean()
        newvalue = newvalue.view(-1)
        clipped = t(batch["values"]) + torch.clamp(newvalue - t(batch["values"]), -cfg.clip_coef, cfg.clip_coef)
        v_loss = 0.5 * torch.max((newvalue - t(batch["returns"])) ** 2, (clipped - t(batch["returns"])) ** 2).mean()
        loss = pg_loss - cfg.ent_coef * entropy.mean() + v_loss * cfg.vf_coef
        optimizer.zero_grad()
        loss.backward()
        grad = torch.cat([q.grad.reshape(-1) for q in agent.parameters()]).numpy().copy()
        total = float(torch.nn.utils.clip_grad_norm_(agent.parameters(), cfg.max_grad_norm))
        optimizer.step()
        mine = twin.epoch(p, batch, cfg, torch.float64)
        assert twin.distance(mine["grad"], grad) <= 1e-12 and abs(mine["stats"]["loss"] - float(loss.detach())) <= 1e-12
        norm, p, m, v = twin.step(p, m, v, mine["grad"], k, cfg)
        assert abs(norm - total) <= 1e-12 and norm > cfg.max_grad_norm  # (the clip acts)
        assert twin.distance(p, torch.nn.utils.parameters_to_vector(agent.parameters()).detach().numpy()) <= 1e-12


def gpu_batches():
    for weights in sorted(wide_twin.WEIGHTS):
        for game, size in twin.CASES:
            yield game, weights, size


@pytest.mark.parametrize("game,weights,size", list(gpu_batches()))
def test_input_conditions_of_every_gpu_batch(game, weights, size):
    """Asserted on the very samples the GPU cases use.  ReLU kinks: no hidden pre-activation of any sample is closer to 0 than 8 x
    the largest float32-vs-twin pre-activation distance of the batch, unless it is exactly 0 in both.  Loss kinks: no sample
    within 1e-5 of |ratio - 1| = clip, |v - v_old| = clip or equal branches of either max (inside the clip range the branches are
    equal by construction and carry the same gradient: no kink); a quarter at least of the samples is ratio-clipped and a quarter
    value-clipped.  The filter dropped at most 15 % of the candidates."""
    batch = twin.make_batch(game, weights, size)
    cfg = twin.config()
    assert len(batch["actions"]) == size and batch["mask"][np.arange(size), batch["actions"]].all()
    checks = twin.sample_checks(batch["params"], batch, cfg)
    window = twin.FACTOR * checks["pre_d"].max()
    assert window > 0 and checks["relu_gap"].min() >= window
    assert checks["loss_gap"].min() >= twin.KINK
    assert batch["dropped"] <= 0.15
    c = cfg.clip_coef
    assert (np.abs(checks["ratio"] - 1) > c).mean() >= 0.25 and (np.abs(checks["moved"]) > c).mean() >= 0.25
    # the policy loss's branches, which depend on the batch through the normalised advantages: with and without NORM_ADV
    for flags in ((), (("norm_adv", False),)):
        exact = twin.parity(game, weights, size, flags)[1]
        outside = np.abs(exact["ratio"] - 1) > c
        gap = np.abs(exact["adv"] * (exact["ratio"] - np.clip(exact["ratio"], 1 - c, 1 + c)))
        assert (gap[outside] >= twin.KINK).all()


def test_records_place_the_samples_in_ascending_cells():
    batch = twin.make_batch("balance", "orthogonal", 33)
    steps, n = twin.record_shape(33)
    rec = twin.make_record(batch, steps, n, batch["seed"])
    cells = np.flatnonzero(rec["active"].reshape(-1))
    assert len(cells) == 33 < steps * n and (np.diff(cells) > 0).all() and steps in (4, 5)
    for name, key in (("obs", "obs"), ("states", "state"), ("action_masks", "mask"), ("actions", "actions"), ("returns", "returns")):
        flat = rec[name].reshape((steps * n,) + rec[name].shape[2:])
        assert np.array_equal(flat[cells], batch[key]) and flat.dtype == batch[key].dtype
    # an inactive cell does not hold the data of the sample a wrong gather would most likely take for it
    inactive = np.flatnonzero(rec["active"].reshape(-1) == 0)
    assert len(inactive) and not np.array_equal(rec["returns"].reshape(-1)[inactive[:1]], batch["returns"][:1])


@pytest.mark.parametrize("size", [32, 64])
def test_integer_construction_stays_exact(size):
    """Every sum of absolute terms of the critic's forward and backward pass stays under 2^24 (in units of 1 / B, B a power of
    two): float32 holds every partial sum exactly, in any order."""
    params, rec, expected, bound = twin.integer_case(size)
    assert bound < 2 ** 24 and size & (size - 1) == 0
    assert np.array_equal(params, np.round(params)) and np.array_equal(expected * size, np.round(expected * size))
    assert np.array_equal(expected.astype(np.float32).astype(np.float64), expected)
    # the gradient reaches every layer and is not symmetric in rows and columns
    s = rec["states"].shape[2]
    w1 = expected[:512 * s].reshape(512, s)
    assert np.count_nonzero(w1) > w1.size // 8 and not np.array_equal(w1[:s, :s], w1[:s, :s].T)
    assert np.count_nonzero(expected[512 * s + 512:512 * s + 512 + 512 * 512]) > 1000


def test_python_layer_value_errors():
    policy = WidePolicy.__new__(WidePolicy)  # (no device here: the checks in front of the call)
    with pytest.raises(ValueError, match="WidePolicy"):
        WideOptimizer(object())
    with pytest.raises(ValueError, match="WideOptimizer"):
        agent_update(policy, object(), None)
    import inspect
    assert isinstance(CleanPPOAgent.device_update, property) and CleanPPOAgent.device_update.fset is not None
    assert "device_update" not in inspect.signature(CleanPPOAgent.__init__).parameters  # the constructor keeps the reference's signature
    assert list(inspect.signature(agent_update).parameters)[:5] == ["policy", "optimizer", "record", "advantages", "returns"]
