"""GPU: ``ppo_update`` (mrl_ppo_update: gradient, reduce, clip + Adam) against the float64 twin of tests/ppo_twin.py.

Shapes (D, A) = (4, 2), (4, 3), (6, 3); agents initialised as the reference's trainer does, the second set with the actor's
last layer times 100; a batch of S = 4099 samples, so that the gathers are real.  Minibatch sizes: 2; 63 and 65, either side
of a wavefront; 257; 2049; three of the gradient kernel's tiles plus 5, the tile being read off
``mrl_ppo_workspace_bytes`` (at least three workgroups and a ragged tail); and two sizes beyond the cap on workgroups, which
is where that function stops growing: the cap plus 5 samples (two tiles per workgroup, fewer workgroups than the cap, a last
one of a single ragged tile) and twice the cap plus a tile and 5 (three tiles per workgroup), with repeated sample numbers.

Margins: d is, per kind of number, the largest distance of torch's float32 CPU computation of the trainer's own lines from
the twin on the same inputs; the device must be within 8 x d.  For the vector kinds (gradient, parameters, moments) that is
the largest over the elements of the case at hand.  A scalar stat has one element, and one case's distance is a single draw
of a rounding error (down to 0.01 ulp of the stat here), which bounds nothing: its d is the largest over the three shapes
and three batches each (two at the largest sizes) at the same weight set, minibatch size and flags, ``ppo_twin.stat_margins``.  Against a row's OWN distance the
first build's stats, summed in float32, measured up to 123 (old_approx_kl) with the gradient at 2.6 at the most, and the
present one, which sums the float32 terms in double and rounds once, still up to 295 (pg_loss); those ratios are printed.
Measured with the pooled d: at most 6.6 (old_approx_kl).  The chained rows and the index row assert the gradient and clipfrac.  The batches hold synthetic "old" data that put 16-38 % of the
samples above the ratio clip, 16-29 % below it and about 60 % on the clipped value branch, and no sample within 1e-5 of a
kink of the loss (tests/test_ppo_update_api.py asserts both for every case here).  Each test prints the ratios it measured."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import policy_twin  # noqa: E402
import ppo_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CartpoleSimulator, ExecMode, MlpPolicy, PpoOptimizer, Rollout,  # noqa: E402
                                                         ppo_update)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED = "three tiles and a tail"


def workspace_bytes(width, rows=1, shape=(4, 64, 2)):
    out = ctypes.c_uint64(0)
    _lib.check(_lib.lib().mrl_ppo_workspace_bytes(shape[0], shape[1], shape[2], width, rows, ctypes.byref(out)))
    return out.value


@functools.lru_cache(maxsize=None)
def tile():
    return twin.tile_size(workspace_bytes)


def resolve(width):
    return 3 * tile() + 5 if width == RAGGED else width


def cuda(array):
    return torch.from_numpy(np.ascontiguousarray(array)).cuda()


def cpu(tensor):
    return tensor.cpu().numpy().copy()


class Device:
    """A policy, its optimizer and a batch on the GPU."""

    def __init__(self, params, batch, cfg, step=0, moments=None):
        d = batch.obs.shape[1]
        self.policy = MlpPolicy(d, int(twin._num_actions(params, d)), device="cuda:0")
        self.policy.params.copy_(cuda(params))
        self.optimizer = PpoOptimizer(self.policy, lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.optimizer.step = step
        if moments is not None:
            self.optimizer.exp_avg.copy_(cuda(moments[0]))
            self.optimizer.exp_avg_sq.copy_(cuda(moments[1]))
        self.cfg = cfg
        self.batch = twin.Batch(*[cuda(a) for a in batch])
        b = self.batch
        self.rollout = Rollout(b.obs, b.actions, b.logprobs, b.values, None, None, None, None, None)

    def update(self, indices, grads=True):
        c = self.cfg
        result = ppo_update(self.policy, self.optimizer, self.rollout, self.batch.advantages, self.batch.returns, cuda(indices),
                            clip_coef=c.clip_coef, ent_coef=c.ent_coef, vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm,
                            norm_adv=c.norm_adv, clip_vloss=c.clip_vloss, stats=True, grads=grads)
        return cpu(result.stats), cpu(result.grads) if grads else None

    def state(self):
        return cpu(self.policy.params), cpu(self.optimizer.exp_avg), cpu(self.optimizer.exp_avg_sq)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def check_row(what, got_stats, got_grad, exact, single, width, stat_d=None):
    """One row of the device against the twin's row ``exact``.  The gradient must be within 8 d, d = |``single`` - ``exact``|,
    and clipfrac must be the twin's count / B.  With ``stat_d`` (``twin.stat_margins`` of the case's group) every other stat
    must be within 8 x its d; the ratios against the row's own distance are printed either way."""
    d = twin.row_margins(exact, single)
    ratios = {"grad": twin.distance(got_grad, exact["grad"]) / d["grad"]}
    own = {}
    for column, name in enumerate(twin.STATS):
        if name == "clipfrac":
            continue
        off = abs(float(got_stats[column]) - exact["stats"][name])
        own[name] = off / d[name] if d[name] > 0 else (0.0 if off == 0 else float("inf"))
        if stat_d is not None:
            ratios[name] = off / stat_d[name]
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e;" % d["grad"],
          "stats / this row's own distance:", {k: round(v, 2) for k, v in own.items()})
    count = round(exact["stats"]["clipfrac"] * width)
    assert got_stats[twin.STATS.index("clipfrac")] == np.float32(count) / np.float32(width), what
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)


@pytest.mark.parametrize("width", twin.FIXED_SIZES + [RAGGED])
@pytest.mark.parametrize("scale", twin.SCALES)
@pytest.mark.parametrize("shape", twin.SHAPES)
def test_gradient_and_stats_parity(shape, scale, width):
    width = resolve(width)
    if width != 3 * tile() + 5:
        assert width in twin.FIXED_SIZES
    else:
        # every workgroup adds one partial vector (and a few floats of padding) to the workspace
        groups = 1 + round((workspace_bytes(width) - workspace_bytes(1)) / (workspace_bytes(tile() + 1) - workspace_bytes(1)))
        assert groups >= 4 and width % tile(), "at least three whole workgroups and a ragged one"
    case = (shape[0], shape[1], scale, width, "default")
    fixed = twin.fixed_case(case)
    stats, grads = Device(fixed["params"], fixed["batch"], fixed["cfg"]).update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed["twin"], fixed["f32"], width, twin.stat_margins(case))


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("shape", twin.SHAPES)
def test_parity_with_several_tiles_per_workgroup(shape, which):
    """Beyond the cap a workgroup walks several tiles: its register and AGPR sums persist and the LDS images are reused."""
    saturation = twin.saturation(workspace_bytes)
    assert saturation % tile() == 0 and saturation // tile() >= 2
    width = twin.large_sizes(tile(), saturation)[which]
    assert workspace_bytes(width) == workspace_bytes(saturation) and width % tile()
    case = (shape[0], shape[1], 1.0, width, "default")
    fixed = twin.fixed_case(case)
    assert len(np.unique(fixed["indices"][0])) < width
    stats, grads = Device(fixed["params"], fixed["batch"], fixed["cfg"]).update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed["twin"], fixed["f32"], width, twin.stat_margins(case))


@pytest.mark.parametrize("variant", [v for v in sorted(twin.VARIANTS) if v != "default"])
@pytest.mark.parametrize("shape", twin.SHAPES)
def test_flag_variants(shape, variant):
    case = (shape[0], shape[1], 1.0, 257, variant)
    fixed = twin.fixed_case(case)
    device = Device(fixed["params"], fixed["batch"], fixed["cfg"])
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed["twin"], fixed["f32"], 257, twin.stat_margins(case))
    if variant == "no_grad_clip":  # the step is Adam on the unclipped gradient
        want = twin.clip_adam(fixed["params"], 0.0 * grads[0], 0.0 * grads[0], grads[0], 0, fixed["cfg"])
        clipped = twin.clip_adam(fixed["params"], 0.0 * grads[0], 0.0 * grads[0], grads[0], 0, twin.Config(max_grad_norm=0.01))
        assert twin.distance(device.state()[1], want[2]) < 1e-3 * twin.distance(want[2], clipped[2])


@pytest.mark.parametrize("max_grad_norm", [0.5, 1e6])
@pytest.mark.parametrize("step", [0, 999])
@pytest.mark.parametrize("case", twin.ADAM_CASES)
def test_adam_parity_on_the_devices_own_gradient(case, step, max_grad_norm):
    fixed = twin.fixed_case(case)
    cfg = twin.Config(max_grad_norm=max_grad_norm, norm_adv=False)
    moments = twin.moments(fixed["params"].size, 5) if step else None
    device = Device(fixed["params"], fixed["batch"], cfg, step=step, moments=moments)
    before = device.state()
    stats, grads = device.update(fixed["indices"])
    after = device.state()
    assert device.optimizer.step == step + 1
    exact = twin.clip_adam(*before, grads[0], step, cfg)
    single = twin.clip_adam_torch(*before, grads[0], step, cfg, torch.float32)
    assert (exact[0] > 0.5) and exact[0] < 1e6, "the norm must exceed the trainer's 0.5 and stay below the bound that never clips"
    got = (float(stats[0][twin.STATS.index("total_norm")]),) + after
    ratios = {}
    for name, g, e, s in zip(("total_norm", "params", "exp_avg", "exp_avg_sq"), got, exact, single):
        d = twin.distance(s, e)
        off = twin.distance(g, e)
        ratios[name] = off / d if d > 0 else (0.0 if off == 0 else float("inf"))
    print(case, step, max_grad_norm, "measured / d:", {k: round(v, 2) for k, v in ratios.items()})
    assert not np.array_equal(before[0], after[0])
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (name, ratio)


@pytest.mark.parametrize("width", twin.CHAIN_SIZES)
@pytest.mark.parametrize("shape", twin.SHAPES)
def test_chained_rows(shape, width):
    case = (shape[0], shape[1], 1.0, width, "default")
    fixed = twin.fixed_case(case, twin.CHAIN_ROWS)
    cfg, indices, rows = fixed["cfg"], fixed["indices"], twin.CHAIN_ROWS

    def whole():
        device = Device(fixed["params"], fixed["batch"], cfg)
        stats, grads = device.update(indices)
        assert device.optimizer.step == rows
        return device.state() + (stats, grads)

    first, second = whole(), whole()
    names = ("params", "exp_avg", "exp_avg_sq", "stats", "grads")
    for name, a, b in zip(names, first, second):
        same_bits(a, b, f"{case}: {name} of a second identical run")
    device = Device(fixed["params"], fixed["batch"], cfg)
    before, stats, grads = [], [], []
    for k in range(rows):
        before.append(device.state()[0])
        s, g = device.update(indices[k:k + 1])
        stats.append(s[0])
        grads.append(g[0])
    assert device.optimizer.step == rows
    for name, a, b in zip(names, first, device.state() + (np.stack(stats), np.stack(grads))):
        same_bits(a, b, f"{case}: {name} of one call of {rows} rows against {rows} calls of one")
    skipped = 0
    for k in range(rows):
        exact = twin.row(before[k], fixed["batch"], indices[k], cfg)
        if exact["kink"] <= twin.KINK:
            skipped += 1
            continue
        single = twin.row(before[k], fixed["batch"], indices[k], cfg, torch.float32)
        check_row(f"{case} row {k}", stats[k], grads[k], exact, single, width)
    print(f"{case}: {skipped} of {rows} rows skipped")
    assert skipped <= twin.CHAIN_MAX_SKIPPED
    assert not np.array_equal(before[0], before[1])


def test_matrix_core_operand_maps_with_exact_integers():
    """dW2 of the critic as exact integers: a first layer that saturates tanh (h1 in {-1, 0, 1}), a second layer of zeros
    (h2 = 0, so d2[j] = W3[j] d3), W3[j] = j - 20, returns of 65536 r with integer r and B = 32768 (d3 = -r exactly).  Then
    dW2[j][i] = sum_s d2[j][s] h1[i][s] is an asymmetric integer matrix below 2^24 that float32 holds exactly whatever the
    order of the sums: a wrong A, B or C/D lane map of the MFMA, or a sum lost between a workgroup's tiles, changes it."""
    d, a, h, count = 4, 2, 64, 32768
    rng = np.random.default_rng(3)
    patterns = np.array([[(i + 1) // 3 ** k % 3 - 1 for k in range(d)] for i in range(h)], np.float64)  # 64 different rows of -1 / 0 / 1
    obs = rng.choice([-1.0, 1.0], size=(count, d))
    r = rng.integers(-3, 4, size=count).astype(np.float64)
    w3 = np.arange(h, dtype=np.float64) - 20.0
    critic = np.concatenate([(64.0 * patterns).reshape(-1), np.zeros(h), np.zeros(h * h), np.zeros(h), w3, np.zeros(1)])
    params = np.concatenate([critic, np.zeros(twin.initial_params(d, a, 1.0).size - critic.size)]).astype(np.float32)
    batch = twin.Batch(obs.astype(np.float32), np.zeros(count, np.int32), np.full(count, np.log(0.5), np.float32),
                       np.zeros(count, np.float32), (65536.0 * r).astype(np.float32), np.zeros(count, np.float32))
    h1 = np.sign(patterns @ obs.T)                      # (unit of layer 1, sample)
    d2 = w3[:, None] * (-r)[None, :]                    # (unit of layer 2, sample)
    want_w2, want_b2 = d2 @ h1.T, d2.sum(axis=1)
    assert np.abs(want_w2).max() < 2 ** 24 and not np.array_equal(want_w2, want_w2.T) and np.abs(want_w2).min() == 0 < np.abs(want_w2).max()
    cfg = twin.Config(norm_adv=False, clip_vloss=False, max_grad_norm=0.0)
    _, grads = Device(params, batch, cfg).update(np.arange(count, dtype=np.int32)[None, :])
    at = d * h + h
    same_bits(grads[0][at:at + h * h].reshape(h, h), want_w2.astype(np.float32), "dW2 of the critic")
    same_bits(grads[0][at + h * h:at + h * h + h], want_b2.astype(np.float32), "db2 of the critic")


def test_indices_and_inputs_left_alone():
    d, a, width = 4, 2, 65
    params = twin.initial_params(d, a, 1.0)
    batch = twin.make_batch(params, d, a, twin.BATCH, 77)
    # descending, every sample number twice over, the batch's last sample first
    indices = (twin.BATCH - 1 - np.arange(width) // 2).astype(np.int32)[None, :]
    cfg = twin.Config()
    exact = twin.row(params, batch, indices[0], cfg)
    assert exact["kink"] > twin.KINK
    device = Device(params, batch, cfg)
    pointer = device.policy.params.data_ptr()
    device_indices = cuda(indices)
    result = ppo_update(device.policy, device.optimizer, device.rollout, device.batch.advantages, device.batch.returns,
                        device_indices, grads=True)
    check_row("repeated, descending indices", cpu(result.stats)[0], cpu(result.grads)[0], exact,
              twin.row(params, batch, indices[0], cfg, torch.float32), width)
    for name, tensor, array in zip(twin.Batch._fields, device.batch, batch):
        same_bits(cpu(tensor), array, f"batch.{name} after the call")
    same_bits(cpu(device_indices), indices, "indices after the call")
    assert device.policy.params.data_ptr() == pointer and not np.array_equal(cpu(device.policy.params), params)


def test_rollout_reads_the_updated_parameters():
    """after an update ``rollout_policy`` runs on ``policy.params`` as it stands: there is no ``load_``"""
    fixed = twin.fixed_case((4, 2, 1.0, 257, "default"), twin.CHAIN_ROWS)
    device = Device(fixed["params"], fixed["batch"], twin.Config(lr=1e-2))
    device.update(fixed["indices"], grads=False)
    params = cpu(device.policy.params)
    assert twin.distance(params, fixed["params"]) > 1e-2
    n, rows = 63, 4
    sim = CartpoleSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    rollout = sim.rollout_policy(device.policy, rows, seed=9)
    obs, actions = cpu(rollout.obs).reshape(-1, 4), cpu(rollout.actions).reshape(-1)
    values, logprobs = cpu(rollout.values).reshape(-1), cpu(rollout.logprobs).reshape(-1)
    sim.close()
    d_value, d_logp = policy_twin.margins(twin.agent_from(params, 4, 2, torch.float32), params, obs, actions)
    exact = policy_twin.act(params, obs, np.zeros(len(obs)), 2)
    off_value = twin.distance(values, exact["values"])
    off_logp = twin.distance(logprobs, exact["logp"][np.arange(len(obs)), actions])
    stale = policy_twin.act(fixed["params"], obs, np.zeros(len(obs)), 2)
    print("measured / d: values %.2f, logprobs %.2f" % (off_value / d_value, off_logp / d_logp))
    assert off_value <= twin.FACTOR * d_value and off_logp <= twin.FACTOR * d_logp
    assert twin.distance(values, stale["values"]) > 100 * twin.FACTOR * d_value, "the rollout ran on the parameters before the update"


def test_trainer_on_the_device():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import cartpole_train_device
    finally:
        sys.path.pop(0)
    history = cartpole_train_device.train(64, 32, 2, 5)
    assert len(history) == 2 and history[-1]["optimizer_step"] == 2 * 4 * 4
    for entry in history:
        for name in twin.STATS:
            assert np.isfinite(entry[name]) and np.isfinite(entry["last_" + name]), (name, entry)
    assert history[0]["entropy"] > 0.5 and history[0]["episodes"] > 0 and history[0]["lr"] > history[1]["lr"] > 0


def test_refusals_on_a_live_device():
    fixed = twin.fixed_case((4, 2, 1.0, 63, "default"))
    device = Device(fixed["params"], fixed["batch"], fixed["cfg"])
    before = device.state()
    p, o, b = device.policy.params, device.optimizer, device.batch
    indices = cuda(fixed["indices"])
    shape = _lib.MlpPolicyDesc(p.data_ptr(), 4, 64, 2, 0, 0)
    opt = _lib.PpoOptimizerDesc(p.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr(), 0)
    cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, 3)
    workspace = o.workspace(63, 1)
    L = _lib.lib()

    def call(obs, workspace_bytes, stream):
        batch = _lib.PpoBatch(obs, b.actions.data_ptr(), b.logprobs.data_ptr(), b.advantages.data_ptr(), b.returns.data_ptr(),
                              b.values.data_ptr(), twin.BATCH)
        rc = L.mrl_ppo_update(ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), 1, 63, ctypes.byref(cfg),
                              workspace.data_ptr(), workspace_bytes, None, None, 0, stream)
        return rc, L.mrl_last_error().decode()

    # the Python layer's own refusals, which need parameters on the GPU to be reached
    good = dict(advantages=b.advantages, returns=b.returns, indices=indices)
    for name, bad in (("indices", indices.long()), ("indices", indices[0]), ("advantages", b.advantages.double()),
                      ("returns", b.returns[::2]), ("returns", b.returns[:-1]), ("advantages", b.advantages.cpu())):
        with pytest.raises(ValueError, match=name):
            ppo_update(device.policy, o, device.rollout, **dict(good, **{name: bad}))
    strided = torch.stack([b.obs, b.obs], dim=1)[:, 0]
    with pytest.raises(ValueError, match="rollout.obs"):
        ppo_update(device.policy, o, device.rollout._replace(obs=strided), **good)
    with pytest.raises(ValueError, match="rollout.actions"):
        ppo_update(device.policy, o, device.rollout._replace(actions=b.actions.long()), **good)
    assert o.step == 0
    rc, message = call(b.obs.data_ptr() + 4, workspace.numel(), None)
    assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_update" in message and "boundary" in message
    rc, message = call(b.obs.data_ptr(), workspace_bytes(63) - 1, None)
    assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_update" in message and "workspace" in message
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device="cuda:0")
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc, message = call(b.obs.data_ptr(), workspace.numel(), side.cuda_stream)
            scratch.add_(0)
    assert rc == _lib.MRL_ERR_INVALID and "mrl_ppo_update" in message and "captured" in message
    torch.cuda.synchronize()
    for name, a, c in zip(("params", "exp_avg", "exp_avg_sq"), before, device.state()):
        same_bits(a, c, f"{name} after three refused calls")
    rc, message = call(b.obs.data_ptr(), workspace.numel(), None)
    assert rc == _lib.MRL_OK, message
    torch.cuda.synchronize()
    assert not np.array_equal(before[0], device.state()[0])
