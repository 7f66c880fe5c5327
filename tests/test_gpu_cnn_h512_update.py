"""GPU: ``mappo_update_h512`` (mrl_mappo_h512_update: the layered update of the hidden-512 CNN actor-critic) against
tests/mappo_twin.py's float64 twin pointed at the 512 module (tests/cnn_h512_update_cases.py).

Margins as in tests/test_gpu_mappo_update.py: d is, per kind of number, the distance of the float32 CPU computation of the same
losses from the twin on the same inputs; the device must be within 8 x d.  A scalar stat's d is pooled over the cases of its test.
The inputs' conditions are asserted by tests/test_cnn_h512_update_api.py.  Each test prints the ratios it measured."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_h512_update_cases as cases  # noqa: E402
import mappo_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib, simulators  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnRecord, MappoOptimizerH512, ValueNorm, mappo_update_h512)  # noqa: E402

DEV = torch.device("cuda", 0)
shapes = cases.shapes


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


class Device:
    """A 512 policy, its optimizer, a ValueNorm and a batch (as a record and a ring) on the GPU."""

    def __init__(self, key, worlds, params, batch, cfg, state=twin.STATE0, step=0, moments=None):
        w, h, p, f = shapes.shape(key)
        self.policy = CnnPolicy(w, h, f, hidden=512, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(params, np.float32)))
        self.optimizer = MappoOptimizerH512(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.optimizer.step = step
        if moments is not None:
            self.optimizer.exp_avg.copy_(cuda(moments[0]))
            self.optimizer.exp_avg_sq.copy_(cuda(moments[1]))
        steps = len(batch.ring) // (worlds * p)
        assert steps * worlds * p == len(batch.ring)
        self.record = CnnRecord(steps, worlds, p, DEV)
        self.record.actions.copy_(cuda(batch.actions).view(steps, worlds, p))
        self.record.logprobs.copy_(cuda(batch.logprobs).view(steps, worlds, p))
        self.record.values[:steps].copy_(cuda(batch.values).view(steps, worlds, p))
        self.ring = torch.zeros((steps + 1, worlds, p, h, w, f), dtype=torch.int8, device=DEV)
        self.ring[:steps].copy_(cuda(batch.ring).view(steps, worlds, p, h, w, f))
        self.advantages = cuda(batch.advantages).view(steps, worlds, p)
        self.returns = cuda(batch.returns).view(steps, worlds, p)
        self.cfg = cfg
        self.value_norm = ValueNorm(DEV, beta=0.99999, epsilon=1e-5)
        self.value_norm.state.copy_(cuda(np.asarray(state, np.float32)))

    def update(self, indices):
        c = self.cfg
        result = mappo_update_h512(self.policy, self.optimizer, self.record, self.ring, self.advantages, self.returns, cuda(indices),
                                   value_norm=self.value_norm if c.valuenorm else None, clip_param=c.clip_param, entropy_coef=c.entropy_coef,
                                   value_loss_coef=c.value_loss_coef, max_grad_norm=c.max_grad_norm, huber_delta=c.huber_delta,
                                   use_huber_loss=c.huber, use_clipped_value_loss=c.clipped_value, use_max_grad_norm=c.clip_grads,
                                   stats=True, grads=True)
        return cpu(result.stats), cpu(result.grads)

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


def device_of(fixed, **kwargs):
    return Device(fixed["layout"], fixed["worlds"], fixed["params"], fixed["batch"], fixed["cfg"], **kwargs)


def check_row(what, got_stats, got_grad, fixed, stat_d):
    """tests/test_gpu_mappo_update.py's ``check_row``; the gradient's ratio per net"""
    exact, single, width, na = fixed["twin"], fixed["f32"], fixed["indices"].shape[1], cases.actor_size(fixed["layout"])
    d = twin.row_margins(exact, single)
    ratios = {"actor_grad": twin.distance(got_grad[:na], exact["grad"][:na]) / d["grad"],
              "critic_grad": twin.distance(got_grad[na:], exact["grad"][na:]) / d["grad"]}
    for name in twin.STATS:
        if name != "clipfrac":
            off = abs(float(got_stats[_lib.MAPPO_STATS.index(name)]) - exact["stats"][name])
            ratios[name] = off / stat_d[name] if stat_d[name] > 0 else (0.0 if off == 0 else float("inf"))
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d["grad"])
    count = round(exact["stats"]["clipfrac"] * width)
    assert got_stats[_lib.MAPPO_STATS.index("clipfrac")] == np.float32(np.float64(count) / np.float64(width)), what
    assert got_stats[_lib.MAPPO_STATS.index("reserved")] == 0
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)


@pytest.mark.parametrize("case", cases.PARITY, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_and_stats_match_the_twin(hip_lib, case):
    fixed = cases.fixed(*case)
    device = device_of(fixed)
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(tuple(cases.PARITY)))
    assert device.optimizer.step == 1


@pytest.mark.parametrize("case", cases.CROSSING, ids=lambda c: "-".join(str(x) for x in c))
def test_crossing_the_shares_and_the_slab(hip_lib, case):
    """a ragged last share, empty shares; a second slab that must add to the first one's sums, not restart from 0"""
    fixed = cases.fixed(*case)
    stats, grads = device_of(fixed).update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(tuple(cases.CROSSING)))


@pytest.mark.parametrize("layout, n", [("cramped_room", 33), ("asymmetric_advantages", 33), ("coordination_ring", 3)])
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, layout, n):
    """the forward pass with stores is the act's, rows off 4-byte boundaries included: on unchanged parameters the ratio is exactly
    1, and with the record's own values as returns (plain squared error) the value loss and the critic's gradient are exactly 0"""
    from madrona_rl_envs_playground_amd.envs import OvercookedMadrona
    w, h, _, f = twin.shape_of(layout)
    policy = CnnPolicy.from_module(cases.h512.module_of(w, h, f, "trained"), device=DEV)
    env = OvercookedMadrona(layout, n, 0, horizon=400)
    record, ring = env.rollout(policy, 2, seed=5, first_step=0)
    count = 2 * n * 2
    returns = record.values[:2].clone()
    indices = torch.arange(count, dtype=torch.int32, device=DEV).view(1, count)
    result = mappo_update_h512(policy, MappoOptimizerH512(policy), record, ring, torch.ones_like(returns), returns, indices, value_norm=None,
                               use_huber_loss=False, use_clipped_value_loss=False, grads=True)
    stats = dict(zip(_lib.MAPPO_STATS, cpu(result.stats)[0]))
    assert stats["ratio"] == 1.0 and stats["clipfrac"] == 0.0 and stats["policy_loss"] == -1.0
    assert stats["value_loss"] == 0.0 and stats["critic_grad_norm"] == 0.0
    grads = cpu(result.grads)[0]
    na = sum(p.numel() for p in policy.module().actor.parameters())
    assert not grads[na:].any() and grads[:na].any()
    env.close()


@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_matrix_core_operand_maps_with_exact_integers(hip_lib, key):
    """critic only, every number an integer below 2^24 (asserted on the CPU): the flatten index, the channel-block offsets and
    the C/D row maps of every weight and bias gradient, bit for bit against int64 back-propagation"""
    case = cases.integer_case(key)
    device = Device(key, twin.N, case["params"], case["batch"], case["cfg"])
    _, grads = device.update(case["indices"])
    same_bits(grads[0][cases.actor_size(key):], case["grad"].astype(np.float32), "the critic's gradient")


@pytest.mark.parametrize("clips", [True, False])
def test_the_step_matches_the_twin(hip_lib, clips):
    """teacher-forced on the device's own gradient: parameters, moments and both norms; actor and critic at different rates"""
    fixed = cases.fixed("cramped_room", 65)
    cfg = fixed["cfg"]._replace(max_grad_norm=twin.f32(1e-3 if clips else 1e3), lr=twin.f32(3e-4), critic_lr=twin.f32(7e-4))
    key, params, na = fixed["layout"], fixed["params"], cases.actor_size(fixed["layout"])
    moments, step = twin.moments(params.size, 11), 5
    device = Device(key, fixed["worlds"], params, fixed["batch"], cfg, step=step, moments=moments)
    stats, grads = device.update(fixed["indices"])
    got, grad = device.state(), grads[0].astype(np.float64)
    exact = cases.step_both(key, params, moments[0], moments[1], grad, step, cfg)
    for net, (sl, lr, column) in enumerate(((slice(0, na), cfg.lr, "actor_grad_norm"), (slice(na, None), cfg.critic_lr, "critic_grad_norm"))):
        limit = cfg.max_grad_norm
        total32, p32, m32, v32 = twin.clip_adam_torch(params[sl], moments[0][sl], moments[1][sl], grad[sl], step, limit, lr, cfg, torch.float32)
        total, p, m, v = exact[net], exact[2][sl], exact[3][sl], exact[4][sl]
        assert (total > limit) == clips
        ratios = {}
        for name, have, want, single in (("params", got["params"][sl], p, p32), ("exp_avg", got["exp_avg"][sl], m, m32),
                                         ("exp_avg_sq", got["exp_avg_sq"][sl], v, v32)):
            ratios[name] = twin.distance(have, want) / max(twin.distance(single, want), float(np.abs(want).max()) * 2.0 ** -24)
        ratios["norm"] = abs(float(stats[0][_lib.MAPPO_STATS.index(column)]) - total) / max(abs(total32 - total), total * 2.0 ** -24)
        print("net", net, "clips", clips, "measured / d:", {k: round(r, 2) for k, r in ratios.items()})
        for name, ratio in ratios.items():
            assert ratio <= twin.FACTOR, (net, name, ratio)
    assert device.optimizer.step == step + 1


def test_one_call_k_calls_a_second_run_and_a_side_stream_agree_bit_for_bit(hip_lib):
    fixed = cases.fixed("cramped_room", 65, "default", 3)
    whole = device_of(fixed)
    stats, grads = whole.update(fixed["indices"])
    want = whole.state()
    single = device_of(fixed)
    for k in range(3):
        s, g = single.update(fixed["indices"][k:k + 1])
        same_bits(s[0], stats[k], f"stats of row {k}, one row per call")
        same_bits(g[0], grads[k], f"gradient of row {k}, one row per call")
    again = device_of(fixed)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        s2, g2 = again.update(fixed["indices"])
    side.synchronize()
    same_bits(s2, stats, "stats on a side stream")
    same_bits(g2, grads, "gradients on a side stream")
    for name, value in want.items():
        same_bits(single.state()[name], value, f"{name}, one row per call")
        same_bits(again.state()[name], value, f"{name}, second run on a side stream")
    assert whole.optimizer.step == single.optimizer.step == 3 and not np.array_equal(want["params"], fixed["params"])


def test_refusals_change_nothing(hip_lib):
    fixed = cases.fixed("cramped_room", 65)
    device = device_of(fixed)
    stats = torch.full((1, 8), 7.0, device=DEV)
    before = device.state()
    L = _lib.lib()
    w, h, p, f = shapes.shape(fixed["layout"])
    indices = cuda(fixed["indices"][:1])
    workspace = device.optimizer.workspace(indices.shape[1], 1)

    def call(hidden=512, flags=0, ws_bytes=None, stream=None, shape=(w, h, f)):
        policy = _lib.MappoPolicyDesc(device.policy.params.data_ptr(), hidden, _lib.MAPPO_H512 | flags, *shape)
        opt = _lib.MappoOptimizerDesc(device.policy.params.data_ptr(), device.optimizer.exp_avg.data_ptr(), device.optimizer.exp_avg_sq.data_ptr(), 0)
        batch = _lib.MappoBatch(device.ring.data_ptr(), device.record.actions.data_ptr(), device.record.logprobs.data_ptr(),
                                device.record.values.data_ptr(), device.returns.data_ptr(), device.advantages.data_ptr(), len(fixed["batch"].ring))
        cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 15)
        return L.mrl_mappo_update(ctypes.byref(policy), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), 1, indices.shape[1],
                                       ctypes.byref(cfg), device.value_norm.state.data_ptr(), workspace.data_ptr(),
                                       workspace.numel() if ws_bytes is None else ws_bytes, stats.data_ptr(), None, 0,
                                       stream if stream is not None else torch.cuda.current_stream().cuda_stream)

    refused = {"hidden 64": call(hidden=64), "recurrent": call(flags=_lib.CNN_RECURRENT), "small workspace": call(ws_bytes=workspace.numel() - 16)}
    refused["a kitchen that does not fit"] = call(shape=(12, 5, 26))
    assert b"LDS image of 203872 bytes" in L.mrl_last_error()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            refused["capturing stream"] = call(stream=torch.cuda.current_stream().cuda_stream)
            scratch.add_(0)
    for what, rc in refused.items():
        assert rc == 1, what
    torch.cuda.synchronize()
    for name, value in before.items():
        same_bits(device.state()[name], value, name)
    assert (cpu(stats) == 7.0).all() and device.optimizer.step == 0
    assert simulators.mappo_update_h512 is mappo_update_h512
