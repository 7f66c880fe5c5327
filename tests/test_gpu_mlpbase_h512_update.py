"""GPU: ``mappo_update_h512`` on an ``MlpBasePolicyH512`` (mrl_mappo_mlp_update with MRL_MLPBASE_H512: the layered update of the
hidden-512 MLPBase actor-critic) against tests/mlpbase_twin.py's float64 twin pointed at the 512 module
(tests/mlpbase_h512_update_cases.py).

Margins as in tests/test_gpu_cnn_h512_update.py: d is, per kind of number, the distance of the float32 CPU computation of the same
losses from the twin on the same inputs; the device must be within 8 x d.  A scalar stat's d is pooled over the cases of its test.
The inputs' conditions are asserted by tests/test_mlpbase_h512_update_api.py.  Each test prints the ratios it measured.

Measured / d on an MI355X (the largest per test): see DESIGN.md section 33."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mlpbase_h512_update_cases as cases  # noqa: E402
import mlpbase_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (MappoOptimizer, MappoOptimizerH512, MlpBasePolicy, MlpBasePolicyH512, MlpBaseRecord,  # noqa: E402
                                                         ValueNorm, mappo_update, mappo_update_h512)

DEV = torch.device("cuda", 0)
STAT = _lib.MAPPO_STATS.index
beam = cases.beam


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


class Device:
    """A 512 policy, its optimizer, a ValueNorm and a batch (as a record) on the GPU."""

    def __init__(self, fixed, cfg=None):
        batch = fixed["batch"]
        self.cfg = cfg = cfg or fixed["cfg"]
        self.policy = MlpBasePolicyH512(fixed["layer_N"], DEV)
        self.policy.params.copy_(cuda(np.asarray(fixed["params"], np.float32)))
        self.optimizer = MappoOptimizerH512(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        t, n, p = beam.T, beam.N, beam.P
        self.record = MlpBaseRecord(t, n, p, DEV)
        self.record.actions.copy_(cuda(batch.actions).view(t, n, p))
        self.record.logprobs.copy_(cuda(batch.logprobs).view(t, n, p))
        self.record.values[:t].copy_(cuda(batch.values).view(t, n, p))
        self.record.obs[:t].copy_(cuda(batch.obs).view(t, n, p, 7))
        self.advantages = cuda(batch.advantages).view(t, n, p)
        self.returns = cuda(batch.returns).view(t, n, p)
        self.value_norm = ValueNorm(DEV, beta=0.99999, epsilon=1e-5)
        self.value_norm.state.copy_(cuda(np.asarray(twin.STATE0, np.float32)))

    def update(self, indices):
        c = self.cfg
        result = mappo_update_h512(self.policy, self.optimizer, self.record, None, self.advantages, self.returns, cuda(indices),
                                   value_norm=self.value_norm if c.valuenorm else None, clip_param=c.clip_param, entropy_coef=c.entropy_coef,
                                   value_loss_coef=c.value_loss_coef, max_grad_norm=c.max_grad_norm, huber_delta=c.huber_delta,
                                   use_huber_loss=c.huber, use_clipped_value_loss=c.clipped_value, use_max_grad_norm=c.clip_grads,
                                   stats=True, grads=True)
        return cpu(result.stats), cpu(result.grads)

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


def check_row(what, got_stats, got_grad, fixed, stat_d):
    """tests/test_gpu_cnn_h512_update.py's ``check_row``: the gradient's ratio per net, every stat within 8 x its pooled d"""
    exact, single, width, na = fixed["twin"], fixed["f32"], fixed["indices"].shape[1], cases.actor_size(fixed["layer_N"])
    d = twin.row_margins(exact, single)
    ratios = {"actor_grad": twin.distance(got_grad[:na], exact["grad"][:na]) / d["grad"],
              "critic_grad": twin.distance(got_grad[na:], exact["grad"][na:]) / d["grad"]}
    for name in twin.STATS:
        if name != "clipfrac":
            off = abs(float(got_stats[STAT(name)]) - exact["stats"][name])
            ratios[name] = off / stat_d[name] if stat_d[name] > 0 else (0.0 if off == 0 else float("inf"))
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d["grad"])
    count = round(exact["stats"]["clipfrac"] * width)
    assert got_stats[STAT("clipfrac")] == np.float32(np.float64(count) / np.float64(width)), what
    assert got_stats[STAT("reserved")] == 0
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)
    for sl in cases.fc_h_slices(fixed["layer_N"]):
        assert not got_grad[sl].any(), "fc_h's gradient"


@pytest.mark.parametrize("case", cases.PARITY, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_and_stats_match_the_twin(hip_lib, case):
    fixed = cases.fixed(*case)
    device = Device(fixed)
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(tuple(cases.PARITY)))
    if case[2] == "dead":  # behind the dead ReLU: exactly zero, in both nets
        assert all(not grads[0][at:at + cases.DEAD].any() for at in (0, cases.actor_size(case[0])))
    assert device.optimizer.step == 1


@pytest.mark.parametrize("case", cases.CROSSING, ids=lambda c: "-".join(str(x) for x in c))
def test_crossing_the_shares_and_the_slab(hip_lib, case):
    """a ragged last share; a second slab that must add to the first one's sums, not restart from 0; two rows"""
    fixed = cases.fixed(*case, rows=2)
    stats, grads = Device(fixed).update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(tuple(cases.CROSSING)))
    assert np.isfinite(grads[1]).all() and grads[1].any()


@pytest.mark.parametrize("layer_N", (1, 2))
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, layer_N):
    """the forward pass with stores is the act's: on unchanged parameters the ratio is exactly 1, and with the record's own values as
    returns (plain squared error) the value loss and the critic's gradient are exactly 0"""
    from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
    t, n = 2, 33
    policy = MlpBasePolicyH512.from_module(cases.h512.make_module(layer_N, "trained"), device=DEV)
    env = BalanceMadronaTorch(n, 0)
    record = env.rollout(policy, t, seed=5, first_step=0)
    count = t * n * 2
    returns = record.values[:t].clone()
    indices = torch.arange(count, dtype=torch.int32, device=DEV).view(1, count)
    result = mappo_update_h512(policy, MappoOptimizerH512(policy), record, None, torch.ones_like(returns), returns, indices, value_norm=None,
                               use_huber_loss=False, use_clipped_value_loss=False)
    stats = cpu(result.stats)[0]
    assert stats[STAT("ratio")] == 1.0 and stats[STAT("clipfrac")] == 0.0 and stats[STAT("policy_loss")] == -1.0
    assert stats[STAT("value_loss")] == 0.0 and stats[STAT("critic_grad_norm")] == 0.0
    env.close()


@pytest.mark.parametrize("clips", [True, False])
def test_the_step_matches_the_twin(hip_lib, clips):
    """two rows with ValueNorm, a call each, every step teacher-forced on the device's own gradient and the state before it:
    parameters, moments and the ValueNorm state; fc_h is left bit for bit as it was"""
    fixed = cases.fixed(2, 65, "trained", rows=2)
    layer_N, batch = fixed["layer_N"], fixed["batch"]
    cfg = fixed["cfg"]._replace(max_grad_norm=twin.f32(1e-3 if clips else 1e3), lr=twin.f32(3e-4), critic_lr=twin.f32(7e-4))
    device = Device(fixed, cfg)
    start, na, keep = device.state(), cases.actor_size(layer_N), None
    with cases.width_512():
        keep = twin.used(layer_N)
    norm64, norm32 = np.asarray(twin.STATE0, np.float64), np.asarray(twin.STATE0, np.float32)
    for k in range(2):
        before = device.state()
        stats, grads = device.update(fixed["indices"][k:k + 1])
        got, grad = device.state(), grads[0].astype(np.float64)
        exact = cases.step_both(layer_N, before["params"], before["exp_avg"], before["exp_avg_sq"], grad, k, cfg)
        ratios = {}
        for net, (sl, lr) in enumerate(((slice(0, na), cfg.lr), (slice(na, None), cfg.critic_lr))):
            u = keep[sl]
            single = twin.clip_adam_torch(before["params"][sl][u], before["exp_avg"][sl][u], before["exp_avg_sq"][sl][u], grad[sl][u], k,
                                          cfg.max_grad_norm, lr, cfg, torch.float32)
            assert (exact[net] > cfg.max_grad_norm) == clips
            for i, name in enumerate(("params", "exp_avg", "exp_avg_sq")):
                want = exact[2 + i][sl][u]
                ratios[f"{name}[{net}]"] = twin.distance(got[name][sl][u], want) / max(twin.distance(single[1 + i], want),
                                                                                       float(np.abs(want).max()) * 2.0 ** -24)
        returns = np.asarray(batch.returns)[fixed["indices"][k]]
        norm64, norm32 = twin.value_norm_update(norm64, returns, cfg)[0], twin.value_norm_update(norm32, returns, cfg, np.float32)[0]
        d = np.maximum(np.abs(norm32 - norm64), np.abs(norm64) * 2.0 ** -24)
        ratios["value_norm"] = float((np.abs(got["value_norm"] - norm64) / d).max())
        print("row", k, "clips", clips, "measured / d:", {name: round(r, 2) for name, r in ratios.items()})
        for name, ratio in ratios.items():
            assert ratio <= twin.FACTOR, (k, name, ratio)
    for sl in cases.fc_h_slices(layer_N):
        same_bits(device.state()["params"][sl], start["params"][sl], "fc_h's parameters")
        assert start["params"][sl].any()
    assert device.optimizer.step == 2


def test_one_call_k_calls_a_second_run_and_a_side_stream_agree_bit_for_bit(hip_lib):
    fixed = cases.fixed(2, 65, "trained", rows=3)
    narrow = beam.fixed_case((2, "trained", "synthetic", 65, "default"))

    def hidden_64():
        policy = MlpBasePolicy(layer_N=2, device=DEV)
        policy.params.copy_(cuda(np.asarray(narrow["params"], np.float32)))
        record, b = MlpBaseRecord(beam.T, beam.N, beam.P, DEV), narrow["batch"]
        shape = (beam.T, beam.N, beam.P)
        record.actions.copy_(cuda(b.actions).view(shape)), record.logprobs.copy_(cuda(b.logprobs).view(shape))
        record.values[:beam.T].copy_(cuda(b.values).view(shape)), record.obs[:beam.T].copy_(cuda(b.obs).view(*shape, 7))
        result = mappo_update(policy, MappoOptimizer(policy), record, None, cuda(b.advantages).view(shape), cuda(b.returns).view(shape),
                              cuda(narrow["indices"]), grads=True)
        return cpu(result.stats), cpu(result.grads), cpu(policy.params)

    plain_before = hidden_64()
    whole = Device(fixed)
    stats, grads = whole.update(fixed["indices"])
    want = whole.state()
    single = Device(fixed)
    for k in range(3):
        s, g = single.update(fixed["indices"][k:k + 1])
        same_bits(s[0], stats[k], f"stats of row {k}, one row per call")
        same_bits(g[0], grads[k], f"gradient of row {k}, one row per call")
    again = Device(fixed)
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
    for a, b in zip(plain_before, hidden_64()):
        same_bits(a, b, "a hidden-64 update before and after")


def test_refusals_change_nothing(hip_lib):
    fixed = cases.fixed(2, 65, "trained")
    device = Device(fixed)
    stats = torch.full((1, 8), 7.0, device=DEV)
    before = device.state()
    L = _lib.lib()
    p, o, r = device.policy, device.optimizer, device.record
    indices = cuda(fixed["indices"][:1])
    workspace = o.workspace(indices.shape[1], 1)
    opt = _lib.MappoOptimizerDesc(p.params.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr(), 0)
    batch = _lib.MappoMlpBatch(r.obs.data_ptr(), r.actions.data_ptr(), r.logprobs.data_ptr(), r.values.data_ptr(), device.returns.data_ptr(),
                               device.advantages.data_ptr(), len(fixed["batch"].obs))
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 15)

    def call(hidden=512, flags=0, ws_bytes=None, stream=None, entry=L.mrl_mappo_mlp_update, optimizer=opt):
        policy = _lib.MlpBasePolicyDesc(p.params.data_ptr(), hidden, 2, _lib.MLPBASE_H512 | flags)
        return entry(ctypes.byref(policy), ctypes.byref(optimizer), ctypes.byref(batch), indices.data_ptr(), 1, indices.shape[1], ctypes.byref(cfg),
                     device.value_norm.state.data_ptr(), workspace.data_ptr(), workspace.numel() if ws_bytes is None else ws_bytes,
                     stats.data_ptr(), None, 0, stream if stream is not None else torch.cuda.current_stream().cuda_stream)

    refused = {"recurrent": call(flags=_lib.MLPBASE_RECURRENT), "hidden 64": call(hidden=64)}
    refused["small workspace"] = call(ws_bytes=workspace.numel() - 1)
    assert b"MRL_MLPBASE_H512_HIDDEN" in L.mrl_last_error()
    bank = _lib.MappoBankOptimizerDesc(p.params.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr(), p.params.numel() * 4, 1, 0, 1, 0)
    refused["bank update"] = call(entry=L.mrl_mappo_mlp_bank_update, optimizer=bank)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            refused["capturing stream"] = call(stream=torch.cuda.current_stream().cuda_stream)
            scratch.add_(0)
    for what, rc in refused.items():
        assert rc == 1, what
    torch.cuda.synchronize()
    for name, value in before.items():
        same_bits(device.state()[name], value, name)
    assert (cpu(stats) == 7.0).all() and device.optimizer.step == 0
