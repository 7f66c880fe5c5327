"""GPU: ``mappo_update`` (mrl_mappo_update: ValueNorm, gradient, reduce, clip + Adam per net) against the float64 twin of
tests/mappo_twin.py.

Margins: d is, per kind of number, the largest distance of the float32 CPU computation of the same losses from the twin on the
same inputs; the device must be within 8 x d.  For the vector kinds (gradient, parameters, moments) that is the largest over
the elements of the case at hand; a scalar stat's d is pooled over the cases of its weight set (``mappo_twin.stat_margins``).
The inputs' conditions -- no sample within 1e-5 of a kink, no pre-activation near 0, the branch shares -- are asserted for
every case here by tests/test_mappo_update_api.py.  Each test prints the ratios it measured."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_twin  # noqa: E402
import mappo_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs import OvercookedMadrona  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnPolicy, CnnRecord, MappoOptimizer, ValueNorm, mappo_advantages,  # noqa: E402
                                                         mappo_update, minibatch_indices)

DEV = torch.device("cuda", 0)


def workspace_bytes(width, rows=1, layout="cramped_room"):
    w, h, _, f = twin.shape_of(layout)
    out = ctypes.c_uint64(0)
    _lib.check(_lib.lib().mrl_mappo_workspace_bytes(w, h, f, 64, width, rows, ctypes.byref(out)))
    return out.value


@functools.lru_cache(maxsize=None)
def saturation():
    return twin.saturation(workspace_bytes)


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


class Device:
    """A policy, its optimizer, a ValueNorm and a batch (as a record and a ring) on the GPU."""

    def __init__(self, layout, worlds, params, batch, cfg, state=twin.STATE0, step=0, moments=None):
        w, h, p, f = twin.shape_of(layout)
        self.policy = CnnPolicy(w, h, f, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(params, np.float32)))
        self.optimizer = MappoOptimizer(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
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

    def update(self, indices, grads=True, stats=True):
        c = self.cfg
        result = mappo_update(self.policy, self.optimizer, self.record, self.ring, self.advantages, self.returns, cuda(indices),
                              value_norm=self.value_norm if c.valuenorm else None, clip_param=c.clip_param, entropy_coef=c.entropy_coef,
                              value_loss_coef=c.value_loss_coef, max_grad_norm=c.max_grad_norm, huber_delta=c.huber_delta,
                              use_huber_loss=c.huber, use_clipped_value_loss=c.clipped_value, use_max_grad_norm=c.clip_grads,
                              stats=stats, grads=grads)
        return cpu(result.stats) if stats else None, cpu(result.grads) if grads else None

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


def device_of(fixed, **kwargs):
    return Device(fixed["layout"], fixed["worlds"], fixed["params"], fixed["batch"], fixed["cfg"], **kwargs)


def check_row(what, got_stats, got_grad, fixed, stat_d):
    """One row of the device against the twin's: the gradient within 8 d of the case, every stat within 8 x its pooled d, clipfrac
    the twin's count / B."""
    exact, single, width = fixed["twin"], fixed["f32"], fixed["indices"].shape[1]
    d = twin.row_margins(exact, single)
    ratios = {"grad": twin.distance(got_grad, exact["grad"]) / d["grad"]}
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


@pytest.mark.parametrize("case", twin.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_and_stats_match_the_twin(hip_lib, case):
    fixed = twin.fixed_case(case)
    device = device_of(fixed)
    before = device.state()
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, twin.stat_margins(case[2]))
    after = device.state()
    if fixed["cfg"].valuenorm:
        state32 = twin.row(fixed["params"], fixed["layout"], fixed["batch"], fixed["indices"][0], fixed["cfg"], twin.STATE0, torch.float32)["state"]
        d = np.maximum(np.abs(state32 - fixed["twin"]["state"]), np.abs(fixed["twin"]["state"]) * 2.0 ** -24)
        assert (np.abs(after["value_norm"] - fixed["twin"]["state"]) <= twin.FACTOR * d).all()
    else:
        same_bits(after["value_norm"], before["value_norm"], "the ValueNorm state without MRL_MAPPO_VALUENORM")
    assert device.optimizer.step == 1


@pytest.mark.parametrize("which", [0, 1])
def test_beyond_the_cap_on_partial_vectors(hip_lib, which):
    """accumulators that persist from tile to tile, the ragged last tile and the trimmed workgroup count"""
    tile, size = saturation()
    case = twin.large_cases(tile, size)[which]
    assert workspace_bytes(case[4]) == workspace_bytes(size) == workspace_bytes(1 << 30)
    fixed = twin.fixed_case(case)
    stats, grads = device_of(fixed).update(fixed["indices"])
    pooled = twin.stat_margins(case[2], tuple(twin.large_cases(tile, size)))
    check_row(str(case), stats[0], grads[0], fixed, pooled)


@pytest.mark.parametrize("layout", cnn_twin.INTEGER_LAYOUTS)
def test_matrix_core_operand_maps_with_exact_integers(hip_lib, layout):
    """critic only, every number an integer below 2^24: dW_conv, dW_fc1, dW_fc2 (asymmetric integer matrices), dW_head and the
    biases bit for bit against numpy's integer arithmetic"""
    case = twin.integer_case(layout)
    assert case["bound"] < 2 ** 24
    for name, matrix in case["matrices"].items():
        assert np.abs(matrix).max() > 0 and (matrix.shape[0] != matrix.shape[1] or not np.array_equal(matrix, matrix.T)), name
    device = Device(layout, twin.N, case["params"], case["batch"], case["cfg"])
    _, grads = device.update(case["indices"])
    critic = grads[0][twin.actor_size(layout):]
    same_bits(critic, case["grad"].astype(np.float32), "the critic's gradient")


@pytest.mark.parametrize("clips", [True, False])
def test_the_step_matches_the_twin(hip_lib, clips):
    """teacher-forced on the device's own gradient: parameters, moments and both norms; actor and critic at different rates"""
    case = ("cramped_room", twin.N, "trained", "synthetic", 65, "default")
    fixed = twin.fixed_case(case)
    cfg = fixed["cfg"]._replace(max_grad_norm=twin.f32(1e-3 if clips else 1e3), lr=twin.f32(3e-4), critic_lr=twin.f32(7e-4))
    layout, params, na = fixed["layout"], fixed["params"], twin.actor_size(fixed["layout"])
    moments, step = twin.moments(params.size, 11), 5
    device = Device(layout, fixed["worlds"], params, fixed["batch"], cfg, step=step, moments=moments)
    stats, grads = device.update(fixed["indices"])
    got = device.state()
    grad = grads[0].astype(np.float64)
    exact = twin.step_both(layout, params, moments[0], moments[1], grad, step, cfg)
    for net, (sl, lr, column) in enumerate(((slice(0, na), cfg.lr, "actor_grad_norm"), (slice(na, None), cfg.critic_lr, "critic_grad_norm"))):
        limit = cfg.max_grad_norm
        total32, p32, m32, v32 = twin.clip_adam_torch(params[sl], moments[0][sl], moments[1][sl], grad[sl], step, limit, lr, cfg, torch.float32)
        total, p, m, v = twin.clip_adam(params[sl], moments[0][sl], moments[1][sl], grad[sl], step, limit, lr, cfg)
        assert (total > limit) == clips
        ratios = {}
        for name, have, want, single in (("params", got["params"][sl], p, p32), ("exp_avg", got["exp_avg"][sl], m, m32),
                                         ("exp_avg_sq", got["exp_avg_sq"][sl], v, v32)):
            ratios[name] = twin.distance(have, want) / max(twin.distance(single, want), float(np.abs(want).max()) * 2.0 ** -24)
        norm_d = max(abs(total32 - total), total * 2.0 ** -24)
        ratios["norm"] = abs(float(stats[0][_lib.MAPPO_STATS.index(column)]) - total) / norm_d
        print("net", net, "clips", clips, "measured / d:", {k: round(r, 2) for k, r in ratios.items()})
        for name, ratio in ratios.items():
            assert ratio <= twin.FACTOR, (net, name, ratio)
    # each half moves at its own rate: the other net's rate changes nothing in it
    other = Device(layout, fixed["worlds"], params, fixed["batch"], cfg._replace(lr=twin.f32(9e-4)), step=step, moments=moments)
    other.update(fixed["indices"])
    same_bits(other.state()["params"][na:], got["params"][na:], "the critic's half under another actor rate")
    assert not np.array_equal(other.state()["params"][:na], got["params"][:na])
    other = Device(layout, fixed["worlds"], params, fixed["batch"], cfg._replace(critic_lr=twin.f32(9e-4)), step=step, moments=moments)
    other.update(fixed["indices"])
    same_bits(other.state()["params"][:na], got["params"][:na], "the actor's half under another critic rate")
    assert device.optimizer.step == step + 1


ROWS = 6


@functools.lru_cache(maxsize=None)
def chain_case():
    return twin.fixed_case(("cramped_room", twin.N, "trained", "synthetic", 65, "default"), rows=ROWS)


def test_value_norm_over_six_rows_from_a_fresh_state(hip_lib):
    """the state after K = 6 rows against the twin's recurrence, and every row's targets through value_loss: the twin is
    teacher-forced on its own gradients over the six rows (its own ValueNorm state, its own Adam steps)"""
    fixed = chain_case()
    cfg, batch, layout = fixed["cfg"], fixed["batch"], fixed["layout"]
    zero = (0.0, 0.0, 0.0)
    device = device_of(fixed, state=zero)
    stats, _ = device.update(fixed["indices"], grads=False)
    state64, state32 = np.zeros(3), np.zeros(3, np.float32)
    for k in range(ROWS):
        gathered = batch.returns[fixed["indices"][k].astype(np.int64)]
        state64, _, _ = twin.value_norm_update(state64, gathered, cfg)
        state32, _, _ = twin.value_norm_update(state32, gathered, cfg, np.float32)
    got = device.state()["value_norm"]
    d = np.maximum(np.abs(state32.astype(np.float64) - state64), np.abs(state64) * 2.0 ** -24)
    print("ValueNorm state measured / d:", np.abs(got - state64) / d)
    assert (np.abs(got - state64) <= twin.FACTOR * d).all()
    params = fixed["params"].astype(np.float64)
    m, v, state = np.zeros(params.size), np.zeros(params.size), np.zeros(3)
    exact, single = [], []
    for k in range(ROWS):
        out = twin.row(params, layout, batch, fixed["indices"][k], cfg, state)
        single.append(twin.row(params, layout, batch, fixed["indices"][k], cfg, state, torch.float32)["stats"]["value_loss"])
        exact.append(out["stats"]["value_loss"])
        assert out["kink"] > twin.KINK, (k, out["kink"])  # a condition of the inputs, in the twin
        state = out["state"]
        _, _, params, m, v = twin.step_both(layout, params, m, v, out["grad"], k, cfg)
    assert np.abs(state - state64).max() == 0
    # d of the one scalar, pooled over the six rows (tests/ppo_twin.py says why one row's own distance bounds nothing)
    d_loss = max(max(abs(a - b) for a, b in zip(exact, single)), max(abs(a) for a in exact) * 2.0 ** -24)
    ratios = [abs(float(stats[k][_lib.MAPPO_STATS.index("value_loss")]) - exact[k]) / d_loss for k in range(ROWS)]
    print("value_loss of the six rows, measured / d:", [round(r, 2) for r in ratios], "d = %.2e" % d_loss)
    assert max(ratios) <= twin.FACTOR, ratios


def test_one_call_k_calls_and_a_second_run_agree_bit_for_bit(hip_lib):
    fixed = chain_case()
    whole = device_of(fixed)
    stats, grads = whole.update(fixed["indices"])
    want = whole.state()
    single = device_of(fixed)
    for k in range(ROWS):
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
    assert whole.optimizer.step == single.optimizer.step == ROWS
    assert not np.array_equal(want["params"], fixed["params"])


def test_closed_loop_rollout_update_act(hip_lib):
    """env.rollout -> mappo_advantages -> mappo_update -> env.act: before any update the recomputed log-probs are the record's
    bit for bit (ratio exactly 1, clipfrac 0 on row 0), and the act that follows reads the updated tensor in place"""
    layout, n, t = "cramped_room", 33, 4
    module = cnn_twin.make_module(layout, "trained")
    policy = CnnPolicy.from_module(module, device=DEV)
    start = cpu(policy.params)
    env = OvercookedMadrona(layout, n, 0, horizon=cnn_twin.HORIZON)
    record, ring = env.rollout(policy, t, seed=31, first_step=0)
    value_norm = ValueNorm(DEV)
    advantages, returns = mappo_advantages(record, value_norm)
    assert advantages.shape == returns.shape == (t, n, 2)
    count = t * n * 2
    indices = minibatch_indices(count, 1, 2, generator=torch.Generator().manual_seed(3), device=DEV)
    optimizer = MappoOptimizer(policy)
    result = mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=value_norm, grads=True)
    stats = cpu(result.stats)
    assert stats[0][_lib.MAPPO_STATS.index("ratio")] == 1.0 and stats[0][_lib.MAPPO_STATS.index("clipfrac")] == 0.0
    assert stats[1][_lib.MAPPO_STATS.index("ratio")] != 1.0
    assert optimizer.step == 2
    grads = cpu(result.grads)
    # the twin's own two updates on the same data
    cfg = twin.Config(huber_delta=10.0)
    batch = twin.Batch(cpu(ring)[:t].reshape(count, *cpu(ring).shape[3:]), cpu(record.actions).reshape(-1), cpu(record.logprobs).reshape(-1),
                       cpu(record.values)[:t].reshape(-1), cpu(returns).reshape(-1), cpu(advantages).reshape(-1))
    params, m, v, state = start.astype(np.float64), np.zeros(start.size), np.zeros(start.size), np.zeros(3)
    for k, inds in enumerate(cpu(indices)):
        out = twin.row(params, layout, batch, inds, cfg, state)
        if k == 0:
            # gradient parity on the ring of a real rollout, at the rollout's own parameters.  The conditions of the inputs
            # hold for this rollout seed (asserted: they are properties of the twin, not of the device's answer)
            single = twin.row(params, layout, batch, inds, cfg, state, torch.float32)
            closest, worst = twin.relu_margin({"twin": out, "f32": single})
            assert out["kink"] > twin.KINK and closest > twin.FACTOR * worst, (out["kink"], closest, worst)
            d_grad = twin.distance(single["grad"], out["grad"])
            print("real ring, row 0: gradient measured / d:", twin.distance(grads[0], out["grad"]) / d_grad, "d = %.2e" % d_grad)
            assert twin.distance(grads[0], out["grad"]) <= twin.FACTOR * d_grad
        state = out["state"]
        _, _, params, m, v = twin.step_both(layout, params, m, v, out["grad"], k, cfg)
    after = record.__class__(1, n, 2, DEV)
    env.act(policy, record=after, seed=31, step=t)
    torch.cuda.synchronize()
    rows = cnn_twin.rows_of(cpu(ring)[t])
    exact = cnn_twin.act(params, rows, np.zeros(len(rows)))
    d_value, d_logp = cnn_twin.layout_margins(layout, "trained")
    got_values, got_actions, got_logp = cpu(after.values)[0].reshape(-1), cpu(after.actions)[0].reshape(-1), cpu(after.logprobs)[0].reshape(-1)
    print("values off by", np.abs(got_values - exact["values"]).max(), "d", d_value, "; log-probs off by",
          np.abs(got_logp - exact["logp"][np.arange(len(rows)), got_actions]).max(), "d", d_logp)
    assert not np.array_equal(cpu(policy.params), start)
    assert np.abs(got_values - exact["values"]).max() <= twin.FACTOR * d_value
    assert np.abs(got_logp - exact["logp"][np.arange(len(rows)), got_actions]).max() <= twin.FACTOR * d_logp


@pytest.mark.parametrize("with_norm", [True, False])
def test_advantages_and_returns_are_compute_returns(hip_lib, with_norm):
    """mappo_advantages on the record of a real rollout with episode ends in it (horizon 3, T = 8) against the twin's float64
    restatement of compute_returns and of R_MAPPO.train's normalisation, with a ValueNorm state of a run in progress and with none"""
    layout, n, t = "cramped_room", 33, 8
    policy = CnnPolicy.from_module(cnn_twin.make_module(layout, "trained"), device=DEV)
    env = OvercookedMadrona(layout, n, 0, horizon=3)
    record, _ = env.rollout(policy, t, seed=17, first_step=0)
    value_norm = None
    if with_norm:
        value_norm = ValueNorm(DEV)
        value_norm.state.copy_(cuda(np.asarray(twin.STATE0, np.float32)))
    advantages, returns = mappo_advantages(record, value_norm, gamma=0.99, gae_lambda=0.95)
    arrays = [cpu(x) for x in (record.rewards, record.values, record.dones, record.next_done)]
    assert 0 < arrays[2].sum() < arrays[2].size and np.abs(arrays[0]).sum() >= 0
    cfg, state = twin.Config(), twin.STATE0 if with_norm else None
    exact = twin.compute_returns(*arrays, 0.99, 0.95, cfg, state)
    single = twin.compute_returns(*arrays, 0.99, 0.95, cfg, state, np.float32)
    for name, have, want, ref32 in (("advantages", cpu(advantages), exact[0], single[0]), ("returns", cpu(returns), exact[1], single[1])):
        d = max(twin.distance(ref32, want), float(np.abs(want).max()) * 2.0 ** -24)
        print(name, "with ValueNorm" if with_norm else "without", "measured / d:", twin.distance(have, want) / d, "d = %.2e" % d)
        assert have.shape == want.shape == (t, n, 2)
        assert twin.distance(have, want) <= twin.FACTOR * d, name
    # the masks: a world that finished between step k and k + 1 takes nothing across that boundary
    assert np.ptp(exact[1]) > 0
    env.close()


@pytest.mark.parametrize("layout, n", [("cramped_room", 33), ("asymmetric_advantages", 33), ("coordination_ring", 3)])
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, layout, n):
    """the update's forward pass is the act's on every layout shape, rows off 4-byte boundaries included: on unchanged parameters
    the ratio is exactly 1, and with the record's own values as returns (plain squared error) the value loss is exactly 0"""
    t = 2
    policy = CnnPolicy.from_module(cnn_twin.make_module(layout, "trained"), device=DEV)
    env = OvercookedMadrona(layout, n, 0, horizon=cnn_twin.HORIZON)
    record, ring = env.rollout(policy, t, seed=5, first_step=0)
    count = t * n * 2
    returns = record.values[:t].clone()
    indices = torch.arange(count, dtype=torch.int32, device=DEV).view(1, count)
    result = mappo_update(policy, MappoOptimizer(policy), record, ring, torch.ones_like(returns), returns, indices, value_norm=None,
                          use_huber_loss=False, use_clipped_value_loss=False)
    stats = cpu(result.stats)[0]
    assert stats[_lib.MAPPO_STATS.index("ratio")] == 1.0 and stats[_lib.MAPPO_STATS.index("clipfrac")] == 0.0
    assert stats[_lib.MAPPO_STATS.index("value_loss")] == 0.0 and stats[_lib.MAPPO_STATS.index("critic_grad_norm")] == 0.0
    assert stats[_lib.MAPPO_STATS.index("policy_loss")] == -1.0
    env.close()


def test_training_tool_runs_two_updates(hip_lib):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "overcooked_train_device.py")
    spec = importlib.util.spec_from_file_location("overcooked_train_device", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    seen = []
    history = tool.train("cramped_room", 33, 8, 2, seed=1, ppo_epoch=2, num_mini_batch=2, horizon=5, lr_decay=True, log=seen.append)
    assert len(history) == 2 == len(seen)
    assert [entry["optimizer_step"] for entry in history] == [4, 8] and history[1]["lr"] == 2.5e-4
    for entry in history:
        assert entry["episodes"] >= 33 and entry["mean_return"] is not None and entry["global_step"] == (entry["update"] + 1) * 8 * 33
        for name in _lib.MAPPO_STATS[:7]:
            assert np.isfinite(entry[name]), name
        assert 0.5 < entry["ratio"] < 1.5 and entry["dist_entropy"] > 0 and entry["critic_grad_norm"] > 0
    assert history[0]["value_loss"] != history[1]["value_loss"]


def test_refusals_change_nothing(hip_lib):
    fixed = chain_case()
    device = device_of(fixed)
    stats = torch.full((1, 8), 7.0, device=DEV)
    before = device.state()
    L = _lib.lib()
    w, h, p, f = twin.shape_of(fixed["layout"])
    count = len(fixed["batch"].ring)
    indices = cuda(fixed["indices"][:1])
    workspace = device.optimizer.workspace(indices.shape[1], 1)

    def call(hidden=64, width=indices.shape[1], size=count, flags=15, ws_bytes=None, params=None, state=True, ws_offset=0, stream=None):
        policy = _lib.MappoPolicyDesc(params or device.policy.params.data_ptr(), hidden, 0, w, h, f)
        opt = _lib.MappoOptimizerDesc(device.policy.params.data_ptr(), device.optimizer.exp_avg.data_ptr(), device.optimizer.exp_avg_sq.data_ptr(), 0)
        batch = _lib.MappoBatch(device.ring.data_ptr(), device.record.actions.data_ptr(), device.record.logprobs.data_ptr(),
                                device.record.values.data_ptr(), device.returns.data_ptr(), device.advantages.data_ptr(), size)
        cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, flags)
        return L.mrl_mappo_update(ctypes.byref(policy), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), 1, width, ctypes.byref(cfg),
                                  device.value_norm.state.data_ptr() if state else None, workspace.data_ptr() + ws_offset,
                                  workspace.numel() if ws_bytes is None else ws_bytes, stats.data_ptr(), None, 0,
                                  stream if stream is not None else torch.cuda.current_stream().cuda_stream)

    refused = {"hidden": call(hidden=32), "B == 0": call(width=0), "S == 0": call(size=0), "unknown flag": call(flags=16),
               "small workspace": call(ws_bytes=workspace.numel() - 16), "misaligned workspace": call(ws_offset=4),
               "misaligned params": call(params=device.policy.params.data_ptr() + 4), "no ValueNorm state": call(state=False)}
    assert L.mrl_mappo_update(None, None, None, None, 1, 1, None, None, None, 0, None, None, 0, None) == 1
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
    after = device.state()
    for name, value in before.items():
        same_bits(after[name], value, name)
    assert (cpu(stats) == 7.0).all() and device.optimizer.step == 0
    # a kitchen whose LDS image does not fit, as mrl_cnn_act refuses it
    out = ctypes.c_uint64(0)
    assert L.mrl_mappo_workspace_bytes(12, 5, 26, 64, 64, 1, ctypes.byref(out)) == 1
    # the Python ValueErrors that need GPU tensors
    good = dict(policy=device.policy, optimizer=device.optimizer, record=device.record, ring=device.ring, advantages=device.advantages,
                returns=device.returns, indices=indices)
    for name, bad in (("ring", device.ring.float()), ("ring", device.ring[:1]), ("advantages", device.advantages.double()),
                      ("advantages", device.advantages[:1]), ("returns", device.returns.cpu()), ("indices", indices.long()),
                      ("indices", indices[0]), ("optimizer", MappoOptimizer(CnnPolicy(w, h, f, device=DEV))), ("record", object())):
        with pytest.raises(ValueError):
            mappo_update(**{**good, name: bad})
    with pytest.raises(ValueError):
        mappo_update(**good, value_norm=object())
    assert device.optimizer.step == 0
    # K == 0 enqueues nothing
    mappo_update(**{**good, "indices": indices[:0]}, value_norm=device.value_norm)
    torch.cuda.synchronize()
    for name, value in before.items():
        same_bits(device.state()[name], value, name + " after K == 0")
