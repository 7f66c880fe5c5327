"""GPU: MAPPO's RECURRENT CNN actor-critic in the kitchens -- ``mrl_cnn_act``, ``mrl_rollout_cnn`` and ``mrl_mappo_update`` with
``MRL_CNN_RECURRENT`` through the Python binding against the float64 twin of tests/cnn_gru_twin.py, the closed loop rollout ->
``mappo_advantages`` -> ``mappo_update``, the C-level refusals and the plain path behind a recurrent call.

Cases and inputs: tests/cnn_gru_twin.py; their conditions are asserted by tests/test_cnn_gru_api.py.  Margins: d is, per kind of
number, the largest distance of the float32 CPU computation from the twin on the same inputs; the device must be within 8 x d.
Each test prints its ratios."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_gru_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd._mappo import _mappo_config  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (CnnGruPolicy, CnnGruRecord, CnnPolicy, CnnRecord, ExecMode, MappoOptimizer,  # noqa: E402
                                                         OvercookedSimulator, SimplecookedSimulator, ValueNorm, chunk_indices, cnn_act,
                                                         mappo_advantages, mappo_update, minibatch_indices)
from update_twin import clip_adam, clip_adam_torch, distance  # noqa: E402

DEV = torch.device("cuda", 0)
STAT = _lib.MAPPO_STATS.index
BUFFERS = _lib.CNN_RECORD_BUFFERS + ("h0_actor", "h0_critic")
CFG = twin.Config()


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(t):
    return (t.to_torch() if hasattr(t, "to_torch") else t).cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def make_sim(key, n, horizon=400):
    cls = SimplecookedSimulator if twin.KITCHENS[key] == "simplecooked" else OvercookedSimulator
    return cls(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **twin.layout_params(key, horizon))


def make_policy(key, n=None):
    w, h, p, f = twin.shape(key)
    policy = CnnGruPolicy(w, h, f, device=DEV)
    policy.params.copy_(cuda(twin.params_of(key)))
    if n is not None:
        policy.state(n, p)
    return policy


def marked_record(t, n, p, chunk):
    record = CnnGruRecord(t, n, p, DEV, chunk_length=chunk, logits=True)
    for name in BUFFERS:
        getattr(record, name).fill_(-3)
    return record


def arrays(record, policy):
    out = {name: cpu(getattr(record, name)) for name in BUFFERS}
    out["h_actor"], out["h_critic"] = cpu(policy.running.actor), cpu(policy.running.critic)
    return out


# ---------------------------------------------------------------- act

def run_act(key, n, seats, states, row, chunk=2, **kwargs):
    inputs = twin.act_inputs(key, n, states)
    policy, sim = make_policy(key, n), make_sim(key, n)
    sim.observation_world_major_tensor().to_torch().copy_(cuda(inputs["obs"]))
    sim.done_tensor().to_torch().copy_(cuda(inputs["done"]).view_as(sim.done_tensor().to_torch()))
    policy.running.actor.copy_(cuda(inputs["h_actor"]))
    policy.running.critic.copy_(cuda(inputs["h_critic"]))
    sim.action_tensor().to_torch().fill_(-7)
    record = marked_record(4, n, twin.shape(key)[2], chunk) if kwargs.pop("record", True) else None
    cnn_act(sim, policy, seats, record, row=row, seed=17, step=5, **kwargs)
    torch.cuda.synchronize()
    got = arrays(record, policy) if record is not None else {"h_actor": cpu(policy.running.actor), "h_critic": cpu(policy.running.critic)}
    got["ACTION"] = cpu(sim.action_tensor())[..., 0]
    sim.close()
    return inputs, got


@pytest.mark.parametrize("key, n, seats, states", [("k3x3p1", 3, (0,), "zero"), ("k3x3p1", 65, (0,), "nonzero"), ("cramped_room", 33, (0, 1), "nonzero"),
                                                   ("cramped_room", 33, (1,), "nonzero"), ("simple/1p", 65, (0,), "nonzero"),
                                                   ("k8x5p4", 33, (0, 1, 2, 3), "nonzero"), ("k8x5p4", 3, (0, 1, 2, 3), "zero")])
def test_act_matches_the_twin(hip_lib, key, n, seats, states):
    p, params, pick, row, chunk = twin.shape(key)[2], twin.params_of(key), np.array(seats), 2, 2
    others = [s for s in range(p) if s not in seats]
    inputs, got = run_act(key, n, seats, states, row)
    rows = inputs["obs"][:, pick].reshape((-1,) + inputs["obs"].shape[2:])
    h_actor, h_critic = (inputs[k][:, pick].reshape(-1, twin.HIDDEN) for k in ("h_actor", "h_critic"))
    mask = np.repeat(1.0 - (inputs["done"] != 0), len(seats))
    u = twin.draws(17, 5, n, p).reshape(n, p)[:, pick].reshape(-1)
    exact, d = twin.act(params, key, rows, h_actor, h_critic, mask, u), twin.act_margins(params, key, rows, h_actor, h_critic, mask)
    acted = got["actions"][row][:, pick].reshape(-1)
    decided = ~twin.near_boundary(exact["cdf"], u)
    assert np.array_equal(acted[decided], exact["actions"][decided])
    ratios = {"values": np.abs(got["values"][row][:, pick].reshape(-1) - exact["values"]).max() / d["values"],
              "logp": np.abs(got["logprobs"][row][:, pick].reshape(-1) - exact["logp"][np.arange(len(rows)), acted]).max() / d["logp"],
              "logits": np.abs(got["logits"][row][:, pick].reshape(-1, 6) - exact["logits"]).max() / d["logits"]}
    for name in ("h_actor", "h_critic"):
        ratios[name] = np.abs(got[name][:, pick].reshape(-1, twin.HIDDEN) - exact[name]).max() / d[name]
        same_bits(got[name][:, others], inputs[name][:, others], f"the other seats' rows of {name}")
        # a row that starts a chunk writes h0 with the incoming state, before the mask, bit for bit
        same_bits(got["h0_" + name[2:]][row // chunk][:, pick], inputs[name][:, pick], "h0")
    print((key, n, seats, states), "measured / d:", {k: round(float(v), 2) for k, v in ratios.items()})
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (name, ratio)
    assert np.array_equal(got["ACTION"][pick].T.reshape(-1), acted) and (got["ACTION"][others] == -7).all()
    for name in BUFFERS:  # nothing outside the act's own cells moves
        touched = np.zeros(got[name].shape, bool)
        if name != "next_done":
            touched[{"rewards": row - 1, "h0_actor": row // chunk, "h0_critic": row // chunk}.get(name, row)][:, pick] = True
        assert (got[name][~touched] == -3).all(), name
    # a row inside a chunk leaves h0's bytes alone and gives the same outputs; a second run gives the same bits
    _, inside = run_act(key, n, seats, states, 1)
    assert (inside["h0_actor"] == -3).all() and (inside["h0_critic"] == -3).all()
    same_bits(inside["values"][1], got["values"][row], "values at a row inside a chunk")
    same_bits(inside["h_actor"], got["h_actor"], "h_actor at a row inside a chunk")
    _, again = run_act(key, n, seats, states, row)
    for name, array in got.items():
        same_bits(again[name], array, f"{name} of a second run")


def test_closing_act_and_act_without_a_record(hip_lib):
    key, n = "cramped_room", 33
    inputs, closing = run_act(key, n, None, "nonzero", 4, value_only=True)
    for name in ("h_actor", "h_critic"):
        same_bits(closing[name], inputs[name], f"{name} behind the closing act")
    assert (closing["h0_actor"] == -3).all() and (closing["h0_critic"] == -3).all() and (closing["values"][4] != -3).all()
    _, full = run_act(key, n, None, "nonzero", 2)
    inputs, bare = run_act(key, n, None, "nonzero", 0, record=False)
    same_bits(bare["h_critic"], inputs["h_critic"], "the critic's state without a record")
    same_bits(bare["h_actor"], full["h_actor"], "the actor's state without a record")
    same_bits(bare["ACTION"], full["ACTION"], "ACTION without a record")


# ---------------------------------------------------------------- rollout

@pytest.mark.parametrize("key", ["cramped_room", "simple/1p"])
def test_rollout_equals_acts_and_steps_and_chains(hip_lib, key):
    n, L, p = 33, 2, twin.shape(key)[2]
    T = 4 * L

    def fresh():
        sim = make_sim(key, n, horizon=5)  # episodes end inside the window
        ring = torch.zeros((T + 1,) + tuple(sim.observation_world_major_tensor().to_torch().shape), dtype=torch.int8, device=DEV)
        return sim, make_policy(key, n), CnnGruRecord(T, n, p, DEV, chunk_length=L, logits=True), ring

    sim, policy, whole, ring = fresh()
    sim.rollout_cnn(policy, whole, ring, seed=9, first_step=3)
    torch.cuda.synchronize()
    want = arrays(whole, policy)
    assert want["dones"].any() and not want["dones"].all() and want["h0_actor"][1:].any()
    sim.close()
    # act + step, one by one
    sim, policy, record, _ = fresh()
    for k in range(T):
        cnn_act(sim, policy, None, record, row=k, seed=9, step=3 + k)
        sim.step()
    cnn_act(sim, policy, None, record, row=T, seed=9, step=3 + T, value_only=True)
    torch.cuda.synchronize()
    for name, array in arrays(record, policy).items():
        same_bits(array, want[name], f"{name}: act + step against the rollout")
    sim.close()
    # two rollouts of 2 L with the states carried against one of 4 L
    sim, policy, _, _ = fresh()
    halves = []
    for part in range(2):
        half = CnnGruRecord(2 * L, n, p, DEV, chunk_length=L, logits=True)
        sim.rollout_cnn(policy, half, ring[:2 * L + 1], seed=9, first_step=3 + part * 2 * L)
        torch.cuda.synchronize()
        halves.append(arrays(half, policy))
    for name in ("actions", "logprobs", "rewards", "dones", "logits", "h0_actor", "h0_critic"):
        same_bits(np.concatenate([halves[0][name], halves[1][name]]), want[name], f"{name}: two rollouts against one")
    same_bits(np.concatenate([halves[0]["values"][:-1], halves[1]["values"]]), want["values"], "values: two rollouts against one")
    for name in ("h_actor", "h_critic", "next_done"):
        same_bits(halves[1][name], want[name], f"{name}: two rollouts against one")
    sim.close()


# ---------------------------------------------------------------- update

class Device:
    """A recurrent policy, its optimizer, a ValueNorm and a batch (as a record and a ring) on the GPU."""

    def __init__(self, key, params, batch):
        self.policy = make_policy(key)
        self.policy.params.copy_(cuda(np.asarray(params, np.float32)))
        self.optimizer = MappoOptimizer(self.policy, lr=CFG.lr, critic_lr=CFG.critic_lr, betas=(CFG.beta1, CFG.beta2), eps=CFG.eps)
        t, n, p = batch.actions.shape
        self.record = record = CnnGruRecord(t, n, p, DEV, chunk_length=batch.chunk_length)
        for name in ("actions", "logprobs", "dones", "h0_actor", "h0_critic"):
            getattr(record, name).copy_(cuda(getattr(batch, name)))
        record.values[:t].copy_(cuda(batch.values))
        self.ring = cuda(batch.obs)
        self.advantages, self.returns = cuda(batch.advantages), cuda(batch.returns)
        self.value_norm = ValueNorm(DEV, beta=0.99999, epsilon=1e-5)

    def update(self, indices):
        result = mappo_update(self.policy, self.optimizer, self.record, self.ring, self.advantages, self.returns, cuda(indices),
                              value_norm=self.value_norm, clip_param=CFG.clip_param, entropy_coef=CFG.entropy_coef,
                              value_loss_coef=CFG.value_loss_coef, max_grad_norm=CFG.max_grad_norm, huber_delta=CFG.huber_delta,
                              use_huber_loss=CFG.huber, use_clipped_value_loss=CFG.clipped_value, use_max_grad_norm=CFG.clip_grads,
                              stats=True, grads=True)
        return cpu(result.stats), cpu(result.grads)

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


# (kitchen, L, Bc): every chunk length at the smallest kitchen, the overlay's kitchen at both ends, and 8193 chunks, the smallest
# row that gives one workgroup two tiles (257 tiles over 256 workgroups)
UPDATE_CASES = [("k3x3p1", L, 33) for L in twin.CHUNKS] + [("cramped_room", 2, 33), ("cramped_room", 10, 33), ("k8x5p4", 1, 33), ("k8x5p4", 16, 33),
                                                           ("k3x3p1", 2, 8193)]


@functools.lru_cache(maxsize=None)
def twin_rows(case):
    params, batch, ids = twin.update_case(*case)
    return twin.row(params, case[0], batch, ids[0], CFG), twin.row(params, case[0], batch, ids[0], CFG, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def stat_margins(key):
    """d of every scalar stat, pooled over the kitchen's own cases (one row's own distance bounds nothing)"""
    rows = [twin_rows(case) for case in UPDATE_CASES if case[0] == key]
    return {name: max(abs(single["stats"][name] - exact["stats"][name]) for exact, single in rows) for name in twin.STATS}


@pytest.mark.parametrize("case", UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_stats_and_step_match_the_twin(hip_lib, case):
    gradient_stats_and_step_match_the_twin(case, twin_rows(case), stat_margins(case[0]))


def gradient_stats_and_step_match_the_twin(case, rows, stat_d):
    """one row of a case on the device against ``rows``, the twin's and the float32 CPU row; ``stat_d``: d of every scalar stat
    (also for tests/test_gpu_cnn_gru_shapes.py)"""
    key, L, Bc = case
    params, batch, ids = twin.update_case(*case)
    exact, single = rows
    device = Device(key, params, batch)
    stats, grads = device.update(ids)
    after = device.state()
    d_grad = distance(single["grad"], exact["grad"])
    ratios = {"grad": distance(grads[0], exact["grad"]) / d_grad}
    for name in twin.STATS:
        if name != "clipfrac":
            ratios[name] = abs(float(stats[0][STAT(name)]) - exact["stats"][name]) / stat_d[name]
    d_state = np.maximum(np.abs(single["state"] - exact["state"]), np.abs(exact["state"]) * 2.0 ** -24)
    ratios["value_norm"] = float((np.abs(after["value_norm"] - exact["state"]) / d_state).max())
    print(case, "measured / d:", {k: round(float(v), 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d_grad)
    count = round(exact["stats"]["clipfrac"] * Bc * L)
    assert 0 < count < Bc * L and stats[0][STAT("clipfrac")] == np.float32(np.float64(count) / np.float64(Bc * L))
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (case, name, ratio)
    # the stepped parameters and moments, teacher-forced on the device's own gradient: both nets' clip and Adam from zero moments
    grad, na, step_ratios = grads[0].astype(np.float64), twin.actor_size(key), {}
    for net, (sl, lr) in enumerate(((slice(0, na), CFG.lr), (slice(na, None), CFG.critic_lr))):
        zeros = np.zeros(len(grad[sl]))
        _, p32, m32, v32 = clip_adam_torch(params[sl], zeros, zeros, grad[sl], 0, CFG.max_grad_norm, lr, CFG, torch.float32)
        _, p, m, v = clip_adam(params[sl], zeros, zeros, grad[sl], 0, CFG.max_grad_norm, lr, CFG)
        for name, want, one in (("params", p, p32), ("exp_avg", m, m32), ("exp_avg_sq", v, v32)):
            d = max(distance(one, want), float(np.abs(want).max()) * 2.0 ** -24)
            step_ratios[f"{name}[{net}]"] = distance(after[name][sl], want) / d
    print(case, "the step, measured / d:", {k: round(r, 2) for k, r in step_ratios.items()})
    for name, ratio in step_ratios.items():
        assert ratio <= twin.FACTOR, (case, name, ratio)
    # a second run gives the same bits
    again = Device(key, params, batch)
    stats2, grads2 = again.update(ids)
    same_bits(stats2, stats, "stats of a second run")
    same_bits(grads2, grads, "gradients of a second run")
    for name, value in after.items():
        same_bits(again.state()[name], value, f"{name} of a second run")


def test_rows_in_one_call_equal_calls_of_one_row(hip_lib):
    key = "cramped_room"
    params, batch, ids = twin.update_case(key, 2, 33, rows=3)
    together, one_by_one = Device(key, params, batch), Device(key, params, batch)
    stats, grads = together.update(ids)
    rows = [one_by_one.update(ids[k:k + 1]) for k in range(3)]
    same_bits(np.concatenate([r[0] for r in rows]), stats, "stats")
    same_bits(np.concatenate([r[1] for r in rows]), grads, "gradients")
    for name, value in together.state().items():
        same_bits(one_by_one.state()[name], value, name)
    assert together.optimizer.step == 3 and not np.array_equal(grads[0], grads[1])


def test_every_mask_zero_leaves_weight_hh_without_gradient(hip_lib):
    key = "cramped_room"
    params, batch, ids = twin.update_case(key, 10, 33)
    stats, grads = Device(key, params, batch._replace(dones=np.ones_like(batch.dones))).update(ids)
    keep = np.ones(grads.shape[1], bool)
    for sl in twin.whh_slices(key):
        assert (grads[0][sl] == 0.0).all()
        keep[sl] = False
    assert np.isfinite(grads).all() and (grads[0][keep] != 0).mean() > 0.9


@pytest.mark.parametrize("key, chunk", [("cramped_room", 1), ("cramped_room", 2), ("k8x5p4", 2), ("simple/1p", 10)])
def test_unchanged_parameters_give_the_records_values_and_log_probs(hip_lib, key, chunk):
    """the update's three forward passes are the act's: on unchanged parameters over a real rollout the ratio is exactly 1, and with
    the record's own values as returns (plain squared error) the value loss and the critic's gradient are exactly 0"""
    n, t, p = 33, 2 * chunk, twin.shape(key)[2]
    sim, policy = make_sim(key, n, horizon=7), make_policy(key, n)
    ring = torch.zeros((t + 1,) + tuple(sim.observation_world_major_tensor().to_torch().shape), dtype=torch.int8, device=DEV)
    sim.rollout_cnn(policy, CnnGruRecord(t, n, p, DEV, chunk_length=chunk), ring, seed=4, first_step=0)  # non-zero h0 for the next one
    record = CnnGruRecord(t, n, p, DEV, chunk_length=chunk)
    sim.rollout_cnn(policy, record, ring, seed=5, first_step=t)
    assert cpu(record.h0_actor)[0].any() and (chunk < 2 or cpu(record.dones).any())
    returns = record.values[:t].clone()
    indices = chunk_indices(record, 1, 1, device=DEV)
    assert indices.shape == (1, 2 * n * p)
    result = mappo_update(policy, MappoOptimizer(policy), record, ring, torch.ones_like(returns), returns, indices, value_norm=None,
                          use_huber_loss=False, use_clipped_value_loss=False, stats=True, grads=True)
    stats, grads = cpu(result.stats)[0], cpu(result.grads)[0]
    sim.close()
    assert stats[STAT("ratio")] == 1.0 and stats[STAT("clipfrac")] == 0.0
    assert stats[STAT("value_loss")] == 0.0 and stats[STAT("critic_grad_norm")] == 0.0
    assert not grads[twin.actor_size(key):].any() and grads[:twin.actor_size(key)].any()


# ---------------------------------------------------------------- refusals, closed loop

def captured(call):
    """the return code of ``call(stream)`` on a capturing stream"""
    side, scratch = torch.cuda.Stream(), torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            rc = call(torch.cuda.current_stream().cuda_stream)
            scratch.add_(0)  # (a capture must record something)
    torch.cuda.synchronize()
    return rc


def test_c_level_refusals_change_nothing(hip_lib):
    key, n = "cramped_room", 3
    w, h, p, f = twin.shape(key)
    L, sim, policy = _lib.lib(), make_sim(key, n), make_policy(key, n)
    record = marked_record(4, n, p, 2)
    ring = torch.zeros((5,) + tuple(sim.observation_world_major_tensor().to_torch().shape), dtype=torch.int8, device=DEV)
    space = torch.zeros(int(L.mrl_cnn_bank_workspace_bytes(n, p, 1)) + 256, dtype=torch.uint8, device=DEV)
    state_before = policy.running.actor.clone()
    ref = lambda struct: _lib.base_ref(struct) if struct is not None else None  # noqa: E731

    def act(desc, rec, flags=0, stream=None):
        return L.mrl_cnn_act(sim._handle, 3, ref(desc), ref(rec), 0, 1, 0, flags, space.data_ptr(), space.numel(), stream)

    def rollout(desc, rec, flags=0, stream=None):
        return L.mrl_rollout_cnn(sim._handle, 3, ref(desc), ref(rec), ring.data_ptr(), 1, 0, stream)

    good, r = policy.desc(), record.struct
    gru_record = lambda h0a, h0c, chunk: _lib.CnnGruRecordDesc(r.base, h0a, h0c, chunk)  # noqa: E731
    bad = [(_lib.CnnGruPolicyDesc(good.base, None, good.h_critic), r), (_lib.CnnGruPolicyDesc(good.base, good.h_actor, good.h_critic + 2), r),
           (good, gru_record(r.h0_actor, r.h0_critic, 0)), (good, gru_record(r.h0_actor, r.h0_critic, 3)),
           (good, gru_record(None, r.h0_critic, 2)), (good, gru_record(r.h0_actor + 1, r.h0_critic, 2))]
    for call in (act, rollout):
        for desc, rec in bad:
            assert call(desc, rec) == _lib.MRL_ERR_INVALID
        assert captured(lambda stream: call(good, r, stream=stream)) == _lib.MRL_ERR_INVALID
    assert rollout(good, None) == _lib.MRL_ERR_INVALID
    assert act(good, r, flags=_lib.CNN_RECURRENT) == _lib.MRL_ERR_INVALID  # never a bit of the act's own flags
    # the banks refuse the bit
    bank = _lib.CnnBankDesc(policy.params.data_ptr(), 1, policy.num_params, 64, _lib.CNN_RECURRENT)
    ids = torch.zeros((n, p), dtype=torch.int32, device=DEV)
    plain_record = ctypes.cast(ctypes.pointer(r), ctypes.POINTER(_lib.CnnRecordDesc))
    assert L.mrl_cnn_act_bank(sim._handle, 3, ctypes.byref(bank), ids.data_ptr(), plain_record, None, 0, 1, 0, 0, space.data_ptr(),
                              space.numel(), None) == _lib.MRL_ERR_INVALID
    assert L.mrl_rollout_cnn_bank(sim._handle, 3, ctypes.byref(bank), ids.data_ptr(), None, None, plain_record, None, ring.data_ptr(), 1, 0,
                                  space.data_ptr(), space.numel(), None) == _lib.MRL_ERR_INVALID
    torch.cuda.synchronize()
    same_bits(cpu(policy.running.actor), cpu(state_before), "the state behind refused calls")
    for name in BUFFERS:
        assert (cpu(getattr(record, name)) == -3).all(), name
    assert act(good, r) == _lib.MRL_OK  # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert (cpu(record.values)[0] != -3).all()
    sim.close()


def test_c_level_update_refusals_change_nothing(hip_lib):
    key = "cramped_room"
    params, batch, ids = twin.update_case(key, 2, 33)
    device = Device(key, params, batch)
    L, before, policy, record = _lib.lib(), device.state(), device.policy, device.record
    count = record.num_steps * record.num_worlds * record.num_players
    (entry, _), shape, make_batch, obs = policy._mappo_batch(record, device.ring, count)
    opt = _lib.MappoOptimizerDesc(policy.params.data_ptr(), device.optimizer.exp_avg.data_ptr(), device.optimizer.exp_avg_sq.data_ptr(), 0)
    cfg = _mappo_config(device.optimizer, None, 0.2, 0.01, 1.0, 10.0, 10.0, True, True, True)
    indices, stats = cuda(ids), torch.full((1, 8), -3.0, device=DEV)
    workspace = torch.zeros(device.optimizer.workspace_bytes(33, 1) // 4, dtype=torch.float32, device=DEV)
    plain = (obs.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(), device.returns.data_ptr(),
             device.advantages.data_ptr(), count)

    def call(width=33, stream=None, **changes):
        struct = make_batch(*plain)
        for field, value in changes.items():
            setattr(struct, field, value)
        return entry(_lib.base_ref(shape), ctypes.byref(opt), _lib.base_ref(struct), indices.data_ptr(), 1, width, ctypes.byref(cfg), None,
                     workspace.data_ptr(), workspace.numel() * 4, stats.data_ptr(), None, 0, stream)

    for changes in ({"h0_actor": None}, {"dones": None}, {"h0_critic": record.h0_critic.data_ptr() + 2}, {"chunk_length": 0},
                    {"chunk_length": _lib.CNN_GRU_MAX_CHUNK + 1}, {"chunk_length": 3}, {"num_worlds": record.num_worlds + 1},
                    {"width": count // 2 + 1}):  # the last: more chunk ids in a row than the batch has chunks
        assert call(**changes) == _lib.MRL_ERR_INVALID, changes
    assert captured(lambda stream: call(stream=stream)) == _lib.MRL_ERR_INVALID
    bank_opt = _lib.MappoBankOptimizerDesc(policy.params.data_ptr(), device.optimizer.exp_avg.data_ptr(), device.optimizer.exp_avg_sq.data_ptr(),
                                           policy.num_params * 4, 1, 0, 1, 0)
    assert L.mrl_mappo_bank_update(_lib.base_ref(shape), ctypes.byref(bank_opt), _lib.base_ref(make_batch(*plain)), indices.data_ptr(), 1, 33,
                                   ctypes.byref(cfg), None, workspace.data_ptr(), workspace.numel() * 4, None, None, 0, None) == _lib.MRL_ERR_INVALID
    torch.cuda.synchronize()
    for name, value in device.state().items():
        same_bits(value, before[name], f"{name} behind refused updates")
    assert (cpu(stats) == -3).all()
    assert call() == _lib.MRL_OK
    torch.cuda.synchronize()
    assert (cpu(stats)[0, :7] != -3).all() and not np.array_equal(device.state()["params"], before["params"])


def test_training_tool_twice_and_the_agent_owns_its_state(hip_lib):
    import sys
    sys.path.insert(0, str(__import__("pathlib").Path(__file__).resolve().parents[1] / "tools"))
    import overcooked_train_device as tool
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CnnPolicyAgent
    runs = []
    for _ in range(2):
        final = {}
        history = tool.train("simple", 33, 4, 2, seed=1, ppo_epoch=2, horizon=7, game="simplecooked", recurrent=True, data_chunk_length=2, final=final)
        assert history[-1]["optimizer_step"] == 4 and np.isfinite(final["params"].numpy()).all()
        runs.append(final["params"].numpy())
    same_bits(runs[0], runs[1], "the parameters of two runs of the training tool")
    # the agent binds its own state for its act and puts back what the caller had bound
    env = tool.make_env("simplecooked", "simple", 33, 7)
    _, p, h, w, f = env.static_world_major_observations.shape
    policy = CnnGruPolicy(w, h, f, device=DEV)
    policy.params.copy_(torch.from_numpy(runs[0]))
    mine = policy.state(33, p)
    mine.actor.fill_(0.5)
    agent = CnnPolicyAgent(env, policy, seed=3)
    agent.get_action()
    torch.cuda.synchronize()
    assert policy.running is mine and (cpu(mine.actor) == 0.5).all()
    assert cpu(agent.state.actor)[:, agent.seat].any() and not cpu(agent.state.critic).any()
    env.close()


def test_closed_loop_and_the_plain_path_behind_it(hip_lib):
    key, n, L = "cramped_room", 33, 2
    w, h, p, f = twin.shape(key)
    T = 2 * L

    def plain_run():
        """a plain act and a plain update on fixed inputs: their bits must not depend on what ran before"""
        torch.manual_seed(3)
        policy = CnnPolicy(w, h, f, device=DEV)
        policy.params.copy_(torch.randn(policy.num_params) * 0.05)
        sim = make_sim(key, n)
        sim.observation_world_major_tensor().to_torch().copy_(cuda(twin.observations(key, (n, p), 77)))
        record = CnnRecord(T, n, p, DEV, logits=True)
        ring = cuda(twin.observations(key, (T + 1, n, p), 78))
        cnn_act(sim, policy, None, record, row=0, seed=2, step=0)
        record.logprobs.normal_(-1.5, 0.1)
        record.actions.random_(0, 6)
        advantages, returns = torch.randn(T, n, p, device=DEV), torch.randn(T, n, p, device=DEV)
        result = mappo_update(policy, MappoOptimizer(policy), record, ring, advantages, returns, minibatch_indices(T * n * p, 2, 1, device=DEV),
                              stats=True, grads=True)
        out = (cpu(record.values), cpu(record.logits), cpu(result.stats), cpu(result.grads), cpu(policy.params))
        sim.close()
        return out

    before = plain_run()
    sim, policy = make_sim(key, n, horizon=7), make_policy(key, n)
    optimizer, value_norm = MappoOptimizer(policy), ValueNorm(DEV)
    record = CnnGruRecord(T, n, p, DEV, chunk_length=L, logits=True)
    ring = torch.zeros((T + 1,) + tuple(sim.observation_world_major_tensor().to_torch().shape), dtype=torch.int8, device=DEV)
    sim.rollout_cnn(policy, record, ring, seed=1, first_step=0)
    advantages, returns = mappo_advantages(record, value_norm)
    old = cpu(policy.params)
    result = mappo_update(policy, optimizer, record, ring, advantages.contiguous(), returns.contiguous(),
                          chunk_indices(record, 2, 2, device=DEV), value_norm=value_norm)
    assert np.isfinite(cpu(result.stats)).all() and optimizer.step == 4 and not np.array_equal(cpu(policy.params), old)
    logits = cpu(record.logits)[0]
    sim.rollout_cnn(policy, record, ring, seed=1, first_step=T)  # the next act reads the new parameters
    torch.cuda.synchronize()
    assert np.isfinite(cpu(record.logits)).all() and not np.array_equal(cpu(record.logits)[0], logits)
    sim.close()
    for got, want, name in zip(plain_run(), before, ("values", "logits", "stats", "grads", "params")):
        same_bits(got, want, f"the plain path's {name} behind recurrent calls")
