"""GPU: MAPPO's RECURRENT MLP actor-critic on the balance beam -- ``mrl_mlpbase_act``, ``mrl_rollout_mlpbase`` and
``mrl_mappo_mlp_update`` with ``MRL_MLPBASE_RECURRENT`` through the Python binding against the float64 twin of
tests/mlpbase_gru_twin.py, the closed loop rollout -> ``mappo_advantages`` -> ``mappo_update``, the C-level refusals and the plain
path behind a recurrent call.

Cases, seeds and inputs: tests/balance_gru_cases.py; their conditions are asserted by tests/test_balance_gru_api.py.
Margins: d is, per kind of number, the largest distance of the float32 CPU computation from the twin on the same inputs; the
device must be within 8 x d.  Each test prints its ratios."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import balance_gru_cases as cases  # noqa: E402
import balance_mappo_cases as plain_cases  # noqa: E402
import mlpbase_gru_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (MappoOptimizer, MlpBaseGruPolicy, MlpBaseGruRecord, MlpBaseGruState,  # noqa: E402
                                                         MlpBasePolicy, MlpBaseRecord, ValueNorm, chunk_indices, mappo_advantages,
                                                         mappo_update, minibatch_indices, mlpbase_act)

DEV = torch.device("cuda", 0)
STAT = _lib.MAPPO_STATS.index
RECORD_BUFFERS = _lib.MLPBASE_RECORD_BUFFERS + ("h0_actor", "h0_critic")


def cuda(array):
    return torch.from_numpy(np.array(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


def make_policy(layer_N, weights, worlds=None):
    policy = MlpBaseGruPolicy(layer_N=layer_N, device=DEV)
    policy.params.copy_(cuda(cases.params_of(layer_N, weights)))
    if worlds is not None:
        policy.state(worlds)
    return policy


def record_arrays(record):
    return {name: cpu(getattr(record, name)) for name in RECORD_BUFFERS if getattr(record, name) is not None}


def plant(env, policy, inputs):
    """the case's observations, DONE flags and states into the simulator and the policy's bound state"""
    env.static_observations.copy_(cuda(inputs["obs"]))
    env.static_dones.copy_(cuda(inputs["done"]).view_as(env.static_dones))
    policy.running.actor.copy_(cuda(inputs["h_actor"]))
    policy.running.critic.copy_(cuda(inputs["h_critic"]))


# ---------------------------------------------------------------- act

@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
@pytest.mark.parametrize("weights", cases.WEIGHTS)
@pytest.mark.parametrize("states", cases.STATES)
@pytest.mark.parametrize("n, seats", [(3, (0, 1)), (33, (0, 1)), (65, (0, 1)), (33, (1,))])
def test_act_matches_the_twin(hip_lib, oracle_lib, layer_N, weights, states, n, seats):
    inputs = cases.act_inputs(n, states)
    params = cases.params_of(layer_N, weights)
    d = cases.act_margins(layer_N, weights)
    seed, step, chunk = 17, 5, 2
    rows, h_actor, h_critic, mask = cases.act_twin_inputs(inputs, seats)
    u = cases.draws(seed, step, n, seats)
    exact = twin.act(params, rows, h_actor, h_critic, mask, u, layer_N)
    pick = np.array(seats)
    others = [s for s in (0, 1) if s not in seats]
    results = []
    for row in (2, 1, 2):  # a row that starts a chunk, one that does not, and the first again
        policy = make_policy(layer_N, weights, n)
        env = BalanceMadronaTorch(n, 0)
        plant(env, policy, inputs)
        env.static_actions.fill_(-7)
        record = MlpBaseGruRecord(4, n, 2, DEV, chunk_length=chunk, logits=True)
        for name in RECORD_BUFFERS:
            getattr(record, name).fill_(-3)
        env.act(policy, players=seats, record=record, row=row, seed=seed, step=step)
        torch.cuda.synchronize()
        got, actions = record_arrays(record), cpu(env.static_actions)[..., 0]
        new = {"h_actor": cpu(policy.running.actor), "h_critic": cpu(policy.running.critic)}
        results.append((got, actions, new))
        env.close()
        if row != 2 or len(results) > 1:
            continue
        values, logp, logits = got["values"][row][:, pick].reshape(-1), got["logprobs"][row][:, pick].reshape(-1), got["logits"][row][:, pick].reshape(-1, 4)
        acted = got["actions"][row][:, pick].reshape(-1)
        decided = ~twin.near_boundary(exact["cdf"], u)
        assert decided.mean() > 0.9
        assert np.array_equal(acted[decided], exact["actions"][decided])
        ratios = {"values": np.abs(values - exact["values"]).max() / d["values"],
                  "logp": np.abs(logp - exact["logp"][np.arange(len(rows)), acted]).max() / d["logp"],
                  "logits": np.abs(logits - exact["logits"]).max() / d["logits"]}
        for name in ("h_actor", "h_critic"):
            assert np.isfinite(new[name]).all()
            ratios[name] = np.abs(new[name][:, pick].reshape(-1, twin.HIDDEN) - exact[name]).max() / d[name]
            same_bits(new[name][:, others], inputs[name][:, others], f"the other seats' rows of {name}")
        print((layer_N, weights, states, n, seats), "measured / d:", {k: round(float(v), 2) for k, v in ratios.items()})
        for name, ratio in ratios.items():
            assert ratio <= twin.FACTOR, (name, ratio)
        assert np.array_equal(actions[pick].T.reshape(-1), acted) and (actions[others] == -7).all()
        for name, array in got.items():
            touched = np.zeros(array.shape, bool)
            if name == "rewards":
                touched[row - 1][:, pick] = True
            elif name in ("h0_actor", "h0_critic"):
                touched[row // chunk][:, pick] = True
            elif name != "next_done":
                touched[row][:, pick] = True
            assert (array[~touched] == -3).all(), name
        # h0 holds the incoming state, before the mask, bit for bit
        same_bits(got["h0_actor"][row // chunk][:, pick], inputs["h_actor"][:, pick], "h0_actor")
        same_bits(got["h0_critic"][row // chunk][:, pick], inputs["h_critic"][:, pick], "h0_critic")
        same_bits(got["obs"][row][:, pick], np.ascontiguousarray(inputs["obs"].transpose(1, 0, 2))[:, pick], "record.obs")
        assert np.array_equal(got["dones"][row][:, pick] != 0, np.repeat(inputs["done"][:, None] != 0, len(pick), axis=1))
    # row 1 starts no chunk: h0 keeps every byte; the outputs are those of row 2, in row 1
    middle = results[1][0]
    assert (middle["h0_actor"] == -3).all() and (middle["h0_critic"] == -3).all()
    same_bits(middle["values"][1], results[0][0]["values"][2], "values at a row inside a chunk")
    same_bits(results[1][2]["h_actor"], results[0][2]["h_actor"], "h_actor at a row inside a chunk")
    # a second run gives the same bits
    for name, array in results[0][0].items():
        same_bits(results[2][0][name], array, f"{name} of a second run")
    same_bits(results[2][1], results[0][1], "ACTION of a second run")
    for name in ("h_actor", "h_critic"):
        same_bits(results[2][2][name], results[0][2][name], f"{name} of a second run")


def test_value_only_act_and_no_record(hip_lib, oracle_lib):
    n, t, layer_N, weights = 33, 2, 2, "trained"
    inputs = cases.act_inputs(n, "nonzero")
    policy = make_policy(layer_N, weights, n)
    env = BalanceMadronaTorch(n, 0)
    plant(env, policy, inputs)
    env.static_actions.fill_(-7)
    record = MlpBaseGruRecord(t, n, 2, DEV, chunk_length=1)
    for name in ("h0_actor", "h0_critic"):
        getattr(record, name).fill_(-3)
    mlpbase_act(env.sim, policy, record=record, row=t, value_only=True)
    assert (cpu(env.static_actions) == -7).all()
    rows, h_actor, h_critic, mask = cases.act_twin_inputs(inputs, (0, 1))
    exact = twin.act(cases.params_of(layer_N, weights), rows, h_actor, h_critic, mask, np.zeros(2 * n), layer_N)
    d = cases.act_margins(layer_N, weights)
    ratio = np.abs(cpu(record.values)[t].reshape(-1) - exact["values"]).max() / d["values"]
    print("the closing value, measured / d:", round(float(ratio), 2))
    assert ratio <= twin.FACTOR
    # the closing act leaves both state tensors' bytes alone, and h0 too
    same_bits(cpu(policy.running.actor), inputs["h_actor"], "h_actor behind the value-only act")
    same_bits(cpu(policy.running.critic), inputs["h_critic"], "h_critic behind the value-only act")
    assert (cpu(record.h0_actor) == -3).all() and (cpu(record.h0_critic) == -3).all()
    assert not cpu(record.actions).any() and not cpu(record.logprobs).any() and not cpu(record.values)[:t].any()
    # without a record only the actor runs: ACTION and h_actor change, h_critic does not
    env.act(policy, seed=3, step=0)
    assert ((cpu(env.static_actions) >= 0) & (cpu(env.static_actions) < 4)).all()
    same_bits(cpu(policy.running.critic), inputs["h_critic"], "h_critic behind an act without a record")
    ratio = np.abs(cpu(policy.running.actor).reshape(-1, twin.HIDDEN) - exact["h_actor"]).max() / d["h_actor"]
    assert 0 < ratio <= twin.FACTOR
    env.close()


# ---------------------------------------------------------------- rollout

SIM_TENSORS = ("static_observations", "static_rewards", "static_dones", "static_actions")


def test_rollout_equals_acts_and_steps_one_by_one(hip_lib):
    n, chunk, seed = 33, 2, 9
    t = 4 * chunk
    fused, single = BalanceMadronaTorch(n, 0), BalanceMadronaTorch(n, 0)
    policy, by_hand_policy = make_policy(2, "trained", n), make_policy(2, "trained", n)
    record = fused.rollout(policy, t, seed=seed, first_step=3, record=MlpBaseGruRecord(t, n, 2, DEV, chunk_length=chunk))
    by_hand = MlpBaseGruRecord(t, n, 2, DEV, chunk_length=chunk)
    for k in range(t):
        actions = single.act(by_hand_policy, record=by_hand, row=k, seed=seed, step=3 + k)
        single.n_step(actions)
    mlpbase_act(single.sim, by_hand_policy, record=by_hand, row=t, value_only=True)
    torch.cuda.synchronize()
    a, b = record_arrays(record), record_arrays(by_hand)
    for name in a:
        same_bits(a[name], b[name], name)
    for name in SIM_TENSORS:
        same_bits(cpu(getattr(fused, name)), cpu(getattr(single, name)), name)
    for name in ("actor", "critic"):
        same_bits(cpu(getattr(policy.running, name)), cpu(getattr(by_hand_policy.running, name)), f"the {name}'s state")
    # some worlds finish inside the window (an episode is two steps unless a seat walks off), and the states are alive
    assert a["dones"][1:].any() and not a["dones"][1:].all()
    assert not a["h0_actor"][0].any() and a["h0_actor"][1:].any() and a["h0_critic"][1:].any()
    # two rollouts of 2 L with the states carried equal one of 4 L
    halves, half_policy = BalanceMadronaTorch(n, 0), make_policy(2, "trained", n)
    first = record_arrays(halves.rollout(half_policy, 2 * chunk, seed=seed, first_step=3,
                                         record=MlpBaseGruRecord(2 * chunk, n, 2, DEV, chunk_length=chunk)))
    second = record_arrays(halves.rollout(half_policy, 2 * chunk, seed=seed, first_step=3 + 2 * chunk,
                                          record=MlpBaseGruRecord(2 * chunk, n, 2, DEV, chunk_length=chunk)))
    torch.cuda.synchronize()
    for name in ("actions", "logprobs", "rewards", "dones", "h0_actor", "h0_critic"):
        same_bits(np.concatenate([first[name], second[name]]), a[name], name)
    same_bits(np.concatenate([first["values"][:2 * chunk], second["values"]]), a["values"], "values")
    same_bits(np.concatenate([first["obs"][:2 * chunk], second["obs"]]), a["obs"], "obs")
    same_bits(first["values"][2 * chunk], second["values"][0], "the closing value is the next rollout's first")
    for name in SIM_TENSORS:
        same_bits(cpu(getattr(halves, name)), cpu(getattr(fused, name)), name)
    for name in ("actor", "critic"):
        same_bits(cpu(getattr(half_policy.running, name)), cpu(getattr(policy.running, name)), f"the {name}'s state behind two rollouts")
    for env in (fused, single, halves):
        env.close()


# ---------------------------------------------------------------- C-level refusals

def test_c_level_refusals_change_nothing(hip_lib):
    n, t = 5, 4
    env = BalanceMadronaTorch(n, 0)
    policy = make_policy(1, "trained", n)
    policy.running.actor.fill_(0.25)
    policy.running.critic.fill_(-0.25)
    record = MlpBaseGruRecord(t, n, 2, DEV, chunk_length=2, logits=True)
    for name in RECORD_BUFFERS:
        getattr(record, name).fill_(-3)
    env.static_actions.fill_(-7)
    L, handle = env.sim._L, env.sim._handle

    def snapshot():
        torch.cuda.synchronize()
        return (record_arrays(record), cpu(env.static_actions), cpu(policy.running.actor), cpu(policy.running.critic), cpu(policy.params))

    before = snapshot()

    def refused(desc, rec, what, rollout=False, row=0, flags=0):
        rec_ref = _lib.base_ref(rec) if rec is not None else None
        if rollout:
            rc = L.mrl_rollout_mlpbase(handle, 3, _lib.base_ref(desc), rec_ref, 1, 0, None)
        else:
            rc = L.mrl_mlpbase_act(handle, 3, _lib.base_ref(desc), rec_ref, row, 1, 0, flags, None)
        assert rc == _lib.MRL_ERR_INVALID, what
        after = snapshot()
        for x, y in zip(before[1:], after[1:]):
            same_bits(x, y, what)
        for name in before[0]:
            same_bits(before[0][name], after[0][name], f"{what}: {name}")

    def policy_desc(**changes):
        desc = policy.desc()
        for name, value in changes.items():
            setattr(desc, name, value)
        return desc

    def record_desc(**changes):
        base = _lib.MlpBaseRecordDesc.from_buffer_copy(record.struct.base)
        desc = _lib.MlpBaseGruRecordDesc(base, record.h0_actor.data_ptr(), record.h0_critic.data_ptr(), record.chunk_length)
        for name, value in changes.items():
            if name == "num_steps":
                desc.base.num_steps = value
            else:
                setattr(desc, name, value)
        return desc

    for rollout in (False, True):
        where = "rollout" if rollout else "act"
        refused(policy_desc(h_actor=None), record.struct, f"{where}: NULL h_actor", rollout)
        refused(policy_desc(h_critic=None), record.struct, f"{where}: NULL h_critic", rollout)
        refused(policy_desc(h_actor=policy.running.actor.data_ptr() + 2), record.struct, f"{where}: h_actor off a 4-byte boundary", rollout)
        refused(policy_desc(h_critic=policy.running.critic.data_ptr() + 1), record.struct, f"{where}: h_critic off a 4-byte boundary", rollout)
        refused(policy.desc(), record_desc(chunk_length=0), f"{where}: L = 0", rollout)
        refused(policy.desc(), record_desc(chunk_length=3), f"{where}: T % L != 0", rollout)
        refused(policy.desc(), record_desc(h0_actor=None), f"{where}: NULL h0_actor", rollout)
        refused(policy.desc(), record_desc(h0_critic=None), f"{where}: NULL h0_critic", rollout)
    refused(policy.desc(), None, "rollout: NULL record", rollout=True)
    # the recurrent bit is a bit of the policy's flags only: as a bit of the act's flags it is an unknown flag
    refused(policy.desc(), record.struct, "act: flag 16", flags=_lib.MLPBASE_RECURRENT)
    # the banks refuse the bit
    ids = torch.zeros((n, 2), dtype=torch.int32, device=DEV)
    workspace = torch.zeros(int(L.mrl_mlpbase_bank_workspace_bytes(n, 1)), dtype=torch.uint8, device=DEV)
    bank = _lib.MlpBaseBankDesc(policy.params.data_ptr(), 1, policy.params.numel(), 64, 1, _lib.MLPBASE_RECURRENT)
    plain_record = ctypes.cast(ctypes.pointer(record.struct), ctypes.POINTER(_lib.MlpBaseRecordDesc))
    assert L.mrl_mlpbase_act_bank(handle, 3, ctypes.byref(bank), ids.data_ptr(), plain_record, None, 0, 1, 0, 0, workspace.data_ptr(),
                                  workspace.numel(), None) == _lib.MRL_ERR_INVALID
    assert L.mrl_rollout_mlpbase_bank(handle, 3, ctypes.byref(bank), ids.data_ptr(), None, None, plain_record, None, 1, 0,
                                      workspace.data_ptr(), workspace.numel(), None) == _lib.MRL_ERR_INVALID
    after = snapshot()
    for x, y in zip(before[1:], after[1:]):
        same_bits(x, y, "the banks refuse the recurrent bit")
    for name in before[0]:
        same_bits(before[0][name], after[0][name], f"the banks refuse the recurrent bit: {name}")
    env.close()


def test_c_level_update_refusals_change_nothing(hip_lib, oracle_lib):
    fixed = cases.fixed_case((1, "trained", 33, 2, "default"))
    device = Device(fixed)
    policy, optimizer, record = device.policy, device.optimizer, device.record
    L = _lib.lib()
    indices = cuda(fixed["indices"])
    workspace = optimizer.workspace(33, 1)
    stats = torch.full((1, 8), -3.0, device=DEV)
    before = device.state()
    t, n, p = record.num_steps, record.num_worlds, record.num_players
    count = t * n * p
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 0)
    opt = _lib.MappoOptimizerDesc(policy.params.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), 0)
    shape = _lib.MlpBaseGruPolicyDesc(_lib.MlpBasePolicyDesc(policy.params.data_ptr(), 64, 1, _lib.MLPBASE_RECURRENT), None, None)

    def batch(**changes):
        plain = _lib.MappoMlpBatch(record.obs.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(),
                                   device.returns.data_ptr(), device.advantages.data_ptr(), changes.pop("size", count))
        made = _lib.MappoMlpGruBatch(plain, record.h0_actor.data_ptr(), record.h0_critic.data_ptr(), record.dones.data_ptr(), 2, n, p)
        for name, value in changes.items():
            setattr(made, name, value)
        return made

    def call(entry, batch_struct, opt_struct=opt):
        return entry(_lib.base_ref(shape), ctypes.byref(opt_struct), _lib.base_ref(batch_struct), indices.data_ptr(), 1, 33, ctypes.byref(cfg),
                     None, workspace.data_ptr(), workspace.numel(), stats.data_ptr(), None, 0, None)

    for what, made in (("NULL dones", batch(dones=None)), ("NULL h0_actor", batch(h0_actor=None)), ("NULL h0_critic", batch(h0_critic=None)),
                       ("dones off a 4-byte boundary", batch(dones=record.dones.data_ptr() + 2)), ("L = 0", batch(chunk_length=0)),
                       ("L above the maximum", batch(chunk_length=_lib.MLPBASE_GRU_MAX_CHUNK + 1)),
                       ("chunks inconsistent with the size", batch(size=count - p)), ("no worlds", batch(num_worlds=0)),
                       ("chunks inconsistent with the size", batch(chunk_length=3))):
        assert call(L.mrl_mappo_mlp_update, made) == _lib.MRL_ERR_INVALID, what
    too_many = L.mrl_mappo_mlp_update(_lib.base_ref(shape), ctypes.byref(opt), _lib.base_ref(batch()), indices.data_ptr(), 1, count // 2 + 1,
                                      ctypes.byref(cfg), None, workspace.data_ptr(), workspace.numel(), stats.data_ptr(), None, 0, None)
    assert too_many == _lib.MRL_ERR_INVALID  # more chunk ids a row than the batch has chunks
    bank_opt = _lib.MappoBankOptimizerDesc(policy.params.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(),
                                           4 * policy.params.numel(), 1, 0, 1, 0)
    assert call(L.mrl_mappo_mlp_bank_update, batch(), bank_opt) == _lib.MRL_ERR_INVALID
    torch.cuda.synchronize()
    for name, value in device.state().items():
        same_bits(value, before[name], name)
    assert (cpu(stats) == -3).all()
    assert call(L.mrl_mappo_mlp_update, batch()) == _lib.MRL_OK  # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert (cpu(stats)[0, :7] != -3).all() and not np.array_equal(device.state()["params"], before["params"])


# ---------------------------------------------------------------- update

class Device:
    """A recurrent policy, its optimizer, a ValueNorm and a batch (as a record) on the GPU."""

    def __init__(self, fixed, step=0):
        batch, layer_N = fixed["batch"], fixed["layer_N"]
        self.cfg = cfg = fixed["cfg"]
        self.policy = MlpBaseGruPolicy(layer_N=layer_N, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(fixed["params"], np.float32)))
        self.optimizer = MappoOptimizer(self.policy, lr=cfg.lr, critic_lr=cfg.critic_lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.optimizer.step = step
        t, n, p = np.asarray(batch.actions).shape
        self.record = record = MlpBaseGruRecord(t, n, p, DEV, chunk_length=batch.chunk_length)
        record.actions.copy_(cuda(batch.actions))
        record.logprobs.copy_(cuda(batch.logprobs))
        record.values[:t].copy_(cuda(batch.values))
        record.obs[:t].copy_(cuda(batch.obs))
        record.dones.copy_(cuda(batch.dones))
        record.h0_actor.copy_(cuda(batch.h0_actor))
        record.h0_critic.copy_(cuda(batch.h0_critic))
        self.advantages, self.returns = cuda(batch.advantages), cuda(batch.returns)
        self.value_norm = ValueNorm(DEV, beta=0.99999, epsilon=1e-5)
        self.value_norm.state.copy_(cuda(np.asarray(twin.STATE0, np.float32)))

    def update(self, indices):
        c = self.cfg
        result = mappo_update(self.policy, self.optimizer, self.record, None, self.advantages, self.returns, cuda(indices),
                              value_norm=self.value_norm if c.valuenorm else None, clip_param=c.clip_param, entropy_coef=c.entropy_coef,
                              value_loss_coef=c.value_loss_coef, max_grad_norm=c.max_grad_norm, huber_delta=c.huber_delta,
                              use_huber_loss=c.huber, use_clipped_value_loss=c.clipped_value, use_max_grad_norm=c.clip_grads,
                              stats=True, grads=True)
        return cpu(result.stats), cpu(result.grads)

    def state(self):
        return {"params": cpu(self.policy.params), "exp_avg": cpu(self.optimizer.exp_avg), "exp_avg_sq": cpu(self.optimizer.exp_avg_sq),
                "value_norm": cpu(self.value_norm.state)}


def check_row(what, got_stats, got_grad, fixed, stat_d):
    """One row of the device against the twin's: the gradient within 8 d of the case, every stat within 8 x its pooled d, clipfrac
    the twin's count / (Bc L)."""
    exact, single = fixed["twin"], fixed["f32"]
    samples = fixed["indices"].shape[1] * fixed["batch"].chunk_length
    d = twin.row_margins(exact, single)
    ratios = {"grad": twin.distance(got_grad, exact["grad"]) / d["grad"]}
    for name in twin.STATS:
        if name != "clipfrac":
            off = abs(float(got_stats[STAT(name)]) - exact["stats"][name])
            ratios[name] = off / stat_d[name] if stat_d[name] > 0 else (0.0 if off == 0 else float("inf"))
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d["grad"])
    count = round(exact["stats"]["clipfrac"] * samples)
    assert got_stats[STAT("clipfrac")] == np.float32(np.float64(count) / np.float64(samples)), what
    assert got_stats[STAT("reserved")] == 0
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_gradient_stats_and_step_match_the_twin(hip_lib, oracle_lib, case):
    fixed = cases.fixed_case(case)
    cfg, layer_N, params = fixed["cfg"], fixed["layer_N"], fixed["params"]
    device = Device(fixed)
    before = device.state()
    stats, grads = device.update(fixed["indices"])
    check_row(str(case), stats[0], grads[0], fixed, cases.stat_margins(case[0], case[1]))
    after = device.state()
    if cfg.valuenorm:
        state32 = fixed["f32"]["state"]
        d = np.maximum(np.abs(state32 - fixed["twin"]["state"]), np.abs(fixed["twin"]["state"]) * 2.0 ** -24)
        assert (np.abs(after["value_norm"] - fixed["twin"]["state"]) <= twin.FACTOR * d).all()
    else:
        same_bits(after["value_norm"], before["value_norm"], "the ValueNorm state without MRL_MAPPO_VALUENORM")
    assert device.optimizer.step == 1
    # the stepped parameters and moments, teacher-forced on the device's own gradient: both nets' clip and Adam from zero moments,
    # over the tensors the reference's optimizers see (fc_h has no gradient there)
    grad, na, keep = grads[0].astype(np.float64), twin.actor_size(layer_N), twin.used(layer_N)
    ratios = {}
    for net, (sl, lr) in enumerate(((slice(0, na), cfg.lr), (slice(na, None), cfg.critic_lr))):
        k = keep[sl]
        zeros = np.zeros(int(k.sum()))
        _, p32, m32, v32 = twin.clip_adam_torch(params[sl][k], zeros, zeros, grad[sl][k], 0, cfg.max_grad_norm, lr, cfg, torch.float32)
        _, p, m, v = twin.clip_adam(params[sl][k], zeros, zeros, grad[sl][k], 0, cfg.max_grad_norm, lr, cfg)
        for name, have, want, single in (("params", after["params"][sl][k], p, p32), ("exp_avg", after["exp_avg"][sl][k], m, m32),
                                         ("exp_avg_sq", after["exp_avg_sq"][sl][k], v, v32)):
            off, d = twin.distance(have, want), max(twin.distance(single, want), float(np.abs(want).max()) * 2.0 ** -24)
            ratios[f"{name}[{net}]"] = off / d if d > 0 else (0.0 if off == 0 else float("inf"))
    print(str(case), "the step, measured / d:", {k: round(r, 2) for k, r in ratios.items()})
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (case, name, ratio)
    assert not np.array_equal(after["params"], before["params"])
    # fc_h's parameters and moments keep their bits
    for sl in twin.fc_h_slices(layer_N):
        same_bits(after["params"][sl], before["params"][sl], "fc_h's parameters")
        assert not after["exp_avg"][sl].any() and not after["exp_avg_sq"][sl].any() and not grads[:, sl].any()
        assert before["params"][sl].any()
    # two runs give the same bits
    again = Device(fixed)
    stats2, grads2 = again.update(fixed["indices"])
    same_bits(stats2, stats, "stats of a second run")
    same_bits(grads2, grads, "gradients of a second run")
    for name, value in after.items():
        same_bits(again.state()[name], value, f"{name} of a second run")


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_rows_in_one_call_equal_calls_of_one_row(hip_lib, oracle_lib, layer_N):
    fixed = cases.fixed_case((layer_N, "trained", 33, 2, "default"), rows=3)
    together, one_by_one = Device(fixed), Device(fixed)
    stats, grads = together.update(fixed["indices"])
    rows = [one_by_one.update(fixed["indices"][k:k + 1]) for k in range(3)]
    same_bits(np.concatenate([r[0] for r in rows]), stats, "stats")
    same_bits(np.concatenate([r[1] for r in rows]), grads, "gradients")
    assert together.optimizer.step == one_by_one.optimizer.step == 3
    for name, value in together.state().items():
        same_bits(one_by_one.state()[name], value, name)
    assert not np.array_equal(grads[0], grads[1])


@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_every_mask_zero_leaves_weight_hh_without_gradient(hip_lib, oracle_lib, layer_N):
    fixed = dict(cases.fixed_case((layer_N, "trained", 33, 10, "default")))
    fixed["batch"] = fixed["batch"]._replace(dones=np.ones_like(fixed["batch"].dones))
    device = Device(fixed)
    stats, grads = device.update(fixed["indices"])
    for sl in twin.whh_slices(layer_N):
        assert (grads[0][sl] == 0.0).all()
    keep = np.ones(grads.shape[1], bool)
    for sl in twin.whh_slices(layer_N) + twin.fc_h_slices(layer_N):
        keep[sl] = False
    assert np.isfinite(grads).all() and (grads[0][keep] != 0).mean() > 0.9


@pytest.mark.parametrize("chunk", [1, 2, 10])
@pytest.mark.parametrize("layer_N", cases.LAYER_NS)
def test_recomputed_values_and_log_probs_are_the_records_bit_for_bit(hip_lib, layer_N, chunk):
    """the update's forward pass is the act's: on unchanged parameters over a real rollout the ratio is exactly 1, and with the
    record's own values as returns (plain squared error) the value loss and the critic's gradient are exactly 0"""
    n, t = 33, 2 * chunk
    policy = make_policy(layer_N, "trained", n)
    env = BalanceMadronaTorch(n, 0)
    warm = env.rollout(policy, chunk, seed=4, first_step=0, record=MlpBaseGruRecord(chunk, n, 2, DEV, chunk_length=chunk))  # non-zero h0
    record = env.rollout(policy, t, seed=5, first_step=chunk, record=MlpBaseGruRecord(t, n, 2, DEV, chunk_length=chunk))
    assert cpu(record.h0_actor)[0].any() and cpu(record.dones).any() and warm.num_steps == chunk
    optimizer = MappoOptimizer(policy)
    returns = record.values[:t].clone()
    advantages = torch.ones_like(returns)
    indices = chunk_indices(record, 1, 1, device=DEV)
    assert indices.shape == (1, 2 * n * 2)
    result = mappo_update(policy, optimizer, record, None, advantages, returns, indices, value_norm=None, use_huber_loss=False,
                          use_clipped_value_loss=False, stats=True, grads=True)
    stats, grads = cpu(result.stats)[0], cpu(result.grads)[0]
    assert stats[STAT("ratio")] == 1.0 and stats[STAT("clipfrac")] == 0.0
    assert stats[STAT("value_loss")] == 0.0 and stats[STAT("critic_grad_norm")] == 0.0
    assert not grads[twin.actor_size(layer_N):].any() and grads[:twin.actor_size(layer_N)].any()
    env.close()


def test_closed_loop_and_the_plain_path_behind_it(hip_lib, oracle_lib):
    """rollout -> mappo_advantages -> mappo_update -> the next act reads the new parameters; then, in the same process, one plain
    act and one plain update give the bits they give in a process that never ran a recurrent call (computed first)"""
    def plain_run():
        fixed = plain_cases.fixed_case((2, "trained", "synthetic", 65, "default"))
        policy = MlpBasePolicy(layer_N=2, device=DEV)
        policy.params.copy_(cuda(np.asarray(fixed["params"], np.float32)))
        env = BalanceMadronaTorch(33, 0)
        env.static_observations.copy_(cuda(plain_cases.act_inputs(33, "synthetic")))
        record = MlpBaseRecord(2, 33, 2, DEV, logits=True)
        env.act(policy, record=record, row=0, seed=7, step=1)
        acted = {name: cpu(getattr(record, name)) for name in _lib.MLPBASE_RECORD_BUFFERS}
        env.close()
        optimizer = MappoOptimizer(policy)
        batch = fixed["batch"]
        t, n, p = plain_cases.T, plain_cases.N, plain_cases.P
        record = MlpBaseRecord(t, n, p, DEV)
        record.actions.copy_(cuda(batch.actions).view(t, n, p))
        record.logprobs.copy_(cuda(batch.logprobs).view(t, n, p))
        record.values[:t].copy_(cuda(batch.values).view(t, n, p))
        record.obs[:t].copy_(cuda(batch.obs).view(t, n, p, 7))
        result = mappo_update(policy, optimizer, record, None, cuda(batch.advantages).view(t, n, p), cuda(batch.returns).view(t, n, p),
                              cuda(fixed["indices"]), stats=True, grads=True)
        return acted, cpu(result.stats), cpu(result.grads), cpu(policy.params)

    before = plain_run()
    n, chunk, t = 33, 2, 4
    env = BalanceMadronaTorch(n, 0)
    policy = make_policy(2, "trained", n)
    optimizer, value_norm = MappoOptimizer(policy), ValueNorm(DEV)
    record = env.rollout(policy, t, seed=1, record=MlpBaseGruRecord(t, n, 2, DEV, chunk_length=chunk))
    advantages, returns = mappo_advantages(record, value_norm)
    old = cpu(policy.params)
    result = mappo_update(policy, optimizer, record, None, advantages, returns, chunk_indices(record, 2, 3, device=DEV), value_norm=value_norm)
    stats = cpu(result.stats)
    assert stats.shape == (6, 8) and np.isfinite(stats).all() and optimizer.step == 6
    new = cpu(policy.params)
    assert not np.array_equal(new[twin.used(2)], old[twin.used(2)])
    # the next act reads the new parameters: its values are the twin's on them
    state = {"h_actor": cpu(policy.running.actor), "h_critic": cpu(policy.running.critic)}
    obs, done = cpu(env.static_observations), cpu(env.static_dones).reshape(-1)
    after = MlpBaseGruRecord(chunk, n, 2, DEV, chunk_length=chunk)
    env.act(policy, record=after, row=0, seed=2, step=t)
    inputs = {"obs": obs, "h_actor": state["h_actor"], "h_critic": state["h_critic"], "done": done}
    exact = twin.act(new, *cases.act_twin_inputs(inputs, (0, 1)), np.zeros(2 * n), 2)
    stale = twin.act(old, *cases.act_twin_inputs(inputs, (0, 1)), np.zeros(2 * n), 2)
    off = np.abs(cpu(after.values)[0].reshape(-1) - exact["values"]).max()
    d = twin.act_margins(new, *cases.act_twin_inputs(inputs, (0, 1)), 2)["values"]
    print("the act behind the update, measured / d:", round(float(off / d), 2))
    assert off <= twin.FACTOR * d and off < 0.01 * np.abs(stale["values"] - exact["values"]).max()
    env.close()
    behind = plain_run()
    for name in before[0]:
        same_bits(before[0][name], behind[0][name], f"the plain act's {name} behind a recurrent call")
    for x, y, name in zip(before[1:], behind[1:], ("stats", "grads", "params")):
        same_bits(x, y, f"the plain update's {name} behind a recurrent call")


def test_training_tool_runs_two_recurrent_updates(hip_lib):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "balance_mappo_train_device.py")
    spec = importlib.util.spec_from_file_location("balance_mappo_train_device", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    runs = []
    for _ in range(2):
        evaluation, final = {}, {}
        history = tool.train(33, 8, 2, 1, evaluation=evaluation, final=final, recurrent=True, data_chunk_length=4)
        runs.append((history, evaluation, final["params"].numpy()))
    history, evaluation, params = runs[0]
    assert len(history) == 2 and [entry["optimizer_step"] for entry in history] == [15, 30]
    for entry in history:
        assert 4 * 33 <= entry["episodes"] <= 8 * 33 and entry["mean_return"] is not None
        for name in _lib.MAPPO_STATS[:7]:
            assert np.isfinite(entry[name]), name
        assert 0.5 < entry["ratio"] < 1.5 and entry["dist_entropy"] > 0 and entry["critic_grad_norm"] > 0
    assert history[0]["value_loss"] != history[1]["value_loss"]  # the parameters moved between the updates
    assert params.shape == (twin.num_params(2),) and np.isfinite(params).all()
    assert sum(evaluation["returns"].values()) == 33
    same_bits(runs[1][2], params, "the parameters of a second run")
    with pytest.raises(ValueError, match="chunk_length"):
        tool.train(33, 8, 1, 1, recurrent=True, data_chunk_length=3)


def test_policy_agent_owns_its_state(hip_lib):
    from madrona_rl_envs_playground_amd.pantheonrl_extension import MlpBasePolicyAgent
    n, seed = 33, 21
    policy = make_policy(1, "trained")
    env, plain = BalanceMadronaTorch(n, 0), BalanceMadronaTorch(n, 0)
    agent = MlpBasePolicyAgent(env, policy, seed=seed)
    env.add_partner_agent(agent, player_num=1)
    env.reset()
    own = MlpBaseGruState(n, DEV)
    for k in range(3):
        ego = torch.full((n, 1), k % 4, dtype=torch.int32, device=DEV)
        policy.bind(own)
        mlpbase_act(plain.sim, policy, players=[1], seed=seed, step=k)
        want = cpu(plain.static_actions[1])
        env.step(ego)
        same_bits(cpu(env.static_actions[1]), want, f"the partner's actions at step {k}")
        plain.static_actions[0].copy_(ego)
        plain.sim.step()
    # the agent bound its own state for its call alone: what the caller had bound is bound again
    assert agent.state is not own and policy.running is own
    same_bits(cpu(agent.state.actor), cpu(own.actor), "the agent's own state")
    assert cpu(agent.state.actor)[:, 1].any() and not cpu(agent.state.actor)[:, 0].any() and not cpu(agent.state.critic).any()
    env.close()
    plain.close()
