"""MI355X: MAPPO's MLPBase actor-critic at hidden_size 512 on the balance beam (``mrl_mlpbase_act`` / ``mrl_rollout_mlpbase`` with
``MRL_MLPBASE_H512``) against the float64 torch module (tests/mlpbase_h512_cases.py), its modes, its rollout and its refusals.
The bound is the project's for its 512 kernels: 8 d, d the float32 module's own distance from the float64 one on the same case."""
import ctypes

import numpy as np
import pytest
import torch

import mlpbase_h512_cases as cases
from madrona_rl_envs_playground_amd import _lib
from madrona_rl_envs_playground_amd.envs.balance_beam_env import BalanceMadronaTorch
from madrona_rl_envs_playground_amd.simulators import MlpBasePolicy, MlpBasePolicyH512, MlpBaseRecord, mlpbase_act
from test_gpu_balance_mappo import DEV, cpu, record_arrays, same_bits  # the beam's MAPPO tests' helpers

pytestmark = pytest.mark.gpu


def marked(n, t=3):
    record = MlpBaseRecord(t, n, 2, DEV, logits=True)
    for name in _lib.MLPBASE_RECORD_BUFFERS:
        getattr(record, name).fill_(-3)
    return record


@pytest.mark.parametrize("layer_N, weights, n, seats", cases.FORWARD)
def test_act_matches_the_float64_module(hip_lib, layer_N, weights, n, seats):
    case = cases.forward_case(layer_N, weights, n, seats)
    exact, pick, row = case["exact"], np.array(seats), cases.ROW
    policy = MlpBasePolicyH512.from_module(cases.make_module(layer_N, weights), device=DEV)
    obs = cases.observations(n)
    runs = []
    for _ in range(2):
        env = BalanceMadronaTorch(n, 0)
        env.static_observations.copy_(torch.from_numpy(np.array(obs)).to(DEV))
        env.static_actions.fill_(-7)
        record = marked(n)
        env.act(policy, players=seats, record=record, row=row, seed=cases.SEED, step=cases.STEP)
        torch.cuda.synchronize()
        runs.append((record_arrays(record), cpu(env.static_actions)[..., 0]))
        env.close()
    got, actions = runs[0]
    for name, array in runs[1][0].items():
        same_bits(array, got[name], f"{name} of a second run")
    same_bits(runs[1][1], actions, "ACTION of a second run")
    values, logp = got["values"][row][:, pick].reshape(-1), got["logprobs"][row][:, pick].reshape(-1)
    logits, acted = got["logits"][row][:, pick].reshape(-1, 4), got["actions"][row][:, pick].reshape(-1)
    assert np.isfinite(values).all() and np.isfinite(logp).all() and np.isfinite(logits).all()
    assert case["near"].sum() <= 1 and np.array_equal(acted[~case["near"]], exact["actions"][~case["near"]])
    errors = {"values": np.abs(values - exact["values"]).max(), "logp": np.abs(logp - exact["logp"][np.arange(len(acted)), acted]).max(),
              "logits": np.abs(logits - exact["logits"]).max()}
    print((layer_N, weights, n, seats), "measured / d:", {k: round(float(e / d), 2) if d else float(e) for (k, e), d in zip(errors.items(), case["d"])})
    for (name, error), d in zip(errors.items(), case["d"]):
        assert error <= 8.0 * d, (name, error, d)
    # ACTION equals the record; the other seats, the record's other rows and other seats are untouched
    assert np.array_equal(actions[pick].T.reshape(-1), acted)
    assert (actions[[s for s in (0, 1) if s not in seats]] == -7).all()
    for name, array in got.items():
        touched = np.zeros(array.shape, bool)
        if name != "next_done":
            touched[row - 1 if name == "rewards" else row][:, pick] = True
        assert (array[~touched] == -3).all(), name
    same_bits(got["obs"][row][:, pick], np.ascontiguousarray(obs.transpose(1, 0, 2))[:, pick], "record.obs")


def test_modes_and_rollout(hip_lib):
    n, t, seed = 33, 4, 9  # tests/test_gpu_balance_mappo.py's rollout: episodes end inside it
    policy = MlpBasePolicyH512.from_module(cases.make_module(2, "trained"), device=DEV)
    plain = MlpBasePolicy(layer_N=2, device=DEV)
    plain.params.copy_(torch.from_numpy(cases.beam.params_of(2, "trained")).to(DEV))
    obs = torch.from_numpy(np.array(cases.observations(n))).to(DEV)

    def plain_act():
        env = BalanceMadronaTorch(n, 0)
        env.static_observations.copy_(obs)
        record = marked(n)
        env.act(plain, record=record, row=0, seed=seed, step=1)
        out = record_arrays(record)
        env.close()
        return out

    before = plain_act()
    fused, single = BalanceMadronaTorch(n, 0), BalanceMadronaTorch(n, 0)
    record = fused.rollout(policy, t, seed=seed, first_step=3)
    by_hand = MlpBaseRecord(t, n, 2, DEV)
    for k in range(t):
        single.n_step(single.act(policy, record=by_hand, row=k, seed=seed, step=3 + k))
    mlpbase_act(single.sim, policy, record=by_hand, row=t, value_only=True)
    torch.cuda.synchronize()
    a, b = record_arrays(record), record_arrays(by_hand)
    for name in a:
        same_bits(a[name], b[name], name)
    same_bits(cpu(fused.static_observations), cpu(single.static_observations), "the simulators' observations")
    assert a["dones"].sum() > 0 and a["values"][t].any()
    after = plain_act()
    for name in before:
        same_bits(after[name], before[name], f"the hidden-64 act's {name} behind a hidden-512 rollout")

    # greedy: the first arg-max of the recorded logits; without a record the same ACTION
    greedy = marked(n)
    single.static_actions.fill_(-7)
    single.act(policy, record=greedy, row=0, seed=seed, step=2, greedy=True)
    with_record = cpu(single.static_actions)
    logits = cpu(greedy.logits)[0]
    assert np.array_equal(cpu(greedy.actions)[0], logits.argmax(axis=-1)) and np.array_equal(with_record[..., 0].T, cpu(greedy.actions)[0])
    single.act(policy, record=greedy, row=1, seed=seed, step=2)
    with_record = cpu(single.static_actions)
    single.static_actions.fill_(-7)
    single.act(policy, seed=seed, step=2)
    same_bits(cpu(single.static_actions), with_record, "ACTION of an act without a record")
    for env in (fused, single):
        env.close()


def test_c_level_refusals_change_nothing(hip_lib):
    L, n, INVALID = hip_lib, 33, _lib.MRL_ERR_INVALID
    policy = MlpBasePolicyH512.from_module(cases.make_module(1, "init"), device=DEV)
    env = BalanceMadronaTorch(n, 0)
    env.static_actions.fill_(-7)
    record, before = marked(n), cpu(policy.params)
    stream, handle, rec = torch.cuda.current_stream().cuda_stream, env.sim._handle, ctypes.byref(record.struct)

    def desc(hidden=512, flags=_lib.MLPBASE_H512):
        return ctypes.byref(_lib.MlpBasePolicyDesc(policy.params.data_ptr(), hidden, 1, flags))

    # the bit with another width, with the recurrent bit; the width without the bit
    for d in (desc(hidden=64), desc(hidden=512 | _lib.MLPBASE_H512_HIDDEN), desc(flags=_lib.MLPBASE_H512 | _lib.MLPBASE_RECURRENT), desc(flags=0)):
        assert L.mrl_mlpbase_act(handle, 3, d, rec, 0, 0, 0, 0, stream) == INVALID
        assert L.mrl_rollout_mlpbase(handle, 3, d, rec, 0, 0, stream) == INVALID
    assert L.mrl_mlpbase_act(handle, 3, desc(), rec, 0, 0, 0, _lib.MLPBASE_H512, stream) == INVALID  # never a bit of the act's flags
    for hidden in (512, 64):
        bank = ctypes.byref(_lib.MlpBaseBankDesc(policy.params.data_ptr(), 1, policy.num_params, hidden, 1, _lib.MLPBASE_H512))
        assert L.mrl_mlpbase_act_bank(handle, 3, bank, None, rec, None, 0, 0, 0, 0, None, 0, stream) == INVALID
        assert L.mrl_rollout_mlpbase_bank(handle, 3, bank, None, None, None, rec, None, 0, 0, None, 0, stream) == INVALID
        assert L.mrl_mappo_mlp_update(desc(hidden=hidden), None, None, None, 1, 65, None, None, None, 0, None, None, 0, stream) == INVALID
        assert L.mrl_mappo_mlp_bank_update(desc(hidden=hidden), None, None, None, 1, 65, None, None, None, 0, None, None, 0, stream) == INVALID
    torch.cuda.synchronize()
    same_bits(cpu(policy.params), before, "the parameters")
    assert (cpu(env.static_actions) == -7).all()
    assert all((array == -3).all() for array in record_arrays(record).values())
    env.close()
