"""No GPU: what tests/test_gpu_cnn_gru_shapes.py rests on (tests/cnn_gru_shape_cases.py) -- the input conditions of every new
recurrent case, checked with the twin alone as tests/test_cnn_gru_api.py does for the old ones, and the literal LDS images of the
recurrent act and update against the table's, with two cases on each side of each crossover."""
import ctypes

import numpy as np
import pytest

import cnn_gru_shape_cases as cases
import cnn_gru_twin as twin
import kitchen_shape_cases as table
from madrona_rl_envs_playground_amd import _lib


@pytest.mark.parametrize("key, seats", cases.ACT_CASES)
def test_act_cases_decide_their_draws(key, seats):
    n, p, pick = cases.N, twin.shape(key)[2], np.array(seats)
    assert max(seats) < p and twin.shape(key) == table.shape(key)
    inputs = twin.act_inputs(key, n, "nonzero")
    assert inputs["done"].any() and not inputs["done"].all() and inputs["h_actor"][:, pick].any() and inputs["h_critic"][:, pick].any()
    rows = inputs["obs"][:, pick].reshape((-1,) + inputs["obs"].shape[2:])
    u = twin.draws(17, 5, n, p).reshape(n, p)[:, pick].reshape(-1)
    exact = twin.act(twin.params_of(key), key, rows, inputs["h_actor"][:, pick].reshape(-1, 64), inputs["h_critic"][:, pick].reshape(-1, 64),
                     np.repeat(1.0 - (inputs["done"] != 0), len(seats)), u)
    assert (~twin.near_boundary(exact["cdf"], u)).mean() >= 0.9
    assert len(np.unique(exact["actions"])) > 2
    d = twin.act_margins(twin.params_of(key), key, rows, inputs["h_actor"][:, pick].reshape(-1, 64), inputs["h_critic"][:, pick].reshape(-1, 64),
                         np.repeat(1.0 - (inputs["done"] != 0), len(seats)))
    print((key, seats), "d:", {k: "%.2e" % v for k, v in d.items()})
    assert all(0 < v < 1e-4 for v in d.values())


@pytest.mark.parametrize("case", cases.UPDATE_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_update_cases_clip_some_samples_and_not_others(case):
    key, L, Bc = case
    params, batch, ids = twin.update_case(*case)
    exact, single = cases.twin_rows(case)
    assert 0.05 < exact["stats"]["clipfrac"] < 0.95
    count = round(exact["stats"]["clipfrac"] * Bc * L)
    assert 0 < count < Bc * L and round(single["stats"]["clipfrac"] * Bc * L) == count  # float32 clips the same samples
    assert batch.dones.any() and not batch.dones.all() and batch.h0_actor.any() and batch.h0_critic.any()
    assert batch.chunk_length == L and ids.shape == (1, Bc) and len(np.unique(ids[0])) == Bc
    t, n, p = batch.actions.shape
    assert p == twin.shape(key)[2] and t % L == 0 and ids.max() < t // L * n * p
    # the critic learns: the reference's Huber term is one-sided (e < -delta contributes nothing), and a critic far above its
    # normalised returns would get no gradient at all -- at least a quarter of the samples contribute, and both nets' gradients move
    where = twin.evaluate(twin.module_from(params, key), batch, ids[0])[2]
    _, mean, std = twin.value_norm_update((0.0, 0.0, 0.0), batch.returns[where].reshape(-1), twin.Config())
    error = (batch.returns[where] - mean) / std - exact["values"]
    assert (error >= -twin.Config().huber_delta).mean() >= 0.25, (case, float((error >= -1).mean()))
    na = twin.actor_size(key)
    assert exact["stats"]["value_loss"] > 0 and exact["stats"]["critic_grad_norm"] > 0 and exact["stats"]["actor_grad_norm"] > 0
    assert (exact["grad"][:na] != 0).mean() > 0.5 and (exact["grad"][na:] != 0).mean() > 0.5
    d_grad = float(np.sqrt(np.sum((single["grad"] - exact["grad"]) ** 2)))
    print(case, "clipfrac", exact["stats"]["clipfrac"], "d(grad) = %.2e" % d_grad)
    assert 0 < d_grad < 1e-3 * float(np.sqrt(np.sum(exact["grad"] ** 2)))


@pytest.mark.parametrize("key", sorted({case[0] for case in cases.UPDATE_CASES}))
def test_pooled_stat_margins_cover_every_row(key):
    pooled = cases.stat_margins(key)
    assert set(cases.pool(key)) >= {case for case in cases.UPDATE_CASES if case[0] == key} and len(cases.pool(key)) >= 3
    for case in cases.pool(key):
        exact, single = cases.twin_rows(case)
        assert all(abs(single["stats"][name] - exact["stats"][name]) <= pooled[name] for name in twin.STATS)
    print(key, "pooled d of the stats:", {name: "%.2e" % value for name, value in pooled.items()})
    assert all(0 < pooled[name] < 1e-4 for name in twin.STATS if name != "clipfrac")


def test_lds_literals_and_the_crossovers(hip_lib):
    assert (cases.GRU_ACT_BYTES, cases.GRU_UPDATE_BYTES) == ((64 * 65 + 2 * 32 * 65 + 32 * 8) * 4 + 75264, 135680)
    assert {key for key, _ in cases.ACT_CASES} | {case[0] for case in cases.UPDATE_CASES} == set(cases.LDS)
    for key, (act, update) in cases.LDS.items():
        _, _, _, plain_act, plain_update = table.ACCEPTED[key]
        assert act == max(plain_act, cases.GRU_ACT_BYTES), key
        assert update == max(plain_update - cases.TAIL, cases.GRU_UPDATE_BYTES) + cases.TAIL, key
        assert act <= table.LDS_LIMIT and update <= table.LDS_LIMIT
        w, h, _, f = twin.shape(key)
        out = ctypes.c_uint64(0)
        assert hip_lib.mrl_mappo_workspace_bytes(w, h, f, 64 | _lib.CNN_GRU_HIDDEN, cases.BC, 1, ctypes.byref(out)) == _lib.MRL_OK and out.value > 0
    # the table's entries nearest each crossover on either side are cases, and two cases lie on each side of each
    plain_acts = {key: table.ACCEPTED[key][3] for key in table.KEYS}
    tails = {key: table.ACCEPTED[key][4] - cases.TAIL for key in table.KEYS}
    act_keys, update_keys = [key for key, _ in cases.ACT_CASES], [case[0] for case in cases.UPDATE_CASES]
    assert max((v, k) for k, v in plain_acts.items() if v < cases.GRU_ACT_BYTES)[1] == "forced_coordination" in act_keys
    assert min((v, k) for k, v in plain_acts.items() if v > cases.GRU_ACT_BYTES)[1] == "k15x3p2" in act_keys
    assert max((v, k) for k, v in tails.items() if v < cases.GRU_UPDATE_BYTES)[1] == "k6x5p4" in update_keys
    assert min((v, k) for k, v in tails.items() if v > cases.GRU_UPDATE_BYTES)[1] == "counter_circuit" in update_keys
    assert sum(plain_acts[k] < cases.GRU_ACT_BYTES for k in act_keys) >= 2 and sum(plain_acts[k] > cases.GRU_ACT_BYTES for k in act_keys) >= 2
    assert sum(tails[k] < cases.GRU_UPDATE_BYTES for k in update_keys) >= 2 and sum(tails[k] > cases.GRU_UPDATE_BYTES for k in update_keys) >= 2
    assert all(tails[k] != cases.GRU_UPDATE_BYTES and plain_acts[k] != cases.GRU_ACT_BYTES for k in table.KEYS)
    # the classes: P = 3, npos 12, 13 and 25, last slabs 23 and 4
    of = {key: table.classes(*(twin.shape(key)[i] for i in (0, 1, 3))) for key in update_keys}
    assert {c["npos"] for c in of.values()} >= {12, 13, 25} and {c["last_slab"] for c in of.values()} >= {23, 4}
    assert 3 in {twin.shape(key)[2] for key in update_keys} and 3 in {twin.shape(key)[2] for key in act_keys}
    assert {(twin.shape(key)[0] - 2) * (twin.shape(key)[1] - 2) for key in act_keys} >= {12, 13, 25}
