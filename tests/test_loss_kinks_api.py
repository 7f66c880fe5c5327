"""No GPU: the conditions of every case of tests/kink_cases.py, which tests/test_gpu_loss_kinks.py runs on the device.  They are
properties of the twins and of int64 numpy, never of the device's answer.

For the exact cases: float32 torch equals the float64 twin bit for bit; the twin equals int64 numpy; every gradient element
times 2 B is an integer; the sum of absolute terms times 2 B is below 2^24, so float32 holds every partial sum in whatever order
the device takes it; every category occurs four times at least in a mixed row; the literal tables are what the twins compute
per category; and the twins' own kink distance is exactly 0 -- the OPPOSITE of the condition of every other case of the four
learners (``test_input_conditions_of_every_gpu_case`` and its like), on purpose: do not "repair" it.

For the tolerance cases: the twin's identities the device is asked to reproduce (the gradient at clip 0 equals the one at clip
0.2 when the old log-probs are the computation's own; an advantage of 0 leaves the entropy term alone; a constant advantage
normalises to 0), and the input conditions that make a float32 gradient comparable with the twin at all."""
import ctypes

import numpy as np
import pytest
import torch

import kink_cases as cases
import mappo_twin
import mlpbase_twin
import ppo_twin
import wide_twin
import wide_update_twin
from madrona_rl_envs_playground_amd import _lib

LIMIT = 2 ** 24


def ppo_tile(lib):
    def size(width):
        out = ctypes.c_uint64(0)
        assert lib.mrl_ppo_workspace_bytes(4, 64, 2, width, 1, ctypes.byref(out)) == _lib.MRL_OK
        return out.value
    return ppo_twin.tile_size(size)


def same_bits32(a, b):
    """a and b rounded to float32 have the same bits"""
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def check_exact(what, twin_grad, f32_grad, integers, unit, bound):
    """the conditions of one exact gradient (a slice of the twin's): int64 numpy's, float32's, integers over ``unit``, the bound"""
    assert np.array_equal(twin_grad * unit, np.asarray(integers, np.float64).reshape(-1)), what
    assert np.array_equal(f32_grad, twin_grad) and same_bits32(f32_grad, twin_grad), what
    assert np.array_equal(np.rint(twin_grad * unit), twin_grad * unit), what
    assert bound < LIMIT, (what, bound)


def check_table(what, table, row):
    """the literal table is what the twin's loss computes for this row's samples, and (a category alone) what the row reports"""
    _, _, slope, loss = cases.table_columns(table, row["categories"])
    assert np.array_equal(slope, row["slope"]) and np.array_equal(loss, row["loss"]), what


def test_tables_cover_the_squared_error_analogues():
    moved, err, slope, _ = cases.table_columns(cases.SQUARED_TABLE, np.arange(len(cases.SQUARED_TABLE)))
    near = np.clip(moved, -cases.CLIP, cases.CLIP)  # v_c - v_old; err_c = err - moved + near
    err_c = err - moved + near
    kinds = {"interior tie": (moved == 0) & (err != 0), "upper end": moved == cases.CLIP, "lower end": moved == -cases.CLIP,
             "tie beyond": (np.abs(moved) > cases.CLIP) & (np.abs(err) == np.abs(err_c)),
             "plain larger": (np.abs(moved) > cases.CLIP) & (np.abs(err) > np.abs(err_c)),
             "clipped larger": (np.abs(moved) > cases.CLIP) & (np.abs(err) < np.abs(err_c)), "zero error": (moved == 0) & (err == 0)}
    for name, hit in kinds.items():
        assert hit.any(), name
    assert (slope[kinds["tie beyond"]] == 0.5 * err[kinds["tie beyond"]]).all() and (slope[kinds["clipped larger"]] == 0).all()


@pytest.mark.parametrize("flags", sorted(cases.MAPPO_FLAGS))
def test_cnn_mixed_rows_are_exact(flags):
    row = cases.cnn_row("mixed", flags)
    na = mappo_twin.actor_size(row["layout"])
    check_exact(flags, row["twin"]["grad"][na:], row["f32"]["grad"][na:], row["critic"], row["unit"], row["bound"])
    assert row["indices"].shape == (1, 64) and len(np.unique(row["indices"])) == 64
    assert np.bincount(row["categories"], minlength=len(cases.MAPPO_TABLE)).min() >= 4
    assert row["twin"]["stats"]["value_loss"] == row["f32"]["stats"]["value_loss"] == row["loss"].mean()
    if flags == "default":
        check_table(flags, cases.MAPPO_TABLE, row)
        assert row["loss"].mean() == np.mean([entry[2] for entry in cases.MAPPO_TABLE]) == 5.3125
        assert np.abs(row["critic"]).max() == 24192  # (the largest |element| x 2 B; 16 812 on the index row the issue drew)
    # exactly on the kinks -- except with both flags off, where the loss is smooth
    assert row["twin"]["kink"] == (1.0 if flags == "neither" else 0.0)
    # the planting leaves the actor's columns alone
    plain = mappo_twin.integer_case(row["layout"])
    for name in ("actions", "logprobs", "advantages"):
        assert np.array_equal(getattr(row["batch"], name), getattr(plain["batch"], name))
    assert np.array_equal(row["batch"].ring, plain["batch"].ring) and np.array_equal(row["indices"], plain["indices"])


@pytest.mark.parametrize("category", range(len(cases.MAPPO_TABLE)))
def test_cnn_category_rows_are_exact(category):
    row = cases.cnn_row(category)
    na = mappo_twin.actor_size(row["layout"])
    check_exact(category, row["twin"]["grad"][na:], row["f32"]["grad"][na:], row["critic"], row["unit"], row["bound"])
    check_table(category, cases.MAPPO_TABLE, row)
    assert row["indices"].shape == (1, 32) and (row["categories"] == category).all()
    _, slope, loss = cases.MAPPO_TABLE[category]
    # a row that holds one category alone gives the table's db_head and value_loss
    assert row["twin"]["grad"][-1] == slope and row["twin"]["stats"]["value_loss"] == row["f32"]["stats"]["value_loss"] == loss
    assert (row["twin"]["kink"] == 0.0) == (category in cases.MAPPO_ON_KINK)


@pytest.mark.parametrize("which", ["mixed"] + list(range(len(cases.MAPPO_TABLE))))
def test_mlp_rows_have_an_exact_head(which):
    row = cases.mlp_row(which)
    module = mlpbase_twin.module_from(row["params"], 1)
    assert not module.critic.v_out.weight.any() and module.critic.v_out.bias.item() == cases.MLP_VALUE
    na, head = mlpbase_twin.actor_size(1), mlpbase_twin.HIDDEN + 1
    for name in ("twin", "f32"):
        grad = row[name]["grad"]
        assert grad[-1] * row["unit"] == row["db_head"] and not grad[na:-head].any(), (which, name)
        assert row[name]["stats"]["value_loss"] == row["loss"].mean()
    check_table(which, cases.MAPPO_TABLE, row)
    assert np.abs(row["twin"]["grad"][-head:-1]).max() > 0 or not row["slope"].any()
    if which == "mixed":
        assert np.bincount(row["categories"], minlength=len(cases.MAPPO_TABLE)).min() >= 4 and row["twin"]["kink"] == 0.0
    else:
        assert row["twin"]["grad"][-1] == cases.MAPPO_TABLE[which][1]
        assert (row["twin"]["kink"] == 0.0) == (which in cases.MAPPO_ON_KINK)


@pytest.mark.parametrize("which", ["mixed"] + list(range(len(cases.SQUARED_TABLE))))
def test_ppo_rows_are_exact(hip_lib, which):
    tile = ppo_tile(hip_lib)
    row = cases.ppo_row(tile, which)
    width = row["indices"].shape[1]
    assert tile < width <= 2 * tile and width & (width - 1) == 0 and row["unit"] == 2 * width
    for key, at in zip(("dW2", "db2"), row["slices"]):
        check_exact((which, key), row["twin"]["grad"][at], row["f32"]["grad"][at], row[key], row["unit"], row["bound"])
    check_table(which, cases.SQUARED_TABLE, row)
    assert row["twin"]["stats"]["v_loss"] == row["f32"]["stats"]["v_loss"] == row["loss"].mean()
    if which == "mixed":
        assert np.bincount(row["categories"], minlength=len(cases.SQUARED_TABLE)).min() >= 4 and row["twin"]["kink"] == 0.0
        assert np.abs(row["dW2"]).max() > 0 and np.abs(row["db2"]).max() > 0
    else:
        _, slope, loss = cases.SQUARED_TABLE[which]
        # the table is the twin's: d2[j] = W3[j] d3 with W3[j] = j - 20, so db2[21] is the category's dL/dv
        assert row["twin"]["grad"][row["slices"][1]][21] == slope and row["twin"]["stats"]["v_loss"] == loss
        assert (row["twin"]["kink"] == 0.0) == (which in cases.SQUARED_ON_KINK)


@pytest.mark.parametrize("which", ["mixed"] + list(range(len(cases.SQUARED_TABLE))))
def test_wide_rows_are_exact(which):
    row = cases.wide_row(which)
    size = cases.wide_critic_size(row["rec"]["states"].shape[2])
    assert len(row["critic"]) == size and row["unit"] == 2 * cases.WIDE_SIZE
    check_exact(which, row["twin"]["grad"][:size], row["f32"]["grad"][:size], row["critic"], row["unit"], row["bound"])
    check_table(which, cases.SQUARED_TABLE, row)
    assert row["twin"]["stats"]["v_loss"] == row["f32"]["stats"]["v_loss"] == row["loss"].mean()
    if which == "mixed":
        assert np.bincount(row["categories"], minlength=len(cases.SQUARED_TABLE)).min() >= 4
        assert np.count_nonzero(row["critic"]) > size // 8
    else:
        _, slope, loss = cases.SQUARED_TABLE[which]
        assert row["twin"]["grad"][size - 1] == slope and row["twin"]["stats"]["v_loss"] == loss  # (the head's bias)
    # the wide twin has no kink census of its own: the samples are on the kinks by the table, which ``ppo_twin``'s census saw


def test_value_norm_floor_case_is_exact():
    row = cases.floor_case()
    na = mappo_twin.actor_size(row["layout"])
    check_exact("floor", row["twin"]["grad"][na:], row["f32"]["grad"][na:], row["critic"], row["unit"], row["bound"])
    assert row["twin"]["stats"]["value_loss"] == row["f32"]["stats"]["value_loss"] == row["value_loss"] > 0
    assert not row["batch"].returns.any() and np.abs(row["critic"]).max() > 0
    # the row's norm: mean 0, the variance on its floor; the state after one row: only the debiasing term has moved, to the
    # float32 1 - beta that torch, and so the C ABI's configuration, rounds on its own -- at or above epsilon
    cfg = row["cfg"]
    assert row["twin"]["norm"] == (0.0, 0.1)
    for name in ("twin", "f32"):
        assert row[name]["state"].tolist() == [0.0, 0.0, cfg.vn_one_minus_beta]
    assert row["states"][0].tolist() == [0.0, 0.0, cfg.vn_one_minus_beta] and cfg.vn_one_minus_beta >= cfg.vn_epsilon
    assert cfg.vn_one_minus_beta == float(np.float32(1.0 - 0.99999))
    assert all(state.dtype == np.float32 and not state[:2].any() for state in row["states"])
    assert row["states"][0][2] < row["states"][1][2] < row["states"][2][2] and (row["indices"] == row["indices"][0]).all()


def test_under_floor_case_conditions():
    row = cases.under_floor_case()
    assert mappo_twin.conditions_hold(row), (row["twin"]["kink"], mappo_twin.relu_margin(row))
    gathered = row["batch"].returns[row["indices"][0].astype(np.int64)]
    for dtype in (np.float64, np.float32):
        variance = cases.unfloored_variance(cases.UNDER_FLOOR_STATE, gathered, row["cfg"], dtype)
        assert 0 < variance < 5e-3, (dtype, variance)  # half the floor at the most: the floor itself is no kink of the case
    # normalised by 0.1, not by 0.05
    assert row["twin"]["norm"][1] == 0.1 and abs(row["twin"]["norm"][0] - 0.5) < 1e-3
    b = row["twin"]["branches"]
    assert b["value_clipped"] >= 0.25 and 0.1 <= b["huber_above"] <= 0.9, b
    # a floor of another size is far away: without one (std 0.05) every target doubles
    state = np.asarray(cases.UNDER_FLOOR_STATE, np.float64)
    wrong = mappo_twin.row(row["params"], row["layout"], row["batch"]._replace(returns=(0.5 + 2 * (row["batch"].returns - 0.5)).astype(np.float32)),
                           row["indices"][0], row["cfg"], state)
    d = mappo_twin.row_margins(row["twin"], row["f32"])
    assert mappo_twin.distance(wrong["grad"], row["twin"]["grad"]) > 100 * d["grad"]
    assert abs(wrong["stats"]["value_loss"] - row["twin"]["stats"]["value_loss"]) > 1e-2


@pytest.mark.parametrize("name", sorted(cases.LEARNERS))
def test_actor_identities_hold_in_both_precisions(name):
    """B1 and B2 on a host-made record: with the old log-probs the computation's own, closing the clip interval to the point 1
    changes nothing (torch passes the full gradient on a tie that sits on both ends of the clamp), and an advantage of 0 leaves
    the entropy term alone wherever the ratio is"""
    learner = cases.LEARNERS[name]
    params, batch, indices = cases.synthetic_actor_batch(name)
    count = len(indices)
    assert count == cases.ACTOR_T * cases.ACTOR_N * (2 if name in ("cramped_room", "beam") else 1)
    advantages = batch["advantages"] if isinstance(batch, dict) else batch.advantages
    assert (advantages > 0).sum() > count // 4 and (advantages < 0).sum() > count // 4
    closed, open_ = cases.actor_rows(learner, params, batch, indices, 0.0), cases.actor_rows(learner, params, batch, indices, 0.2)
    zero = np.zeros(count, np.float32)
    still = cases.actor_rows(learner, params, batch, indices, 0.2, advantages=zero)
    pushed = cases.actor_rows(learner, params, batch, indices, 0.2, shift=cases.signs(count), advantages=zero)
    for precision in ("twin", "f32"):
        assert np.array_equal(closed[precision]["grad"], open_[precision]["grad"]), (name, precision)
        stats = closed[precision]["stats"]
        if "ratio" in stats:
            assert stats["ratio"] == 1.0 and stats["clipfrac"] == 0.0
        else:
            assert stats["approx_kl"] == 0.0 and stats["old_approx_kl"] == 0.0 and stats["clipfrac"] == 0.0
        assert np.array_equal(learner.actor(still[precision]["grad"]), learner.actor(pushed[precision]["grad"])), (name, precision)
        assert np.isfinite(pushed[precision]["grad"]).all() and pushed[precision]["stats"]["clipfrac"] == 1.0
    # a halved or a dropped surrogate gradient is tens of d away
    d = mappo_twin.distance(learner.actor(closed["twin"]["grad"]), learner.actor(closed["f32"]["grad"]))
    dropped = mappo_twin.distance(learner.actor(closed["twin"]["grad"]), learner.actor(still["twin"]["grad"]))
    assert d > 0 and dropped / 2 > 100 * d, (name, dropped, d)
    assert np.abs(learner.actor(still["twin"]["grad"])).max() > 100 * d  # the entropy term alone is a gradient, not nothing


@pytest.mark.parametrize("name", ["cartpole", "hanabi_very_small"])
def test_constant_advantages_normalise_to_zero(name):
    case = cases.constant_advantage_case(name)
    advantages = case["batch"]["advantages"] if name != "cartpole" else case["batch"].advantages
    assert len(advantages) == 64 and (advantages == np.float32(0.75)).all()
    # 64 x 0.75 = 48 and 64 x 0.5625 = 36 are exact in float32: mean 0.75, every deviation 0, whatever the order of the sums
    for dtype in (np.float32, np.float64):
        a = advantages.astype(dtype)
        assert a.sum(dtype=dtype) == 48 and (a * a).sum(dtype=dtype) == 36 and a.std(ddof=1) == 0
    for with_norm, plain in (("twin", "plain"), ("f32", "plain32")):
        assert np.array_equal(case[with_norm]["grad"], case[plain]["grad"]), (name, with_norm)
        assert case[with_norm]["stats"]["pg_loss"] == 0.0
    if name == "cartpole":
        # the value loss's kinks are the batch's own (the ratio's are out of play: the advantage is 0)
        assert case["twin"]["kink"] > ppo_twin.KINK


def test_illegal_top_case_conditions():
    case = cases.illegal_top_case()
    batch, cfg, column = case["batch"], case["cfg"], case["column"]
    size, a = batch["mask"].shape
    assert size == 65 and not batch["mask"][:, column].any() and batch["mask"].any(axis=1).all()
    assert batch["mask"][np.arange(size), batch["actions"]].all()
    weights, bias = cases.wide_actor_head(case["params"], a)
    assert case["params"][bias][column] == cases.ILLEGAL_BIAS
    d, s, _ = wide_twin.dims(cases.MASK_GAME)
    logits = wide_twin.act(case["params"], batch["obs"], batch["state"], np.ones_like(batch["mask"]), np.zeros(size))["logits"]
    assert (logits.argmax(axis=1) == column).all() and np.abs(np.delete(logits, column, axis=1)).max() < 100  # above every legal logit
    checks = wide_update_twin.sample_checks(case["params"], batch, cfg)
    assert checks["loss_gap"].min() >= wide_update_twin.KINK
    assert checks["relu_gap"].min() >= wide_update_twin.FACTOR * checks["pre_d"].max()
    clipped = np.abs(checks["ratio"] - 1) > cfg.clip_coef
    assert clipped.mean() >= 0.25 and (np.abs(checks["moved"]) > cfg.clip_coef).mean() >= 0.25
    adv = batch["advantages"].astype(np.float64)
    normed = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    off = np.abs(checks["ratio"] - np.clip(checks["ratio"], 1 - cfg.clip_coef, 1 + cfg.clip_coef))
    assert not ((off > 0) & (np.abs(normed) * off < 10 * wide_update_twin.KINK)).any()
    for name in ("twin", "f32"):
        grad = case[name]["grad"]
        assert grad[bias][column] == 0 and not grad[weights].reshape(a, -1)[column].any() and np.isfinite(grad).all()
        assert np.abs(np.delete(grad[bias], column)).min() > 0


def test_single_legal_case_conditions():
    case = cases.single_legal_case()
    batch = case["batch"]
    size = len(batch["actions"])
    assert size == 33 and (batch["mask"].sum(axis=1) == 1).all() and batch["mask"][np.arange(size), batch["actions"]].all()
    critic = cases.wide_critic_size(batch["state"].shape[1])
    for name in ("twin", "f32"):
        assert not case[name]["grad"][critic:].any() and case[name]["grad"][:critic].any() and np.isfinite(case[name]["grad"]).all()
        assert case[name]["stats"]["entropy"] == 0.0
    # new log-prob 0: -logratio is the old log-prob itself
    assert abs(case["twin"]["stats"]["old_approx_kl"] - batch["logprobs"].astype(np.float64).mean()) < 1e-12
    assert (batch["advantages"] > 0).any() and (batch["advantages"] < 0).any()
    checks = wide_update_twin.sample_checks(case["params"], batch, case["cfg"])
    value_gap = np.minimum(np.abs(np.abs(checks["moved"]) - case["cfg"].clip_coef), checks["loss_gap"])
    assert checks["loss_gap"].min() >= wide_update_twin.KINK and value_gap.min() >= wide_update_twin.KINK


def test_rows_with_nothing_to_learn(hip_lib):
    na = mappo_twin.actor_size(cases.CNN_LAYOUT)
    row = cases.nothing_cnn()
    assert not row["twin"]["grad"][na:].any() and row["twin"]["stats"]["value_loss"] == 0 and row["cfg"].clip_grads
    row = cases.nothing_mlp()
    assert not row["twin"]["grad"][mlpbase_twin.actor_size(1):].any() and row["twin"]["stats"]["value_loss"] == 0
    row = cases.nothing_ppo(ppo_tile(hip_lib))
    assert not row["twin"]["grad"][:row["critic_size"]].any() and row["twin"]["grad"][row["critic_size"]:].any()
    assert row["twin"]["stats"]["v_loss"] == 0 and row["cfg"].max_grad_norm > 0
    row = cases.nothing_wide()
    size = cases.wide_critic_size(row["rec"]["states"].shape[2])
    assert not row["twin"]["grad"][:size].any() and row["twin"]["stats"]["v_loss"] == 0 and row["cfg"].max_grad_norm > 0
