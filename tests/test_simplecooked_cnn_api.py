"""No GPU: what the Simplecooked CNN tests on the GPU rest on (tests/simplecooked_cnn_cases.py) -- the shapes, the float64 twin
against torch float32 on every forward case's inputs and how many draws lie near a boundary, the integer construction's bound,
the input conditions of every update case -- and the Python surface: ``act`` / ``rollout`` on the Simplecooked env, ``game`` in the
training tool, and what ``--recipe colab`` resolves to."""
import importlib.util
import inspect
import os

import numpy as np
import pytest

import cnn_twin
import mappo_twin
import simplecooked_cnn_cases as cases
from madrona_rl_envs_playground_amd import layouts
from madrona_rl_envs_playground_amd.envs import overcooked2_env, overcooked_env

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def simplecooked_shapes():
    with cases.shapes():
        yield


def load_tool():
    spec = importlib.util.spec_from_file_location("overcooked_train_device", os.path.join(REPO, "tools", "overcooked_train_device.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def test_shapes_are_the_layouts_own():
    assert cases.shape("simple") == (5, 4, 2, 20) and cases.shape("unident_s") == (9, 5, 2, 20) and cases.shape("random1") == (5, 5, 2, 20)
    assert cases.shape("random1/1p") == (5, 5, 1, 15) and cases.shape("simple/1p") == (5, 4, 1, 15)
    for key in cases.KEYS:
        w, h, p, f = cases.shape(key)
        params = cases.layout_params(key)
        assert (w, h, p) == (params["width"], params["height"], params["num_players"]) and f == 5 * p + 10
    # the paths the Overcooked cases never ran: an odd K in the convolution, and rows at all four byte offsets of a dword
    w, h, p, f = cases.shape("random1/1p")
    assert (9 * f) % 2 == 1 and w * h * f == 375 and {(s * 375) % 4 for s in range(4)} == {0, 1, 2, 3}
    assert all((9 * cnn_twin.shape(layout)[3]) % 2 == 0 for layout, _ in cnn_twin.CASES)
    # other layouts keep cnn_twin's answer inside the substitution, and outside it nothing is left behind
    assert cnn_twin.shape("cramped_room") == (5, 4, 2, 26)


def test_the_substitution_ends_with_its_block():
    inner = cnn_twin.shape
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(cnn_twin, "shape", cases._overcooked_shape)
        with pytest.raises(KeyError):
            cnn_twin.shape("simple")
        with cases.shapes():
            assert cnn_twin.shape("simple") == (5, 4, 2, 20)
        with pytest.raises(KeyError):
            cnn_twin.shape("simple")
    assert cnn_twin.shape is inner


@pytest.mark.parametrize("key,n,weights,inputs", cases.ALL_CASES)
def test_twin_against_torch_float32_and_the_boundary_condition(key, n, weights, inputs, oracle_lib):
    module = cases.make_module(key, weights)
    obs = cases.case_inputs(key, n, weights, inputs)["obs"]
    w, h, p, f = cases.shape(key)
    assert obs.shape == (n, p, h, w, f) and obs.dtype == np.int8
    rows = cnn_twin.rows_of(obs)
    d_value, d_logp = cases.case_margins(key, n, weights, inputs)
    # float32 against float64 over K <= 672 products of O(1): a few 1e-6 at most; a twin with a wrong index map is off by O(1)
    assert d_value <= 2e-5 and d_logp <= 5e-5, (d_value, d_logp)
    cap_value, cap_logp = cases.layout_margins(key, weights)
    print(f"{key} n={n} {weights} {inputs}: d(values) = {d_value:.3e} of {cap_value:.3e}, d(log-probs) = {d_logp:.3e} of {cap_logp:.3e}")
    assert 0 < d_value <= cap_value and 0 < d_logp <= cap_logp
    # a condition of the GPU test, not a measurement: at most 1 % of the rows have their draw within 1e-5 of a boundary
    u = cnn_twin.draws(cases.case_seed(key, n, weights, inputs), 0, n, p)
    want = cnn_twin.act(cnn_twin.flat(module), rows, u)
    assert cnn_twin.near_boundary(want["cdf"], u).sum() <= 0.01 * len(rows)
    assert ((want["actions"] >= 0) & (want["actions"] <= 5)).all()


def test_stepped_cases_are_not_the_start_state(oracle_lib):
    for key, n, weights, inputs in cases.ALL_CASES:
        if inputs == "stepped" and n > 1:
            obs = cases.case_inputs(key, n, weights, inputs)["obs"]
            assert not all(np.array_equal(obs[0], obs[k]) for k in range(1, n)), key  # the worlds went different ways


@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_integer_construction_stays_exact_in_float32(key):
    layers, obs = cases.integer_case(key)
    w, h, p, f = cases.shape(key)
    assert obs.shape == (cases.INTEGER_N, p, h, w, f) and layers["actor"][0][0].shape == (32, f, 3, 3)
    values, logits, bound = cnn_twin.integer_forward(layers, cnn_twin.rows_of(obs))
    assert bound < 2 ** 24
    params = cnn_twin.integer_params(layers)
    assert np.abs(params).max() < 2 ** 24 and (params == np.round(params)).all()
    v64, l64 = cnn_twin.forward(params, cnn_twin.rows_of(obs))
    assert np.array_equal(v64, values) and np.array_equal(l64, logits)
    lo, hi = cnn_twin.TIE
    assert (logits[:, lo] == logits[:, hi]).all() and (logits.argmax(axis=1) == lo).all()
    assert len(np.unique(values)) > len(values) // 2 and (values != 0).any()
    conv = layers["actor"][0][0]
    assert not np.array_equal(conv, conv.transpose(0, 1, 3, 2))  # not symmetric in (i, j)
    # the last (f, i, j) of every channel -- the product next to the pad of an odd K -- carries weight and meets nonzero inputs
    assert np.abs(conv[:, -1, 2, 2]).sum() > 0 and np.abs(cnn_twin.rows_of(obs)[..., -1]).sum() > 0


@pytest.mark.parametrize("case", cases.MAPPO_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_input_conditions_of_every_update_case(case, oracle_lib):
    """conditions, not measurements (tests/test_mappo_update_api.py): in the twin no sample lies within KINK of a kink of the loss,
    no pre-activation is closer to 0 than 8 x the largest float32-vs-twin pre-activation distance unless it is exactly 0 in both,
    and the batches put their samples on every branch"""
    fixed = cases.fixed_case(case)
    exact, width = fixed["twin"], case[4]
    closest, worst = mappo_twin.relu_margin(fixed)
    print(case, "kink", exact["kink"], "closest pre-activation", closest, "worst float32 distance", worst)
    assert exact["kink"] > mappo_twin.KINK, (case, exact["kink"])
    assert closest > mappo_twin.FACTOR * worst, (case, closest, worst)
    assert mappo_twin.conditions_hold(fixed)
    w, h, p, f = cases.shape(case[0])
    assert len(fixed["batch"].ring) == cases.T * case[1] * p and fixed["batch"].ring.shape[1:] == (h, w, f)
    assert (fixed["indices"] >= 0).all() and (fixed["indices"] < len(fixed["batch"].ring)).all()
    assert len(np.unique(fixed["indices"][0])) == width
    if width < 24:
        return
    b = exact["branches"]
    assert b["ratio_clipped"] >= 0.25 and b["value_clipped"] >= 0.25 and min(b["clipped_high"], b["clipped_low"]) >= 0.1, (case, b)
    assert min(b["huber_above"], b["huber_below"]) >= 0.05, (case, b)


def test_both_kitchen_envs_share_act_and_rollout():
    for name in ("act", "rollout"):
        ours, theirs = getattr(overcooked2_env.OvercookedMadrona, name), getattr(overcooked_env.OvercookedMadrona, name)
        assert ours is theirs  # one body, not a copy
        assert inspect.signature(ours) == inspect.signature(theirs)
    assert list(inspect.signature(overcooked2_env.OvercookedMadrona.act).parameters) == \
        ["self", "policy", "players", "record", "row", "seed", "step", "greedy"]
    assert list(inspect.signature(overcooked2_env.OvercookedMadrona.rollout).parameters) == \
        ["self", "policy", "num_steps", "seed", "first_step", "players", "record", "ring", "greedy"]


def test_train_takes_game_and_the_colab_recipe_resolves():
    tool = load_tool()
    signature = inspect.signature(tool.train)
    assert signature.parameters["game"].default == "overcooked"
    for name in ("lr", "critic_lr", "entropy_coef", "horizon", "ppo_epoch", "num_mini_batch"):
        assert name in signature.parameters
    with pytest.raises(ValueError, match="game"):
        tool.make_env("hanabi", "simple", 3, 8)
    resolve = lambda argv: tool.resolve(tool.parser().parse_args(argv))  # noqa: E731
    # without --game and --recipe: what the tool did before it had either
    assert resolve([]) == {"game": "overcooked", "layout": "cramped_room", "num_envs": 1024, "num_steps": 128, "horizon": 400,
                           "updates": 20, "ppo_epoch": 15, "num_mini_batch": 1, "lr": 5e-4, "critic_lr": 5e-4, "entropy_coef": 0.01}
    assert signature.parameters["horizon"].default == 400 and signature.parameters["lr"].default == 5e-4
    assert signature.parameters["entropy_coef"].default == 0.01 and signature.parameters["ppo_epoch"].default == 15
    # the notebook: simple, 800 worlds, episode_length 200 = horizon, 7 epochs, one minibatch, both rates 1e-2, no entropy bonus,
    # 8 M env steps = 50 updates
    colab = resolve(["--recipe", "colab"])
    assert colab == {"game": "simplecooked", "layout": "simple", "num_envs": 800, "num_steps": 200, "horizon": 200, "updates": 50,
                     "ppo_epoch": 7, "num_mini_batch": 1, "lr": 1e-2, "critic_lr": 1e-2, "entropy_coef": 0.0}
    assert colab["updates"] * colab["num_steps"] * colab["num_envs"] == 8_000_000
    assert "simple" in layouts.SIMPLECOOKED_LAYOUTS
    # an option given wins over the recipe
    mixed = resolve(["--recipe", "colab", "--updates", "3", "--lr", "0.001", "--critic-lr", "0.002", "--entropy-coef", "0.05", "--horizon", "50"])
    assert (mixed["updates"], mixed["lr"], mixed["critic_lr"], mixed["entropy_coef"], mixed["horizon"]) == (3, 1e-3, 2e-3, 0.05, 50)
    assert mixed["num_envs"] == 800 and mixed["game"] == "simplecooked"
    assert resolve(["--game", "simplecooked", "--layout", "random1"])["horizon"] == 400
    assert tool.parser().parse_args(["--evaluate"]).evaluate is True
