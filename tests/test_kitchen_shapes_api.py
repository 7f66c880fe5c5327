"""No GPU: what tests/test_gpu_kitchen_shapes.py rests on (tests/kitchen_shape_cases.py) -- the table of kitchens and team sizes
and the classes of shape it covers, its LDS byte counts against the headers' arithmetic and the library's verdict, the terrain of
every key, the float64 twin against torch float32 on every act case and how many draws lie near a boundary, the integer
constructions' bounds (forward and the critic's back-propagation), the input conditions of every update row, and the refusal of
the shapes past the LDS limit through the C API."""
import ctypes

import numpy as np
import pytest

import cnn_twin
import mappo_twin
import kitchen_shape_cases as cases
from madrona_rl_envs_playground_amd import _lib, layouts

TERRAIN = {name: layouts.TERRAIN_GLYPHS.index(glyph) for name, glyph in (("AIR", " "), ("POT", "P"), ("COUNTER", "X"), ("ONION", "O"),
                                                                        ("DISH", "D"), ("SERVING", "S"))}


@pytest.fixture(autouse=True)
def table_shapes():
    with cases.shapes():
        yield


def test_shape_table_keeps_its_spread():
    """the classes of shape the GPU file runs first: a later edit of the table may move a row, not lose a class"""
    new = [cases.shape(key) for key in cases.KEYS]
    old = list(cases.OLD_SHAPES)
    of = lambda shapes, name: {cases.classes(w, h, f)[name] for w, h, _, f in shapes}  # noqa: E731
    # the old cases: W >= H, P <= 2, npos 6, 9 or 21, slab counts 8, 6 and 5
    assert all(w >= h and p <= 2 for w, h, p, _ in old) and of(old, "npos") == {6, 9, 21} and of(old, "slabs") == {8, 6, 5}
    npos = of(new, "npos")
    assert npos == {1, 2, 3, 4, 5, 7, 9, 12, 13, 18, 25}
    assert {1, 2, 3} <= npos                                      # waves without a position
    assert {n % 4 for n in npos} == {0, 1, 2, 3} and 4 in npos    # one position per wave
    assert 12 in npos and 13 in npos and {n % 12 for n in npos} >= {0, 1}  # exactly one round; a second round for wave 0 alone
    assert {s % 4 for s in of(new, "slabs") | of(old, "slabs")} == {0, 1, 2, 3}  # db_conv on every wave
    assert of(new, "slabs") == {6, 8, 9, 11}
    assert of(new, "last_slab") == {29, 10, 23, 4} and of(old, "last_slab") == {10, 20, 7}
    assert {(9 * f) % 2 for _, _, _, f in new} == {0, 1}          # odd k1 at F = 21 and F = 31
    assert any(w < h for w, h, _, _ in new) and any(h == 3 for _, h, _, _ in new) and any(w == 3 for w, _, _, _ in new)
    assert any(w == 3 and h == 3 for w, h, _, _ in new)
    assert {p for _, _, p, _ in new} == {1, 2, 3, 4}
    assert all(f == 5 * p + 16 for _, _, p, f in new)
    # row lengths: an odd one, and S % 4 = 3 at P = 3 -- the four row shifts within one tile of (world, seat) samples
    assert (3 * 3 * 21) % 2 == 1 and (7 * 3 * 31) % 4 == 3 and {(s * 651) % 4 for s in range(4)} == {0, 1, 2, 3}
    # the two standard layouts no CNN case has run, and worlds: two tiles at P = 1, the last one ragged at every P
    assert {"forced_coordination", "counter_circuit"} <= set(cases.KEYS) & set(layouts.STANDARD_LAYOUTS)
    assert cases.N > 32 and all((cases.N * p) % 32 for _, _, p, _ in new)
    assert {key for key, *_ in cases.CASES} == set(cases.KEYS) == {case[0] for case in cases.MAPPO_CASES}
    assert {key for key, _, _, inputs in cases.CASES if inputs == "stepped"} == {"forced_coordination", "counter_circuit", "k4x4p3"}


def test_lds_literals_are_the_headers_arithmetic_and_the_librarys_verdict(hip_lib):
    """The table's byte counts are literals; ``lds_bytes`` restates cnn_lds and cnn_update_lds, and the library refuses by shape
    exactly the keys whose update image is past the limit.  (The byte count in ``mrl_cnn_act``'s refusal needs a simulator: the
    GPU file holds it against the same literals.)"""
    largest = 0
    for key, (w, h, p, act, update) in cases.TABLE.items():
        f = 5 * p + 16
        got_act, got_update, region_a, region_a_update = cases.lds_bytes(w, h, f)
        assert (got_act, got_update) == (act, update), key
        out = ctypes.c_uint64(0)
        rc = hip_lib.mrl_mappo_workspace_bytes(w, h, f, 64, cases.B, 1, ctypes.byref(out))
        if key in cases.ACCEPTED:
            assert act <= cases.LDS_LIMIT and update <= cases.LDS_LIMIT and rc == _lib.MRL_OK and out.value > 0, key
            largest = max(largest, update)
        else:
            # refused by the act's image and by the update's alike
            assert act > cases.LDS_LIMIT and update > cases.LDS_LIMIT and rc == _lib.MRL_ERR_INVALID, key
            assert hip_lib.mrl_last_error().decode() == (
                "mrl_mappo_workspace_bytes: the kitchen's LDS image does not fit one workgroup's 160 KiB "
                f"(width {w}, height {h}, channels {f}, hidden 64, minibatch_size {cases.B})"), key
    # near the limit from below (the largest image of the other CNN tests is asymmetric_advantages' 154 464 bytes) and past it
    assert cases.lds_bytes(9, 5, 26)[0] == 154464 < cases.ACCEPTED["multiplayer_schelling/1p"][3] < cases.ACCEPTED["k8x5p4"][3]
    assert largest == 162576 and cases.LDS_LIMIT - largest < 2048
    assert min(act for _, _, _, act, _ in cases.REFUSED.values()) - cases.LDS_LIMIT < 4096


def test_region_a_of_the_update_outgrows_the_acts_where_the_table_says():
    for key in cases.KEYS:
        w, h, p, f = cases.shape(key)
        _, _, region_a, region_a_update = cases.lds_bytes(w, h, f)
        assert (region_a_update > region_a) == (key in cases.REGION_A_GROWS), key
    assert "k3x3p1" in cases.REGION_A_GROWS and "k8x5p4" not in cases.REGION_A_GROWS


@pytest.mark.parametrize("key", list(cases.TABLE))
def test_terrain_is_constructible(key, oracle_lib):
    w, h, p, _, _ = cases.TABLE[key]
    params = cases.layout_params(key)
    assert (params["width"], params["height"], params["num_players"], params["horizon"]) == (w, h, p, cases.HORIZON)
    terrain = np.array(params["terrain"]).reshape(h, w)
    starts = list(zip(params["start_player_x"], params["start_player_y"]))
    assert len(starts) == p == len(set(starts)) and all(terrain[y, x] == TERRAIN["AIR"] for x, y in starts)
    if key.partition("/")[0] not in layouts.LAYOUTS:
        assert (terrain[1:-1, 1:-1] == TERRAIN["AIR"]).all()
        border = np.concatenate([terrain[0], terrain[-1], terrain[1:-1, 0], terrain[1:-1, -1]])
        assert sorted(border[border != TERRAIN["COUNTER"]]) == sorted(TERRAIN[k] for k in ("POT", "ONION", "DISH", "SERVING"))
        # none of the four stations sits on a corner, where no player could face it
        assert all(terrain[y, x] == TERRAIN["COUNTER"] for y in (0, h - 1) for x in (0, w - 1))
        interior = [(x, y) for y in range(1, h - 1) for x in range(1, w - 1)]
        assert starts == interior[:p]
        # the base recipe tables: what a named layout with the three-onion order gets
        base = layouts.get_base_layout_params("cramped_room", cases.HORIZON)
        for name in ("recipe_times", "recipe_values", "placement_in_pot_rew", "dish_pickup_rew", "soup_pickup_rew"):
            assert params[name] == base[name], name
    # the CPU oracle takes it, and a step moves the observations
    orc = oracle_lib.OvercookedOracle(params, 3)
    f = 5 * p + 16
    assert orc.obs.size == 3 * p * h * w * f
    before = orc.obs.copy()
    orc.step(np.full((p, 3), 5, np.int32))
    orc.step(np.zeros((p, 3), np.int32))
    assert orc.obs.shape == before.shape
    orc.close()


@pytest.mark.parametrize("key,n,weights,inputs", cases.CASES)
def test_twin_against_torch_float32_and_the_boundary_condition(key, n, weights, inputs, oracle_lib):
    module = cases.make_module(key, weights)
    obs = cases.case_inputs(key, n, weights, inputs)["obs"]
    w, h, p, f = cases.shape(key)
    assert obs.shape == (n, p, h, w, f) and obs.dtype == np.int8
    rows = cnn_twin.rows_of(obs)
    d_value, d_logp = cases.case_margins(key, n, weights, inputs)
    # float32 against float64 over K <= 800 products of O(1): a few 1e-6 at most; a twin with a wrong index map is off by O(1)
    assert d_value <= 2e-5 and d_logp <= 5e-5, (d_value, d_logp)
    cap_value, cap_logp = cases.layout_margins(key, weights)
    u = cnn_twin.draws(cases.case_seed(key, n, weights, inputs), 0, n, p)
    want = cnn_twin.act(cnn_twin.flat(module), rows, u)
    near = int(cnn_twin.near_boundary(want["cdf"], u).sum())
    print(f"{key} n={n} {weights} {inputs}: d(values) = {d_value:.3e} of {cap_value:.3e}, d(log-probs) = {d_logp:.3e} of {cap_logp:.3e}, "
          f"{near} of {len(rows)} draws near a boundary")
    assert 0 < d_value <= cap_value and 0 < d_logp <= cap_logp
    # a condition of the GPU test, not a measurement: at most 1 % of the rows have their draw within 1e-5 of a boundary
    assert near <= 0.01 * len(rows)
    assert ((want["actions"] >= 0) & (want["actions"] <= 5)).all() and len(np.unique(want["actions"])) > 1


def test_stepped_cases_are_not_the_start_state(oracle_lib):
    for key, n, weights, inputs in cases.CASES:
        if inputs == "stepped":
            obs = cases.case_inputs(key, n, weights, inputs)["obs"]
            assert not all(np.array_equal(obs[0], obs[k]) for k in range(1, n)), key  # the worlds went different ways


@pytest.mark.parametrize("key", cases.KEYS)
def test_integer_constructions_stay_exact_in_float32(key):
    """forward (both nets) and the critic's back-propagation: every sum of absolute terms is below 2^24 at ``cnn_twin``'s own
    densities -- F = 36 and npos = 25 make longer sums than any earlier case, and none comes near the bound, so no key is thinned"""
    layers, obs = cases.integer_case(key)
    w, h, p, f = cases.shape(key)
    assert obs.shape == (cnn_twin.INTEGER_N, p, h, w, f) and layers["actor"][0][0].shape == (32, f, 3, 3)
    assert layers["actor"][1][0].shape == (64, 32 * (w - 2) * (h - 2))
    values, logits, bound = cnn_twin.integer_forward(layers, cnn_twin.rows_of(obs))
    update = cases.update_integer_case(key)
    print(f"{key}: forward bound {bound} = 2^{np.log2(bound):.1f}, update bound {update['bound']} = 2^{np.log2(update['bound']):.1f}")
    assert bound < 2 ** 24 and update["bound"] < 2 ** 24
    params = cnn_twin.integer_params(layers)
    assert np.abs(params).max() < 2 ** 24 and (params == np.round(params)).all()
    v64, l64 = cnn_twin.forward(params, cnn_twin.rows_of(obs))
    assert np.array_equal(v64, values) and np.array_equal(l64, logits)
    lo, hi = cnn_twin.TIE
    assert (logits[:, lo] == logits[:, hi]).all() and (logits.argmax(axis=1) == lo).all() and (logits[:, hi] == logits.max(axis=1)).all()
    assert len(np.unique(values)) > len(values) // 2 and (values != 0).any()
    conv = layers["actor"][0][0]
    assert not np.array_equal(conv, conv.transpose(0, 1, 3, 2))  # not symmetric in (i, j)
    # the last (f, i, j) of every channel -- the product next to the pad of an odd K -- carries weight and meets nonzero inputs
    assert np.abs(conv[:, -1, 2, 2]).sum() > 0 and np.abs(cnn_twin.rows_of(obs)[..., -1]).sum() > 0
    # every output position of the convolution feeds fc1 with weight somewhere, in both nets: a position left out shows
    npos = (w - 2) * (h - 2)
    for net in ("actor", "critic"):
        assert (np.abs(layers[net][1][0]).reshape(64, 32, npos).sum(axis=(0, 1)) > 0).all(), (key, net)
    # the update: B = 64 distinct samples, a gradient in every layer, asymmetric matrices
    assert update["indices"].shape == (1, 64) and len(np.unique(update["indices"])) == 64
    assert len(update["batch"].ring) == 2 * mappo_twin.N * p >= 64
    assert update["grad"].size == params.size - mappo_twin.actor_size(key)
    for name, matrix in update["matrices"].items():
        assert np.abs(matrix).max() > 0 and (matrix.shape[0] != matrix.shape[1] or not np.array_equal(matrix, matrix.T)), (key, name)
    # ... and every column of dW_conv's last slab and every position's block of dW_fc1 is somewhere nonzero
    last = cases.classes(w, h, f)["last_slab"]
    assert (np.abs(update["matrices"]["conv"][:, -last:]).sum(axis=0) > 0).all(), key
    assert (np.abs(update["matrices"]["fc1"]).reshape(64, 32, npos).sum(axis=(0, 1)) > 0).all(), key


@pytest.mark.parametrize("case", cases.MAPPO_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_input_conditions_of_every_update_row(case):
    """conditions, not measurements (tests/test_mappo_update_api.py): in the twin no sample lies within KINK of a kink of the loss,
    no pre-activation is closer to 0 than 8 x the largest float32-vs-twin pre-activation distance unless it is exactly 0 in both,
    and the batches put their samples on every branch"""
    fixed = cases.fixed_case(case)
    exact, width = fixed["twin"], case[4]
    closest, worst = mappo_twin.relu_margin(fixed)
    d = mappo_twin.row_margins(exact, fixed["f32"])
    print(case, "kink", exact["kink"], "closest pre-activation", closest, "worst float32 distance", worst, "d(grad) = %.3e" % d["grad"])
    assert exact["kink"] > mappo_twin.KINK, (case, exact["kink"])
    assert closest > mappo_twin.FACTOR * worst, (case, closest, worst)
    assert mappo_twin.conditions_hold(fixed)
    w, h, p, f = cases.shape(case[0])
    assert len(fixed["batch"].ring) == cases.T * case[1] * p and fixed["batch"].ring.shape[1:] == (h, w, f)
    assert (fixed["indices"] >= 0).all() and (fixed["indices"] < len(fixed["batch"].ring)).all()
    assert fixed["indices"].shape == (1, width) and len(np.unique(fixed["indices"][0])) == width
    b = exact["branches"]
    assert b["ratio_clipped"] >= 0.25 and b["value_clipped"] >= 0.25 and min(b["clipped_high"], b["clipped_low"]) >= 0.1, (case, b)
    assert min(b["huber_above"], b["huber_below"]) >= 0.05, (case, b)
    assert 0 < d["grad"] < 1e-4


def test_pooled_stat_margins_cover_every_row():
    pooled = cases.stat_margins()
    for case in cases.MAPPO_CASES:
        fixed = cases.fixed_case(case)
        own = mappo_twin.row_margins(fixed["twin"], fixed["f32"])
        assert all(own[name] <= pooled[name] for name in mappo_twin.STATS)
    print("pooled d of the stats:", {name: "%.2e" % value for name, value in pooled.items()})
    assert all(pooled[name] > 0 for name in mappo_twin.STATS if name != "clipfrac")


def test_other_keys_keep_cnn_twins_answer_and_the_substitution_ends():
    assert cnn_twin.shape("cramped_room") == (5, 4, 2, 26) and cnn_twin.shape("k4x4p3") == (4, 4, 3, 31)
    # the two standard layouts have the shape cnn_twin itself reads off ``layouts``
    for key in ("forced_coordination", "counter_circuit"):
        assert cases.shape(key) == cases._others_shape(key)
    assert cnn_twin.shape("multiplayer_schelling/1p") == (7, 7, 1, 21) and cnn_twin.shape("multiplayer_schelling") == (7, 7, 4, 36)
    inner = cnn_twin.shape
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(cnn_twin, "shape", cases._others_shape)
        with pytest.raises(KeyError):
            cnn_twin.shape("k4x4p3")
        with cases.shapes():
            assert cnn_twin.shape("k4x4p3") == (4, 4, 3, 31)
        with pytest.raises(KeyError):
            cnn_twin.shape("k4x4p3")
    assert cnn_twin.shape is inner
