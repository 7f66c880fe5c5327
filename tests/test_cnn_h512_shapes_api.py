"""No GPU: what tests/test_gpu_cnn_h512_shapes.py rests on (tests/cnn_h512_shape_cases.py) -- how many draws of each forward case
lie near a boundary, that every d is positive, the exact-integer construction's bound at every integer key (K2 up to 6400), the
literal 512 LDS images against the headers' arithmetic, and the parameter count at every key of the table."""
import numpy as np
import pytest

import cnn_h512_shape_cases as cases
import cnn_twin as twin
import kitchen_shape_cases as table
from madrona_rl_envs_playground_amd.simulators import CnnActorCritic


def test_the_cases_run_every_class_they_are_there_for():
    shapes = {key: cases.shape(key) for key in cases.KEYS}
    ran = {(key, n) for key, n, _ in cases.FORWARD}
    assert {(key, cases.N) for key in cases.KEYS} <= ran
    assert {(w - 2) * (h - 2) for w, h, _, _ in shapes.values()} >= {1, 2, 3, 4, 7, 12, 13, 25}
    assert {f for _, _, _, f in shapes.values()} >= {21, 31, 36} and max(256 * (w - 2) * (h - 2) for w, h, _, _ in shapes.values()) == 6400
    # masks with a gap (or a seat alone) at P = 3 and P = 4; tile counts with no ragged tail; calls of one and two samples
    assert sorted((cases.shape(key)[2], mask) for key, _, mask in cases.MASKED) == [(3, 0b010), (3, 0b101), (4, 0b0111), (4, 0b1010)]
    samples = sorted(n * cases.shape(key)[2] for key, n, _ in cases.TILE_EDGES)
    assert samples == [1, 2, 32, 64, 96]
    # the integer keys: 9 F odd (F 21 and 31), F 36, all four row shifts, npos 1, 13 and 25
    integer = [cases.shape(key) for key in cases.INTEGER_KEYS]
    assert {f for _, _, _, f in integer} == {21, 26, 31, 36} and sum(9 * f % 2 for _, _, _, f in integer) >= 3
    assert {(w - 2) * (h - 2) for w, h, _, _ in integer} >= {1, 4, 5, 12, 13, 25} and "k7x3p3" in cases.INTEGER_KEYS
    assert {cases.simulator(key) for key, *_ in cases.ROLLOUTS} == {"SimplecookedSimulator", "OvercookedSimulator"}
    assert max(cases.shape(key)[2] for key, *_ in cases.ROLLOUTS) == 4


@pytest.mark.parametrize("key,n", sorted({case[:2] for case in cases.FORWARD}))
def test_reference_draws_and_margins(key, n):
    ref = cases.reference(key, n)
    w, h, p, f = cases.shape(key)
    assert ref["obs"].shape == (n, p, h, w, f) and ref["obs"].dtype == np.int8
    print(f"{key} n={n}: d(values) = {ref['d_value']:.3e}, d(log-probs) = {ref['d_logp']:.3e}, d(logits) = {ref['d_logits']:.3e}, "
          f"{int(ref['near'].sum())} of {n * p} draws near a boundary")
    assert ref["near"].sum() <= 1  # at most one row whose action a float32 evaluation may decide otherwise
    # float32 against float64 over K <= 6400 products of O(1); a wrong view (H and W swapped) is off by O(1)
    assert 0 < ref["d_value"] <= 1e-4 and 0 < ref["d_logp"] <= 1e-4 and 0 < ref["d_logits"] <= 1e-4
    assert n * p < 6 or len(np.unique(ref["actions"])) > 1
    # a case of a few rows: its own d is a usable unit (float32's results differ from host to host; the GPU test asserts the same)
    for kind, (own, full) in cases.small_case_unit(key, n).items():
        assert 8 * own >= full, (key, n, kind, own, full)


@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_integer_construction_stays_exact_in_float32(key):
    layers, obs = cases.integer_case(key)
    values, logits, bound = twin.integer_forward(layers, twin.rows_of(obs))
    params = twin.integer_params(layers)
    print(f"{key}: bound {bound} = 2^{np.log2(bound):.1f}")
    assert bound < 2 ** 24 and np.abs(params).max() < 2 ** 24
    w, h, p, f = cases.shape(key)
    assert obs.shape == (33, p, h, w, f)
    assert params.size == sum(q.numel() for q in CnnActorCritic(w, h, f, hidden=512).parameters())
    # the outputs tell samples and columns apart
    assert len(np.unique(values)) > len(values) // 2 and len(np.unique(logits)) > logits.size // 4
    # the last (f, i, j) of every channel -- the product next to the pad of an odd K -- carries weight and meets nonzero inputs
    assert np.abs(layers["actor"][0][0][:, -1, 2, 2]).sum() > 0 and np.abs(twin.rows_of(obs)[..., -1]).sum() > 0


def test_lds_literals_and_parameter_counts(hip_lib):
    assert cases.BEHIND_FC1 == 66688 and set(cases.LDS) == set(table.TABLE)
    for key, (w, h, p, act, _) in table.TABLE.items():
        f = 5 * p + 16
        assert cases.LDS[key] == max(table.lds_bytes(w, h, f)[0], cases.BEHIND_FC1) == max(act, 66688), key
        assert (cases.LDS[key] > cases.LDS_LIMIT) == (key in cases.REFUSED_KEYS), key
        count = sum(q.numel() for q in CnnActorCritic(w, h, f, hidden=512).parameters())
        assert int(hip_lib.mrl_cnn_policy_num_params(w, h, f, 512, 6)) == count, key
    # both layouts of the image occur, and the two accepted images nearest the limit are the plain act's
    assert sum(cases.LDS[key] == cases.BEHIND_FC1 for key in cases.KEYS) == 3
    assert sorted(cases.LDS[key] for key in cases.KEYS)[-2:] == [cases.LDS["multiplayer_schelling/1p"], cases.LDS["k8x5p4"]]
