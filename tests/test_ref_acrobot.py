"""CPU: tests/golden/acrobot_ref.npz IS what the reference's own Acrobot sim.cpp computes (regenerated here from the
reference tree when there is one, compiled unchanged: tests/golden/make_acrobot_golden.py), the float64 twin
(tests/acrobot_twin.py) is as close to it as the fixture's tolerance says, and the reference's truncation is the per-world
one of this engine at N = 1 only.  The same for tests/golden/acrobot_far_ref.npz, the transitions from far angles, whose
inputs must also lie on the kernel paths they are named after."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

import acrobot_twin as twin
from conftest import GOLDEN, load_golden

_spec = importlib.util.spec_from_file_location("make_acrobot_golden", os.path.join(GOLDEN, "make_acrobot_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def golden():
    return load_golden("acrobot_ref.npz")


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    if not os.path.isfile(gen.reference_sim()):
        pytest.skip("no reference tree (%s): the committed fixture cannot be regenerated here" % gen.reference_sim())
    if shutil.which("g++") is None:
        pytest.skip("no g++ to compile the reference's sim.cpp with")
    return gen.build_driver(str(tmp_path_factory.mktemp("acrobot_ref")))


def test_fixture_is_what_the_reference_computes(ref_lib, golden):
    """Arrays the reference wrote must match bit for bit.  The twin's float64 results and the tolerances derived from them
    depend on this machine's double-precision cos / sin as well, hence 1e-9 relative."""
    fresh = gen.generate(ref_lib)
    assert sorted(fresh) == sorted(golden)
    for key, want in golden.items():
        got = np.asarray(fresh[key])
        assert got.shape == want.shape and got.dtype == want.dtype, key
        if key.endswith(("_next64", "_tol")):
            assert np.allclose(got, want, rtol=1e-9, atol=1e-15), key
        else:
            assert got.tobytes() == np.asarray(want).tobytes(), key


def test_fixture_shape_and_coverage(golden):
    assert golden["fresh"].shape == (8192, 4) and golden["fresh_last"].shape == (8, 4)
    assert (np.abs(golden["fresh"]) <= 0.1).all() and len(np.unique(golden["fresh"], axis=0)) >= 8180
    assert int(golden["quiet_episodes"]) == 8192
    for name in ("reach", "swing"):
        assert golden[name + "_state"].shape == (2048, 4) and golden[name + "_next64"].dtype == np.float64
        assert set(np.unique(golden[name + "_action"])) == {0, 1, 2}
        assert (golden[name + "_tol"] > 0).all() and (golden[name + "_tol"] < 1e-5).all()
    done = golden["swing_done"].mean()
    assert 0.10 < done < 0.25, "about 17 % of the swing set terminates"
    assert golden["clamp_state"].shape == (64, 4) and golden["clamp_mask"].any(axis=1)[golden["clamp_done"] == 0].all()
    assert 0 < golden["clamp_done"].sum() < 64
    bound = np.array([twin.MAX_VEL_1, twin.MAX_VEL_2], np.float32)
    assert (np.abs(golden["clamp_next"][:, 2:])[golden["clamp_mask"]] == np.broadcast_to(bound, (64, 2))[golden["clamp_mask"]]).all()
    assert os.path.getsize(os.path.join(GOLDEN, "acrobot_ref.npz")) < 512 * 1024


def test_twin_is_within_a_quarter_of_the_tolerance(golden):
    """tol = 4 x the reference's largest distance from the twin: the twin restated here must reproduce that distance, no
    transition left out, and agree on every done flag (the generator dropped what lies within 1e-3 of the threshold)."""
    for name in ("reach", "swing"):
        nxt, height, _ = twin.step(golden[name + "_state"], golden[name + "_action"])
        assert (np.abs(height - 1.0) > 1e-3).all()
        assert np.array_equal(height > 1.0, golden[name + "_done"] != 0)
        assert np.allclose(nxt, golden[name + "_next64"], rtol=1e-9, atol=1e-15)
        live = golden[name + "_done"] == 0
        err = twin.distance(golden[name + "_next"][live], nxt[live])
        assert (err <= golden[name + "_tol"] / 4 * (1 + 1e-6)).all()
        assert (err.max(axis=0) >= golden[name + "_tol"] / 4 * (1 - 1e-6)).all(), "the tolerance is the measured one"
    nxt, height, _ = twin.step(golden["clamp_state"], golden["clamp_action"])
    assert np.array_equal(height > 1.0, golden["clamp_done"] != 0)


@pytest.fixture(scope="module")
def far():
    return load_golden("acrobot_far_ref.npz")


FAR_SETS = [name for name, _, _, _ in gen.FAR]
LOOP_END = twin.PI_F + 64 * 2 * twin.PI_F  # what the 64 trips of the kernel's wrap_plain still bring back into [-pi, pi]


def test_far_fixture_is_what_the_reference_computes(ref_lib, far):
    """acrobot_far_ref.npz, regenerated from the reference tree: the reference's arrays bit for bit, the twin's at 1e-9"""
    fresh = gen.generate_far(ref_lib)
    assert sorted(fresh) == sorted(far)
    for key, want in far.items():
        got = np.asarray(fresh[key])
        assert got.shape == want.shape and got.dtype == want.dtype, key
        if key.endswith(("_next64", "_tol")):
            assert np.allclose(got, want, rtol=1e-9, atol=1e-15), key
        else:
            assert got.tobytes() == np.asarray(want).tobytes(), key


@pytest.mark.parametrize("name", FAR_SETS)
def test_far_twin_is_within_a_quarter_of_the_tolerance(name, far):
    """as test_twin_is_within_a_quarter_of_the_tolerance: the twin reproduces tol / 4 as the largest distance, nothing left
    out, and agrees on every done flag outside the set's band"""
    band = dict((n, b) for n, _, _, b in gen.FAR)[name]
    assert far[name + "_state"].shape == (512, 4) and far[name + "_state"].dtype == np.float32
    assert far[name + "_next"].shape == (512, 4) and far[name + "_next64"].dtype == np.float64
    nxt, height, _ = twin.step(far[name + "_state"], far[name + "_action"])
    assert (np.abs(height - 1.0) > band).all()
    assert np.array_equal(height > 1.0, far[name + "_done"] != 0)
    assert np.allclose(nxt, far[name + "_next64"], rtol=1e-9, atol=1e-15)
    live = far[name + "_done"] == 0
    err = twin.distance(far[name + "_next"][live], nxt[live])
    assert (err <= far[name + "_tol"] / 4 * (1 + 1e-6)).all()
    assert (err.max(axis=0) >= far[name + "_tol"] / 4 * (1 - 1e-6)).all(), "the tolerance is the measured one"
    assert (np.abs(far[name + "_next"][live][:, :2]) <= np.float32(np.pi)).all(), "the reference wrapped every live angle"
    assert 0.05 < (~live).mean() < 0.30, "between 5 % and 30 % of the set finishes"
    print(f"acrobot far {name}: reference to twin {far[name + '_tol'] / 4}, {int((~live).sum())} finished, "
          f"{int(far[name + '_dropped'])} dropped at the threshold, {int(far[name + '_offpath'])} off the path")


@pytest.mark.parametrize("name", FAR_SETS)
def test_far_inputs_reach_their_path(name, far):
    """What makes a set take its path through csrc/acrobot.hip is a property of its INPUTS, asserted from the twin with a
    margin far above any float32 rounding of these angles (1.2e-4 at 2000): the new angle before the wrap against 3 pi,
    5 pi (wrap_fast brings back two turns) and pi + 64 * 2 pi (wrap_plain's loops), and the largest stage angle against
    kFastRange = 128."""
    state, action = far[name + "_state"], far[name + "_action"]
    lo, hi = dict((n, (a, b)) for n, a, b, _ in gen.FAR)[name]
    is_far = np.abs(state[:, :2].astype(np.float64)) > twin.PI_F
    assert is_far.any(axis=1).all()
    assert ((np.abs(state[:, :2])[is_far] >= np.float32(lo)) & (np.abs(state[:, :2])[is_far] <= np.float32(hi))).all()
    assert (np.abs(state[:, 2]) <= 3).all() and (np.abs(state[:, 3]) <= 6).all()
    _, _, _, raw, reach = twin.step(state, action, detail=True)
    assert (reach >= np.abs(state[:, :2]).max(axis=1)).all()
    new = np.abs(raw)[is_far]                       # every far angle's new value
    wide = np.repeat(reach, is_far.sum(axis=1))     # and its world's reach
    if name == "turns2":
        assert ((new > 3 * twin.PI_F + 0.05) & (new < 5 * twin.PI_F - 0.05)).all() and (wide < 127).all()
    elif name == "turns3":
        assert (new > 5 * twin.PI_F + 0.05).all() and (wide < 127).all()
    elif name == "beyond":
        assert (wide > 129).all() and (new < LOOP_END - 1).all()
    else:
        assert (new > LOOP_END + 1).all()
    assert (np.abs(raw)[~is_far] < 3 * twin.PI_F - 0.05).all()  # the other angle: at most one turn off
    assert np.array_equal(gen.on_path(name, state, action), np.ones(512, bool))
    # theta1 only, theta2 only, both; every action; both signs
    patterns = set(map(tuple, is_far.tolist()))
    assert patterns == {(True, False), (False, True), (True, True)}
    assert min((is_far == p).all(axis=1).sum() for p in patterns) > 100
    assert set(np.unique(action)) == {0, 1, 2}
    assert (state[:, :2][is_far] > 0).any() and (state[:, :2][is_far] < 0).any()


def test_far_fixture_size():
    assert os.path.getsize(os.path.join(GOLDEN, "acrobot_far_ref.npz")) < 256 * 1024


def test_reference_truncation_at_one_world(ref_lib, golden):
    """N = 1: an untouched episode under zero torque ends at its 501st step, and again 501 steps later; the world then holds
    the next episode's start state and REWARD is -1 on every step, the last included."""
    ref = gen.RefAcrobot(ref_lib, 1)
    assert np.array_equal(ref.state, golden["fresh"][0:1]) and ref.reward[0] == 0 and ref.episodes == 1
    zero = np.ones(1, np.int32)
    for episode in (1, 2):
        for t in range(1, twin.MAX_STEPS + 2):
            ref.step(zero)
            assert ref.reward[0] == -1.0
            assert bool(ref.done[0]) == (t == twin.MAX_STEPS + 1), (episode, t)
        assert np.array_equal(ref.state.view(np.uint32), golden["fresh"][episode:episode + 1].view(np.uint32))
        assert ref.episodes == episode + 1
    ref.close()


def test_reference_length_is_shared_between_worlds(ref_lib):
    """What this engine departs from: with N = 4 worlds the ONE length counts 4 per step, passes 500 in step 126, and
    world 0 -- the first visited -- alone is reset."""
    ref = gen.RefAcrobot(ref_lib, 4)
    zero = np.ones(4, np.int32)
    for t in range(1, 127):
        ref.step(zero)
        assert ref.done.tolist() == ([1, 0, 0, 0] if t == 126 else [0, 0, 0, 0]), t
    ref.close()
