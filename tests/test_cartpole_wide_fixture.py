"""CPU: tests/golden/cartpole_wide.npz (tests/golden/make_cartpole_wide_golden.py) -- one-step Cartpole transitions from
pole angles beyond pi / 4 -- is what it says it is: every angle on the far side of the kernels' bounded sin / cos, the
`survive` set alive and the `finish` set finished on both the oracle's and the float64 reference's side, the oracle's
float32 results bit for bit, the tolerance 4 x the oracle's measured distance from the reference's float64 step, and, where
there is a reference tree, the float64 results regenerated from it."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden

_spec = importlib.util.spec_from_file_location("make_cartpole_wide_golden", os.path.join(GOLDEN, "make_cartpole_wide_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

QUARTER_PI = np.pi / 4


@pytest.fixture(scope="module")
def wide():
    return load_golden("cartpole_wide.npz")


def test_shapes_and_ranges(wide):
    assert sorted(wide) == sorted(["survive_state", "survive_action", "survive_next", "survive_done", "survive_next64", "survive_tol",
                                   "finish_state", "finish_action", "finish_next64", "finish_done"])
    for name in ("survive", "finish"):
        state, action = wide[name + "_state"], wide[name + "_action"]
        assert state.shape == (512, 4) and state.dtype == np.float32 and action.shape == (512,) and action.dtype == np.int32
        assert wide[name + "_next64"].shape == (512, 4) and wide[name + "_next64"].dtype == np.float64
        assert set(np.unique(action)) == {0, 1}
        assert (np.abs(state[:, 2]) > QUARTER_PI + 0.01).all(), "every angle takes the library's sincosf"
        assert (state[:, 2] > 0).sum() > 150 and (state[:, 2] < 0).sum() > 150
        assert (np.abs(state[:, 0]) <= 1.5).all() and np.isfinite(wide[name + "_next64"]).all()
    theta = np.abs(wide["survive_state"][:, 2])
    assert theta.min() >= np.float32(0.8) and theta.max() <= 3.0 and (theta > 1.5).sum() > 100
    assert (np.abs(wide["survive_next64"][:, 2]) < 0.15 + 1e-5).all() and (np.abs(wide["survive_next64"][:, 0]) < 2.0).all()
    theta = np.abs(wide["finish_state"][:, 2])
    assert theta.min() >= np.float32(0.8) and theta.max() <= 1e4
    assert all(((theta > lo) & (theta <= 10 * lo)).sum() > 60 for lo in (1, 10, 100, 1000)), "log-uniform up to 1e4"
    assert (np.abs(wide["finish_state"][:, [1, 3]]) <= 4).all()
    assert (np.abs(wide["finish_next64"][:, [1, 3]]) < 4.5).all()  # below 8: rounding a new rate to float moves it by at most 2.4e-7
    assert os.path.getsize(os.path.join(GOLDEN, "cartpole_wide.npz")) < 128 * 1024


def _finishes(next64):
    return (np.abs(next64[:, 0]) > gen.X_TH) | (np.abs(next64[:, 2]) > gen.TH_TH)


def test_done_flags_and_tolerance(wide, oracle_lib):
    """no world of `survive` finishes and every world of `finish` does, clear of the thresholds, on the reference's side
    (next64) and on the oracle's; survive_next is the oracle's result and survive_tol 4 x its distance from next64"""
    assert not _finishes(wide["survive_next64"]).any() and not wide["survive_done"].any()
    assert (np.abs(wide["survive_next64"][:, 2]) < gen.TH_TH - 0.05).all()
    assert _finishes(wide["finish_next64"]).all() and wide["finish_done"].all()
    assert (np.abs(wide["finish_next64"][:, 2]) > gen.TH_TH + 0.4).all()
    for name in ("survive", "finish"):
        nxt, done = gen.oracle_step(wide[name + "_state"], wide[name + "_action"])
        assert np.array_equal(done, wide[name + "_done"])
        if name == "survive":
            assert nxt.tobytes() == wide["survive_next"].tobytes()
            err = np.abs(nxt.astype(np.float64) - wide["survive_next64"]).max(axis=0)
            assert np.array_equal(4.0 * err, wide["survive_tol"]) and (err > 0).all()
            print(f"cartpole wide survive: the oracle's largest distance from the float64 reference {err}, in float spacings "
                  f"{(np.abs(nxt.astype(np.float64) - wide['survive_next64']) / np.spacing(np.abs(nxt))).max(axis=0)}")


def test_fixture_is_what_the_reference_computes(wide):
    if not os.path.isfile(gen.reference_env()):
        pytest.skip("no reference tree (%s): the committed fixture cannot be regenerated here" % gen.reference_env())
    fresh = gen.generate()
    assert sorted(fresh) == sorted(wide)
    for key, want in wide.items():
        got = np.asarray(fresh[key])
        assert got.shape == want.shape and got.dtype == want.dtype, key
        if key.endswith("_next64"):
            assert np.allclose(got, want, rtol=1e-12, atol=0), key
        elif key.endswith("_tol"):
            assert np.allclose(got, want, rtol=1e-6, atol=0), key  # (a difference of float32 and float64 values)
        else:
            assert got.tobytes() == want.tobytes(), key
