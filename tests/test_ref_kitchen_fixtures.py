"""tests/golden/overcooked_ref_*.npz and simplecooked_ref_*.npz: what the reference's own kitchen sim.cpp files computed,
compiled unchanged against the Madrona stand-in (tests/golden/make_ref_golden.py, streams in tests/kitchen_ref.py).  They
keep the oracle and the GPU pinned to the compiled C++ where oracle/_ref is not built."""
import os

import numpy as np
import pytest

import kitchen_ref as kr
from oracle import ref
from oracle.oracle import OvercookedOracle, SimplecookedOracle


@pytest.mark.parametrize("fixture", sorted(kr.FIXTURES))
def test_fixture_is_what_the_compiled_reference_computes(fixture):
    """Recorded again from oracle/_ref: every stored array comes out byte for byte."""
    ref.require()
    make_ref = ref.RefOvercooked if kr.fixture_game(fixture) == "overcooked" else ref.RefSimplecooked
    arrays, _ = kr.record_fixture(fixture, make_ref)
    z = np.load(os.path.join(kr.GOLDEN, fixture + ".npz"))
    assert sorted(z.files) == sorted(arrays)
    for k in z.files:
        again = np.asarray(arrays[k])
        assert z[k].dtype == again.dtype and z[k].shape == again.shape and z[k].tobytes() == again.tobytes(), f"{fixture}: {k}"


@pytest.mark.parametrize("fixture", sorted(kr.FIXTURES))
def test_oracle_reproduces_fixture(fixture):
    """Needs no reference build: the oracle steps through the recorded actions and meets the recorded bytes."""
    game = kr.fixture_game(fixture)
    for prefix, params, s in kr.load_fixture(fixture):
        n = s["actions"].shape[2]
        orc = (OvercookedOracle if game == "overcooked" else SimplecookedOracle)(params, n)
        assert np.array_equal(orc.obs, s["first_obs"]), f"{fixture} {prefix}: first obs"
        for t, a in enumerate(s["actions"]):
            orc.step(a)
            assert np.array_equal(orc.obs, s["obs"][t]), f"{fixture} {prefix}: obs, step {t}"
            assert np.array_equal(orc.reward, s["reward"][t]), f"{fixture} {prefix}: reward, step {t}"
            assert np.array_equal(orc.done, s["done"][t]), f"{fixture} {prefix}: done, step {t}"
        for name, got in zip(("players", "objects", "timestep", "dishes_out"), orc.dump()):
            assert np.array_equal(got, s[name]), f"{fixture} {prefix}: {name} after the last step"
        orc.close()
