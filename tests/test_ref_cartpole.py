"""CPU oracle (oracle/cartpole_oracle.c, the reference's own typing: float state, double intermediates, no FMA contraction)
against the reference's own Cartpole sim.cpp compiled unchanged against the Madrona stand-in (oracle/_ref, oracle/ref.py):
reset states and episode order, and long lock-steps that end episodes at both thresholds, bit for bit.  Components start
as 0x00 without constructors on one reference instance and as 0xA5 with default-initialisation on the other; both must
agree, and no guard byte may be written."""
import numpy as np
import pytest

from oracle import ref
from oracle.oracle import CartpoleOracle

X_TH, TH_TH = 2.4, 12 * 2 * np.pi / 360


@pytest.fixture(scope="module", autouse=True)
def _ref_built():
    ref.require()


def _policy(t, state, w):
    """world w % 3: always right, always left, or balance the pole (push toward theta) so that the cart drifts out."""
    pol = w % 3
    balance = (state[:, 2] + 0.3 * state[:, 3] > 0).astype(np.int32)
    return np.where(pol == 0, 1, np.where(pol == 1, 0, balance)).astype(np.int32)


def _same(where, orc, refs):
    for r in refs:
        assert np.array_equal(r.state.view(np.uint32), orc.state.view(np.uint32)), f"{where}: state"
        assert np.array_equal(r.reward, orc.reward), f"{where}: reward"
        assert np.array_equal(r.done, orc.done), f"{where}: done"
        assert r.episodes == orc.episodes, f"{where}: episode counter"
        assert not len(r.guards()), f"{where}: guard bytes written"


def test_reset_states_and_episode_order():
    n = 5000
    orc = CartpoleOracle(n)
    refs = [ref.RefCartpole(n), ref.RefCartpole(n, fill=0xA5, construct=True)]
    _same("create", orc, refs)
    assert orc.episodes == n and (np.abs(orc.state) <= 0.05).all()
    # every world ends on the same step (always push right, identical dynamics up to the fresh state): a batch of resets
    # takes the next indices in ascending world order on both sides
    for t in range(60):
        a = np.ones(n, np.int32)
        orc.step(a)
        for r in refs:
            r.step(a)
        _same(f"step {t}", orc, refs)
    assert orc.episodes > 2 * n


def test_lockstep_near_both_thresholds():
    n, steps = 3000, 1500
    orc = CartpoleOracle(n)
    refs = [ref.RefCartpole(n), ref.RefCartpole(n, fill=0xA5, construct=True)]
    w = np.arange(n)
    by_x = by_theta = 0
    for t in range(steps):
        before = orc.state.copy()
        a = _policy(t, before, w)
        orc.step(a)
        for r in refs:
            r.step(a)
        _same(f"step {t}", orc, refs)
        d = orc.done[:, 0] == 1
        # which threshold ended it: the one the pre-step state was closest to (relative distance)
        near_x = np.abs(before[:, 0]) / X_TH > np.abs(before[:, 2]) / TH_TH
        by_x += int((d & near_x).sum())
        by_theta += int((d & ~near_x).sum())
    print(f"cartpole: {n * steps} world-steps bit-exact, {orc.episodes} episodes ({by_x} ended at |x| = 2.4, "
          f"{by_theta} at |theta| = 12 deg)")
    assert by_x >= 10 and by_theta >= 10
