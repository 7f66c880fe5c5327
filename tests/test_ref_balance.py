"""CPU oracle (oracle/balance_oracle.c) against the reference's own balance-beam sim.cpp compiled unchanged against the
Madrona stand-in (oracle/_ref, oracle/ref.py): reset positions, episode order, both observation rows, positions, time,
reward and done, bit for bit, over every reachable state.  Two reference instances (0x00 without constructors, 0xA5 with
default-initialisation) must agree, and no guard byte may be written."""
import numpy as np
import pytest

from oracle import ref
from oracle.oracle import BalanceOracle


@pytest.fixture(scope="module", autouse=True)
def _ref_built():
    ref.require()


def test_oracle_matches_compiled_reference_on_every_reachable_state():
    n, steps = 4000, 240
    orc = BalanceOracle(n)
    refs = [ref.RefBalance(n), ref.RefBalance(n, fill=0xA5, construct=True)]
    rng = np.random.default_rng(11)
    seen = set()

    def same(where):
        for r in refs:
            for k in ("obs", "loc", "time", "reward", "done"):
                assert np.array_equal(getattr(r, k), getattr(orc, k)), f"{where}: {k}"
            assert r.episodes == orc.episodes, f"{where}: episode counter"
            assert not len(r.guards()), f"{where}: guard bytes written"

    same("create")
    for t in range(steps):
        a = rng.integers(0, 4, size=(2, n)).astype(np.int32)
        # a quarter of the worlds stay on the beam as long as they can (moves of +-1 toward the middle)
        calm = np.arange(n) % 4 == 0
        toward = np.where(orc.loc < 2, 2, 1).astype(np.int32)
        a[:, calm] = toward[:, calm]
        orc.step(a)
        for r in refs:
            r.step(a)
        same(f"step {t}")
        seen.update(zip(orc.loc[0].tolist(), orc.loc[1].tolist(), orc.time.tolist()))
    # every (position, position, time) a world can be in between steps: a fresh deal has time 2 (sim.cpp's resetWorld,
    # TIME - 1), one move later it is 1 on the beam; time 0 always resets
    assert seen >= {(p, q, s) for p in range(5) for q in range(5) for s in (1, 2)}, len(seen)
    assert orc.episodes > 3 * n
