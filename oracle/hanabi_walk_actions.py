"""TEST INFRASTRUCTURE ONLY -- writes the action streams of tests/hanabi_illegal_cases.py:walk (the device tests' own worlds,
steps and seed, every configuration of WALK_CONFIGS) for oracle/hanabi_walk_replay.c, which replays them through the oracle
under the sanitizers (`make -C oracle sanitize-hanabi`).  The oracle is stepped on the RAW actions
(the reference's own behaviour, self-hints included).  The walk draws from the oracle's mask and records, so the oracle
(the ordinary shared library) plays it here; the stream ends with a checksum of everything it held after each step.

    python oracle/hanabi_walk_actions.py OUT_DIR
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

import hanabi_illegal_cases as ic  # noqa: E402
from oracle import oracle  # noqa: E402


def fold(h, a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).astype(np.uint64)
    s = int((b * (np.arange(b.size, dtype=np.uint64) % np.uint64(65521) + np.uint64(1))).sum()) & 0xFFFFFFFF
    return (h * 16777619 + s) & 0xFFFFFFFF


def main(out_dir):
    oracle.build()
    os.makedirs(out_dir, exist_ok=True)
    for name in ic.WALK_CONFIGS:
        cfg = ic.config_of(name)
        orc = oracle.HanabiOracle(cfg, ic.WORLDS)
        head = [cfg["colors"], cfg["ranks"], cfg["max_information_tokens"], cfg["max_life_tokens"], ic.WORLDS, ic.STEPS]
        h, total = 2166136261, {}
        with open(os.path.join(out_dir, f"hanabi_walk_{name}.i32"), "wb") as f:
            f.write(np.array(head, "<i4").tobytes())
            for _, rec, acts, cls in ic.walk(orc, cfg, reference_contract=True):
                f.write(acts.astype("<i4").tobytes())
                for a in (orc.obs, orc.state, orc.mask, orc.done, orc.dump()):
                    h = fold(h, a)
                for k in "ABE":
                    total[k] = total.get(k, 0) + int((cls == getattr(ic, k)).sum())
            f.write(np.array([h], "<u4").tobytes())
        print(f"{name}: {ic.WORLDS} worlds x {ic.STEPS} steps, classes {total}, checksum {h:08x}")


if __name__ == "__main__":
    main(sys.argv[1])
