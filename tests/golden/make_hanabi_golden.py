"""Checks this repo's CPU Hanabi oracle with the REFERENCE's own invariant
checker (envs/hanabi_env.py:157-657, HanabiState + validate_step), imported from
/root/reference in the build container (stubs for gym / HLE / build.*, see
_ref_stubs.py), and writes tests/golden/hanabi_<cfg>.npz: the action streams
plus the observation / state / mask / active / reward / done sequences that
passed that checker.

What the reference checker pins: one active agent that alternates, state prefix
== obs, hands / deck / fireworks / tokens / discards decode consistently with
card conservation, legal-move mask, one-step token/firework/discard/reward/done
simulation, pristine start state after done.  It does NOT look at the
card-knowledge and last-action sections, the RNG draws or the episode->seed map
(envs/hanabi_env.py:296,640-641): those are pinned by the compiled reference
instead (tests/test_ref_hanabi.py, tests/golden/make_ref_golden.py).

Two cases the checker rejects by construction; such steps are counted and
reported, not treated as oracle errors:
* information tokens above the maximum (a rank-5 card played at full tokens; the
  reference simulator adds the token unconditionally, src/hanabi_env/sim.cpp:676-678,
  and its encoders then shift);
* a hand shorter than five cards (deck exhausted): the checker decodes empty
  slots as card 0 and so expects "partner holds colour 0 / rank 0" in the hint
  mask (envs/hanabi_env.py:167,409-431, and it walks `colors` entries for the rank
  hints), whereas the simulator scans the real slots (sim.cpp:410-436).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()
import envs.hanabi_env as ref  # noqa: E402  (reference)

from madrona_rl_envs_playground_amd import hanabi_spec  # noqa: E402
from oracle.oracle import HanabiOracle  # noqa: E402

CONFIGS = {"full": (ref.FULL_CONFIG, 48, 260), "small": (ref.SMALL_CONFIG, 48, 200),
           "very_small": (ref.VERY_SMALL_CONFIG, 32, 60)}


class Obs:
    def __init__(self, active, obs, state, mask):
        self.active, self.obs, self.state, self.action_mask = active, obs, state, mask


def snapshot(orc, cfg):
    no, ns, nm = hanabi_spec.observation_size(cfg), hanabi_spec.state_size(cfg), hanabi_spec.num_moves(cfg)
    return [Obs(torch.from_numpy(orc.active[i].astype(bool)), torch.from_numpy(orc.obs[i, :, :no].astype(np.int8)),
                torch.from_numpy(orc.state[i, :, :ns].astype(np.int8)),
                torch.from_numpy(orc.mask[i, :, :nm].astype(bool))) for i in range(2)]


def main():
    for name, (cfg, n, steps) in CONFIGS.items():
        orc = HanabiOracle(cfg, n)
        rng = np.random.default_rng(7)
        rec = {k: [] for k in ("actions", "obs", "state", "mask", "active", "reward", "done")}
        first = {k: getattr(orc, k).copy() for k in ("obs", "state", "mask", "active")}
        checked = rejected_overflow = rejected_short = 0
        for t in range(steps):
            before = snapshot(orc, cfg)
            dump_before = orc.dump()
            info_before = dump_before[:, 81].copy()
            short_before = (dump_before[:, 105] < 5) | (dump_before[:, 141] < 5)
            a = (rng.random(orc.mask.shape) * (orc.mask != 0)).argmax(-1).astype(np.int32)
            orc.step(a)
            after = snapshot(orc, cfg)
            dump_after = orc.dump()
            info_after = dump_after[:, 81]
            short_after = (dump_after[:, 105] < 5) | (dump_after[:, 141] < 5)
            for w in range(n):
                sl = slice(w, w + 1)
                one = lambda obs: [Obs(o.active[sl], o.obs[sl], o.state[sl], o.action_mask[sl]) for o in obs]
                ok = ref.validate_step(one(before), torch.from_numpy(a[:, sl]), torch.from_numpy(orc.done[sl]),
                                       one(after), torch.from_numpy(orc.reward[:, sl]), cfg, verbose=False)
                over = info_before[w] > cfg["max_information_tokens"] or (
                    not orc.done[w] and info_after[w] > cfg["max_information_tokens"])
                if not ok and over:
                    rejected_overflow += 1
                elif not ok and (short_before[w] or (not orc.done[w] and short_after[w])):
                    rejected_short += 1
                elif not ok:
                    ref.validate_step(one(before), torch.from_numpy(a[:, sl]), torch.from_numpy(orc.done[sl]),
                                      one(after), torch.from_numpy(orc.reward[:, sl]), cfg, verbose=True)
                    raise SystemExit(f"{name}: reference checker rejected world {w} at step {t}")
                else:
                    checked += 1
            rec["actions"].append(a.astype(np.int8))
            for k in ("obs", "state", "mask", "active", "reward", "done"):
                rec[k].append(getattr(orc, k).copy())
        out = os.path.join(HERE, f"hanabi_{name}.npz")
        # the 0/1 observation and state rows go in bit-packed (tests/conftest.py:load_golden unpacks them): the full
        # configuration's fixture stays well under 1 MiB
        bits = {"obs": np.stack(rec["obs"]), "state": np.stack(rec["state"]), "first_obs": first["obs"],
                "first_state": first["state"]}
        packed = {}
        for k, v in bits.items():
            packed[k + "_bits"], packed[k + "_len"] = np.packbits(v, axis=-1), np.int64(v.shape[-1])
        np.savez_compressed(out, actions=np.stack(rec["actions"]), mask=np.stack(rec["mask"]).astype(np.int8),
                            active=np.stack(rec["active"]).astype(np.int8), reward=np.stack(rec["reward"]),
                            done=np.stack(rec["done"]).astype(np.int8), first_mask=first["mask"].astype(np.int8),
                            first_active=first["active"].astype(np.int8), **packed)
        print(f"{name}: {checked} world-steps accepted by the reference checker "
              f"({rejected_overflow} rejected only with information tokens above the maximum, "
              f"{rejected_short} only with a short hand), "
              f"episodes finished {int(np.stack(rec['done']).sum())}, {os.path.getsize(out) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
