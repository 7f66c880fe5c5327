"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/acrobot_ref.npz and acrobot_far_ref.npz: what the reference's own Acrobot
sim.cpp computes, as data.  The reference file is compiled unchanged (tests/golden/acrobot_ref_driver.cpp includes it; the Madrona
stand-in is oracle/madrona_standin with tests/golden/acrobot_standin in front for <madrona/math.hpp>) into a
temporary directory; nothing of it is kept.

    python tests/golden/make_acrobot_golden.py [reference checkout]

The reference is driven with at most 500 worlds per call, and the ONE episode length all its worlds share is set to 0
before every teacher-forced step, so its truncation never fires.  Arrays:

    fresh (8192, 4)        the start states of episodes 0 .. 8191;  fresh_last (8, 4): of episodes 2^32 - 8 .. 2^32 - 1
                           (twice the 4096 first planned: the truncation test at 2049 worlds runs three episodes per world and
                           compares start states up to episode 6146)
    quiet_episodes         episodes 0 .. quiet_episodes - 1 never terminate within 501 steps of zero torque
    reach_*  2048 one-step transitions (state, action -> next, done) sampled from reference play under a uniform random policy
    swing_*  2048 with theta uniform in [-pi, pi], |omega1| <= 3, |omega2| <= 6
    clamp_*  64 from velocities near the bounds: *_mask says which velocity components the reference clamped
    *_next64 the float64 twin's result (tests/acrobot_twin.py);  *_tol (4,) = 4 x the reference's largest distance from it

Dropped before the sets are cut to size: every transition whose twin height -cos t1 - cos(t1 + t2) lies within 1e-3 of 1
(the clamp set: within 0.2, and the twin must agree on the flag and overshoot the bound by 0.5).  *_dropped counts them.

acrobot_far_ref.npz (generate_far): four sets of 512 one-step transitions from angles FAR outside [-pi, pi], which a caller
may write into STATE and which take the step kernel's out-of-range paths (csrc/acrobot.hip: wrap_fast's second select,
the per-world fallback to step_plain, wrap_plain's bounded loops and its one-piece wrap).  Velocities and actions as in
`swing`; by draw index mod 3 theta1, theta2 or both are far, sign random, the other angle uniform in [-pi, pi]:

    turns2  far |theta| in [10.5, 12]          the new angle is two turns off: within what the fast path wraps
    turns3  far |theta| in [5 pi + 1, 120]     stage angles within the fast range, the new angle 3 .. 20 turns off
    beyond  far |theta| in [130, 395]          stage angles beyond the fast range, at most 64 turns off
    piece   far |theta| in [420, 2000]         more than 64 turns off: the reference loops on, the kernel wraps in one piece

Same arrays per set as above (state, action, next, done, next64, tol, dropped), the band 1e-3 (piece: 1e-2: the reference is
3.7e-3 from its twin there).  A draw must also lie ON its set's path by the float64 twin with a margin (on_path below:
tests/test_ref_acrobot.py asserts the same of the stored inputs); *_offpath counts the draws that did not, e.g. a far
angle of 10.5 whose velocity of -6 takes it below 3 pi.
"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
import acrobot_twin as twin  # noqa: E402

OUT = os.path.join(HERE, "acrobot_ref.npz")
OUT_FAR = os.path.join(HERE, "acrobot_far_ref.npz")
FLAGS = ["-O2", "-fPIC", "-ffp-contract=off", "-std=c++17"]
BATCH = 500
FRESH, SET, CLAMP = 8192, 2048, 64
BAND = 1e-3
FAR_SET = 512
FAR = (("turns2", 10.5, 12.0, 1e-3), ("turns3", 5 * np.pi + 1, 120.0, 1e-3), ("beyond", 130.0, 395.0, 1e-3), ("piece", 420.0, 2000.0, 1e-2))
FAST_RANGE = 128.0                                  # csrc/acrobot.hip: kFastRange
LOOP_END = twin.PI_F + 64 * 2 * twin.PI_F           # the largest value wrap_plain's 64 trips bring back into [-pi, pi]


def default_reference_dir():
    return os.environ.get("MRL_REFERENCE_DIR") or os.path.join(REPO, "..", "reference")


def reference_sim(reference_dir=None):
    return os.path.join(os.path.abspath(reference_dir or default_reference_dir()), "src", "acrobat_env", "sim.cpp")


def build_driver(out_dir, reference_dir=None):
    """g++ the driver around the reference's sim.cpp -> out_dir/libref_acrobot.so"""
    lib = os.path.join(out_dir, "libref_acrobot.so")
    cmd = (["g++"] + FLAGS + ["-shared", "-I", os.path.join(HERE, "acrobot_standin"), "-I", os.path.join(REPO, "oracle"),
                             "-I", os.path.join(REPO, "oracle", "madrona_standin"),
                             '-DREF_SIM="%s"' % reference_sim(reference_dir), "-o", lib,
                             os.path.join(HERE, "acrobot_ref_driver.cpp")])
    proc = subprocess.run(cmd, capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("compiling the Acrobot reference driver failed:\n" + proc.stderr[-4000:])
    return lib


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


class RefAcrobot:
    def __init__(self, lib_path, n, first_episode=0):
        L = self.L = ctypes.CDLL(lib_path)
        vp, u32 = ctypes.c_void_p, ctypes.c_uint32
        f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
        L.ref_acrobot_create.restype = vp
        L.ref_acrobot_create.argtypes = [u32, u32]
        L.ref_acrobot_destroy.argtypes = [vp]
        L.ref_acrobot_step.argtypes = [vp, i32p]
        L.ref_acrobot_read.argtypes = [vp, f32p, f32p, i32p]
        L.ref_acrobot_set_state.argtypes = [vp, f32p]
        L.ref_acrobot_set_length.argtypes = [vp, u32]
        L.ref_acrobot_length.restype = u32
        L.ref_acrobot_length.argtypes = [vp]
        L.ref_acrobot_episodes.restype = u32
        L.ref_acrobot_episodes.argtypes = [vp]
        self.n = n
        self.h = L.ref_acrobot_create(n, first_episode & 0xFFFFFFFF)
        self.state = np.zeros((n, 4), np.float32)
        self.reward = np.zeros(n, np.float32)
        self.done = np.zeros(n, np.int32)
        self._read()

    def _read(self):
        self.L.ref_acrobot_read(self.h, _p(self.state, ctypes.c_float), _p(self.reward, ctypes.c_float), _p(self.done, ctypes.c_int32))

    def step(self, actions):
        a = np.ascontiguousarray(actions, dtype=np.int32)
        self.L.ref_acrobot_step(self.h, _p(a, ctypes.c_int32))
        self._read()

    def set_state(self, state):
        s = np.ascontiguousarray(state, dtype=np.float32)
        self.L.ref_acrobot_set_state(self.h, _p(s, ctypes.c_float))
        self._read()

    def set_length(self, length):
        self.L.ref_acrobot_set_length(self.h, int(length))

    @property
    def length(self):
        return int(self.L.ref_acrobot_length(self.h))

    @property
    def episodes(self):
        return int(self.L.ref_acrobot_episodes(self.h))

    def close(self):
        if self.h:
            self.L.ref_acrobot_destroy(self.h)
            self.h = None


def one_step(lib, states, actions):
    """teacher-forced: the reference's next state and done flag for every (state, action), BATCH worlds per call"""
    nxt = np.zeros((len(states), 4), np.float32)
    done = np.zeros(len(states), np.int32)
    for lo in range(0, len(states), BATCH):
        s, a = states[lo:lo + BATCH], actions[lo:lo + BATCH]
        ref = RefAcrobot(lib, len(s))
        ref.set_state(s)
        ref.set_length(0)
        ref.step(a)
        nxt[lo:lo + BATCH], done[lo:lo + BATCH] = ref.state, ref.done  # (a finished world already holds a fresh state)
        ref.close()
    return nxt, done


def fresh_states(lib, first, count):
    out = np.zeros((count, 4), np.float32)
    for lo in range(0, count, BATCH):
        n = min(BATCH, count - lo)
        ref = RefAcrobot(lib, n, first + lo)
        out[lo:lo + n] = ref.state
        ref.close()
    return out


def quiet_episodes(lib, count):
    """how many of episodes 0 .. count - 1, from the front, get through 501 steps of zero torque without terminating"""
    for lo in range(0, count, BATCH):
        n = min(BATCH, count - lo)
        ref = RefAcrobot(lib, n, lo)
        zero = np.ones(n, np.int32)
        for _ in range(twin.MAX_STEPS + 1):
            ref.set_length(0)
            ref.step(zero)
            if ref.done.any():
                ref.close()
                return lo + int(np.argmax(ref.done != 0))
        ref.close()
    return count


def finish_set(name, states, actions, nxt, done, out):
    """drop the transitions at the threshold, cut to SET, add the twin's results and the tolerance"""
    n64, height, _ = twin.step(states, actions)
    keep = np.abs(height - 1.0) > BAND
    assert ((height > 1.0) == (done != 0))[keep].all(), name + ": the reference and its twin disagree on a done flag off the threshold"
    idx = np.flatnonzero(keep)[:SET]
    assert len(idx) == SET, name + ": too few transitions left"
    dropped = int((~keep[:idx[-1] + 1]).sum())
    states, actions, nxt, done, n64 = states[idx], actions[idx], nxt[idx], done[idx], n64[idx]
    live = done == 0
    err = twin.distance(nxt[live], n64[live]).max(axis=0)
    out[name + "_state"], out[name + "_action"], out[name + "_next"], out[name + "_done"] = states, actions, nxt, done
    out[name + "_next64"], out[name + "_tol"], out[name + "_dropped"] = n64, 4.0 * err, np.int64(dropped)


def on_path(name, states, actions):
    """which transitions take the path their set is named after, by the twin and with a margin: |new far angle| before the
    wrap and the largest |stage angle| (the kernel's `reach`)"""
    _, _, _, raw, reach = twin.step(states, actions, detail=True)
    far = np.abs(np.asarray(states, np.float64)[:, :2]) > twin.PI_F
    new = np.abs(raw)
    lowest, highest = np.where(far, new, np.inf).min(axis=1), np.where(far, new, 0.0).max(axis=1)
    if name == "turns2":
        return (lowest > 3 * twin.PI_F + 0.05) & (highest < 5 * twin.PI_F - 0.05) & (reach < FAST_RANGE - 1)
    if name == "turns3":
        return (lowest > 5 * twin.PI_F + 0.05) & (reach < FAST_RANGE - 1)
    if name == "beyond":
        return (reach > FAST_RANGE + 1) & (highest < LOOP_END - 1)
    return lowest > LOOP_END + 1


def finish_far_set(name, count, band, states, actions, nxt, done, out):
    """finish_set for a far set: drop what lies at the threshold (within `band`) or off the set's path, cut to `count`"""
    n64, height, _ = twin.step(states, actions)
    off_band, path = np.abs(height - 1.0) > band, on_path(name, states, actions)
    assert ((height > 1.0) == (done != 0))[off_band].all(), name + ": the reference and its twin disagree on a done flag off the threshold"
    idx = np.flatnonzero(off_band & path)[:count]
    assert len(idx) == count, name + ": too few transitions left"
    used = slice(0, idx[-1] + 1)
    dropped, offpath = int((~off_band[used]).sum()), int((off_band & ~path)[used].sum())
    states, actions, nxt, done, n64 = states[idx], actions[idx], nxt[idx], done[idx], n64[idx]
    live = done == 0
    err = twin.distance(nxt[live], n64[live]).max(axis=0)
    out[name + "_state"], out[name + "_action"], out[name + "_next"], out[name + "_done"] = states, actions, nxt, done
    out[name + "_next64"], out[name + "_tol"] = n64, 4.0 * err
    out[name + "_dropped"], out[name + "_offpath"] = np.int64(dropped), np.int64(offpath)


def generate_far(lib):
    out = {}
    for k, (name, lo, hi, band) in enumerate(FAR):
        rng = np.random.default_rng(20250301 + k)
        n = FAR_SET + 128
        states = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-3, 3, n),
                           rng.uniform(-6, 6, n)], axis=1)
        far = rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(lo, hi, (n, 2))
        pattern = np.arange(n) % 3  # theta1 only, theta2 only, both
        states[:, 0] = np.where(pattern != 1, far[:, 0], states[:, 0])
        states[:, 1] = np.where(pattern != 0, far[:, 1], states[:, 1])
        states = states.astype(np.float32)
        actions = rng.integers(0, 3, n).astype(np.int32)
        nxt, done = one_step(lib, states, actions)
        finish_far_set(name, FAR_SET, band, states, actions, nxt, done, out)
    return out


def generate(lib):
    out = {}
    out["fresh"] = fresh_states(lib, 0, FRESH)
    out["fresh_last"] = fresh_states(lib, 2 ** 32 - 8, 8)
    out["quiet_episodes"] = np.int64(quiet_episodes(lib, FRESH))

    # reachable states: reference play under a uniform random policy, every (state, action, next, done) recorded
    rng = np.random.default_rng(20240917)
    ref = RefAcrobot(lib, BATCH)
    steps = 400
    S = np.zeros((steps, BATCH, 4), np.float32)
    A = np.zeros((steps, BATCH), np.int32)
    N = np.zeros((steps, BATCH, 4), np.float32)
    D = np.zeros((steps, BATCH), np.int32)
    for t in range(steps):
        S[t] = ref.state
        A[t] = rng.integers(0, 3, BATCH)
        ref.set_length(0)
        ref.step(A[t])
        N[t], D[t] = ref.state, ref.done
    ref.close()
    pick = rng.permutation(steps * BATCH)[:SET + 64]
    finish_set("reach", S.reshape(-1, 4)[pick], A.reshape(-1)[pick], N.reshape(-1, 4)[pick], D.reshape(-1)[pick], out)

    rng = np.random.default_rng(20240918)
    n = SET + 64
    states = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(-3, 3, n),
                       rng.uniform(-6, 6, n)], axis=1).astype(np.float32)
    actions = rng.integers(0, 3, n).astype(np.int32)
    nxt, done = one_step(lib, states, actions)
    finish_set("swing", states, actions, nxt, done, out)

    # velocities near the bounds; kept where the reference clamped a component and the twin overshoots that bound clearly
    rng = np.random.default_rng(20240919)
    n = 2048
    sign = rng.choice([-1.0, 1.0], (n, 2))
    states = np.stack([rng.uniform(-np.pi, np.pi, n), rng.uniform(-np.pi, np.pi, n),
                       sign[:, 0] * rng.uniform(0.9, 1.0, n) * twin.MAX_VEL_1,
                       sign[:, 1] * rng.uniform(0.9, 1.0, n) * twin.MAX_VEL_2], axis=1).astype(np.float32)
    actions = rng.integers(0, 3, n).astype(np.int32)
    nxt, done = one_step(lib, states, actions)
    _, height, raw = twin.step(states, actions)
    bound = np.array([twin.MAX_VEL_1, twin.MAX_VEL_2], np.float32)
    clamped = np.abs(nxt[:, 2:]) == bound
    sure = (np.abs(raw) > bound + 0.5) | (np.abs(raw) < bound - 0.5)     # the twin is clearly on one side for both components
    keep = (done == 0) & clamped.any(axis=1) & sure.all(axis=1) & (clamped == (np.abs(raw) > bound)).all(axis=1) & \
        (np.abs(height - 1.0) > 0.2) & (height <= 1.0)
    live = np.flatnonzero(keep)[:CLAMP - 16]
    # and some that finish: the done flag of a clamped state
    keep_done = (done != 0) & (np.abs(height - 1.0) > 0.2) & (height > 1.0)
    over = np.flatnonzero(keep_done)[:16]
    idx = np.sort(np.concatenate([live, over]))
    assert len(idx) == CLAMP, "clamp: too few transitions left"
    out["clamp_state"], out["clamp_action"], out["clamp_next"], out["clamp_done"] = states[idx], actions[idx], nxt[idx], done[idx]
    out["clamp_mask"] = (clamped[idx] & (done[idx] == 0)[:, None])
    return out


def main():
    reference_dir = sys.argv[1] if len(sys.argv) > 1 else None
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_driver(tmp, reference_dir)
        out, far = generate(lib), generate_far(lib)
    np.savez_compressed(OUT, **out)
    np.savez_compressed(OUT_FAR, **far)
    for name, _, _, _ in FAR:
        print(name, "tol", far[name + "_tol"], "dropped", int(far[name + "_dropped"]), "off path", int(far[name + "_offpath"]),
              "done", int(far[name + "_done"].sum()))
    print("->", OUT_FAR, os.path.getsize(OUT_FAR), "bytes")
    for name in ("reach", "swing"):
        print(name, "tol", out[name + "_tol"], "dropped", int(out[name + "_dropped"]), "done", int(out[name + "_done"].sum()))
    print("clamp: done", int(out["clamp_done"].sum()), "clamped components", int(out["clamp_mask"].sum()))
    print("quiet episodes", int(out["quiet_episodes"]), "->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
