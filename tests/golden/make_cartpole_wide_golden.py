"""TEST INFRASTRUCTURE ONLY -- writes tests/golden/cartpole_wide.npz: one-step Cartpole transitions from pole angles beyond
pi / 4, where the bounded-sin/cos variants of csrc/cartpole.hip leave their polynomials for the library's sincosf under
one branch per thread.  A live pole stays within 12 degrees, so only a caller who writes STATE gets there.

    python tests/golden/make_cartpole_wide_golden.py [reference checkout]

next64 is the reference's float64 CartpoleNumpy (envs/cartpole_env.py:130-233), fed Python floats as
make_cartpole_golden.py feeds it; next and done are the CPU oracle's (oracle/cartpole_oracle.c), which
tests/test_ref_cartpole.py pins bit for bit to the reference's compiled sim.cpp.  Two sets of 512, signs of theta random:

    survive  |theta| uniform in [0.8, 3], x in +-1.5, x_dot ~ N(0, 1.5), theta_dot = (target - theta) / 0.02 with the target
             uniform in +-0.15: the world lives, and its new rates -- which took sin / cos from the library -- stay visible
             in every form of the step.  survive_tol (4,) = 4 x the oracle's largest distance from next64 (the Acrobot
             fixture's convention: tests/golden/make_acrobot_golden.py).
    finish   |theta| log-uniform in [0.8, 1e4], x in +-1.5, x_dot ~ N(0, 1.5) and theta_dot ~ N(0, 2) both clipped to +-4:
             every world finishes.  Only next64: the reference overwrites a finished world, so there is no float32
             reference of its post-transition state.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "cartpole_wide.npz")
SET = 512
X_TH, TH_TH = 2.4, 12 * 2 * np.pi / 360


def default_reference_dir():
    return os.path.abspath(os.environ.get("MRL_REFERENCE_DIR") or os.path.join(REPO, "..", "reference"))


def reference_env(reference_dir=None):
    return os.path.join(reference_dir or default_reference_dir(), "envs", "cartpole_env.py")


def reference_class(reference_dir=None):
    """the reference's CartpoleNumpy, imported with the missing packages stubbed (_ref_stubs.py); sys.path and the stub
    modules are put back, so a test session that regenerates the fixture goes on as it was"""
    reference_dir = reference_dir or default_reference_dir()
    before, path = set(sys.modules), list(sys.path)
    try:
        sys.path[:0] = [reference_dir, HERE]
        import _ref_stubs
        _ref_stubs.install()
        from envs.cartpole_env import CartpoleNumpy
        return CartpoleNumpy
    finally:
        for name in set(sys.modules) - before:
            if name.split(".")[0] in ("envs", "gym", "build", "overcooked_ai_py", "hanabi_learning_environment", "tensorboard",
                                      "_ref_stubs") or name == "torch.utils.tensorboard":
                del sys.modules[name]
        sys.path[:] = path


def draw():
    """the float32 start states and the actions of both sets"""
    rng = np.random.default_rng(20250302)
    out = {}
    for name in ("survive", "finish"):
        s = np.empty((SET, 4), np.float64)
        sign = rng.choice([-1.0, 1.0], SET)
        s[:, 0] = rng.uniform(-1.5, 1.5, SET)
        s[:, 1] = rng.normal(0, 1.5, SET)
        if name == "survive":
            s[:, 2] = sign * rng.uniform(0.8, 3.0, SET)
            s[:, 3] = (rng.uniform(-0.15, 0.15, SET) - s[:, 2]) / 0.02
        else:
            s[:, 1] = np.clip(s[:, 1], -4, 4)
            s[:, 2] = sign * np.exp(rng.uniform(np.log(0.8), np.log(1e4), SET))
            s[:, 3] = np.clip(rng.normal(0, 2.0, SET), -4, 4)
        out[name + "_state"] = s.astype(np.float32)
        out[name + "_action"] = rng.integers(0, 2, SET).astype(np.int32)
    return out


def reference_step(cls, states, actions):
    env = cls()
    nxt64, done = np.empty((len(states), 4), np.float64), np.empty(len(states), np.int32)
    for i in range(len(states)):
        env.steps_beyond_done = None
        env.state = tuple(float(v) for v in states[i])
        _, _, d, _ = env.step(int(actions[i]))
        nxt64[i], done[i] = env.state, int(d)
    return nxt64, done


def oracle_step(states, actions):
    if REPO not in sys.path:
        sys.path.insert(0, REPO)
    from oracle import oracle
    oracle.build()
    orc = oracle.CartpoleOracle(len(states))
    orc.state[:] = states
    orc.step(actions)
    out = orc.state.copy(), orc.done[:, 0].copy()
    orc.close()
    return out


def generate(reference_dir=None):
    out = draw()
    cls = reference_class(reference_dir)
    for name in ("survive", "finish"):
        states, actions = out[name + "_state"], out[name + "_action"]
        nxt64, done64 = reference_step(cls, states, actions)
        nxt, done = oracle_step(states, actions)
        out[name + "_next64"], out[name + "_done"] = nxt64, done
        if name == "survive":
            assert not done64.any() and not done.any(), "survive: a world finishes"
            out["survive_next"] = nxt
            out["survive_tol"] = 4.0 * np.abs(nxt.astype(np.float64) - nxt64).max(axis=0)
        else:
            assert done64.all() and done.all(), "finish: a world lives"
    return out


def main():
    out = generate(sys.argv[1] if len(sys.argv) > 1 else None)
    np.savez_compressed(OUT, **out)
    print("survive: tol", out["survive_tol"], "largest |theta_dot|", np.abs(out["survive_state"][:, 3]).max())
    print("finish: largest |theta|", np.abs(out["finish_state"][:, 2]).max(), "->", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
