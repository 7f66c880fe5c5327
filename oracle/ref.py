"""TEST INFRASTRUCTURE ONLY -- ctypes front end of oracle/_ref/libref_{hanabi,cartpole,balance}.so: the
reference's own Hanabi, Cartpole and balance-beam sim.cpp, compiled unchanged against the Madrona stand-in
(oracle/madrona_standin, oracle/ref_driver_*.cpp, oracle/Makefile.ref).  The classes mirror the oracle's
(oracle/oracle.py) but copy their outputs out on every read.

``build(reference_dir)`` runs the recipe; ``require()`` is what a test calls first: it skips (with the
reason) when oracle/_ref/BUILD_INFO is missing, i.e. the reference tree was never there to build from, and
fails when BUILD_INFO exists but a library is missing or does not load.
"""
import ctypes
import os
import subprocess

import numpy as np

from oracle.oracle import HANABI_MOVES, HANABI_OBS, HANABI_STATE, HanabiConfig

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
BUILD_INFO = os.path.join(REF_DIR, "BUILD_INFO")
GAMES = ("hanabi", "cartpole", "balance")
FILLS = (0x00, 0xA5)
# guard-hit rows (world, entity, type code, offset, value); Hanabi type codes as ref_hanabi_guards numbers them
GUARD_OBSERVATION, GUARD_STATE = 0, 1
_libs = {}


def default_reference_dir():
    """MRL_REFERENCE_DIR, else a reference checkout next to this repository."""
    return os.environ.get("MRL_REFERENCE_DIR") or os.path.join(os.path.dirname(_HERE), "..", "reference")


def reference_present(reference_dir=None):
    d = reference_dir or default_reference_dir()
    return all(os.path.isfile(os.path.join(d, "src", sub, "sim.cpp"))
               for sub in ("hanabi_env", "cartpole_env", "balance_beam_env"))


def build(reference_dir=None):
    """Compile the three reference libraries and BUILD_INFO with oracle/Makefile.ref (g++)."""
    d = os.path.abspath(reference_dir or default_reference_dir())
    proc = subprocess.run(["make", "-C", _HERE, "-f", "Makefile.ref", "REF=" + d], capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("oracle/Makefile.ref failed:\n" + proc.stdout[-4000:] + proc.stderr[-4000:])
    return REF_DIR


def require():
    """Skip when _ref was never built (no BUILD_INFO); otherwise load all three libraries or fail."""
    if not os.path.isfile(BUILD_INFO):
        import pytest
        pytest.skip("oracle/_ref not built (no oracle/_ref/BUILD_INFO): build() found no reference tree to compile")
    for g in GAMES:
        lib(g)


def lib(game):
    if game in _libs:
        return _libs[game]
    path = os.path.join(REF_DIR, "libref_%s.so" % game)
    L = ctypes.CDLL(path)  # OSError when missing or broken: a failure, not a skip
    vp, u32, i32p = ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int32)
    u8p, f32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_float)
    pre = "ref_%s_" % game
    create = getattr(L, pre + "create")
    create.restype = vp
    if game == "hanabi":
        create.argtypes = [ctypes.POINTER(HanabiConfig), u32, u32, u32, ctypes.c_int]
        getattr(L, pre + "read").argtypes = [vp, u8p, u8p, i32p, i32p, f32p, i32p]
    elif game == "cartpole":
        create.argtypes = [u32, u32, u32, ctypes.c_int]
        getattr(L, pre + "read").argtypes = [vp, f32p, f32p, i32p]
        L.ref_cartpole_set_state.argtypes = [vp, f32p]
    else:
        create.argtypes = [u32, u32, u32, ctypes.c_int]
        getattr(L, pre + "read").argtypes = [vp, i32p, i32p, i32p, f32p, i32p]
    getattr(L, pre + "destroy").argtypes = [vp]
    getattr(L, pre + "step").argtypes = [vp, i32p]
    getattr(L, pre + "episodes").restype = u32
    getattr(L, pre + "episodes").argtypes = [vp]
    getattr(L, pre + "guards").restype = u32
    getattr(L, pre + "guards").argtypes = [vp, i32p, u32]
    _libs[game] = L
    return L


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


class _Ref:
    game = None

    def _fin(self, h):
        if not h:
            raise ValueError("reference driver rejected the configuration")
        self.h = h

    def step(self, actions):
        a = np.ascontiguousarray(np.asarray(actions).reshape(self._act_shape), dtype=np.int32)
        getattr(self.L, "ref_%s_step" % self.game)(self.h, _p(a, ctypes.c_int32))
        self._read()

    @property
    def episodes(self):
        return int(getattr(self.L, "ref_%s_episodes" % self.game)(self.h))

    def guards(self):
        """Guard bytes written since the last call, as an (hits, 5) int32 array of (world, entity, type code,
        offset past the payload end (negative: before its start), value); the guards are restored."""
        fn = getattr(self.L, "ref_%s_guards" % self.game)
        cap = 4 * self.N + 64
        out = np.zeros((cap, 5), np.int32)
        n = int(fn(self.h, _p(out, ctypes.c_int32), cap))
        if n > cap:
            raise AssertionError("%d guard bytes written in one step" % n)
        return out[:n]

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, "ref_%s_destroy" % self.game)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefHanabi(_Ref):
    game = "hanabi"

    def __init__(self, config, num_worlds, first_episode=0, fill=0x00, construct=False):
        self.L = lib(self.game)
        self.N = N = int(num_worlds)
        self._act_shape = (2, N)
        cfg = HanabiConfig(int(config["colors"]), int(config["ranks"]), int(config["players"]),
                           int(config["max_information_tokens"]), int(config["max_life_tokens"]))
        self.obs = np.zeros((2, N, HANABI_OBS), np.uint8)
        self.state = np.zeros((2, N, HANABI_STATE), np.uint8)
        self.mask = np.zeros((2, N, HANABI_MOVES), np.int32)
        self.active = np.zeros((2, N), np.int32)
        self.reward = np.zeros((2, N), np.float32)
        self.done = np.zeros((N,), np.int32)
        self._fin(self.L.ref_hanabi_create(ctypes.byref(cfg), N, int(first_episode) & 0xFFFFFFFF, fill, int(construct)))
        self._read()

    def _read(self):
        self.L.ref_hanabi_read(self.h, _p(self.obs, ctypes.c_uint8), _p(self.state, ctypes.c_uint8),
                               _p(self.mask, ctypes.c_int32), _p(self.active, ctypes.c_int32),
                               _p(self.reward, ctypes.c_float), _p(self.done, ctypes.c_int32))


class RefCartpole(_Ref):
    game = "cartpole"

    def __init__(self, num_worlds, first_episode=0, fill=0x00, construct=False):
        self.L = lib(self.game)
        self.N = N = int(num_worlds)
        self._act_shape = (N,)
        self.state = np.zeros((N, 4), np.float32)
        self.reward = np.zeros((N, 1), np.float32)
        self.done = np.zeros((N, 1), np.int32)
        self._fin(self.L.ref_cartpole_create(N, int(first_episode) & 0xFFFFFFFF, fill, int(construct)))
        self._read()

    def set_state(self, state):
        st = np.ascontiguousarray(state, dtype=np.float32).reshape(self.N, 4)
        self.L.ref_cartpole_set_state(self.h, _p(st, ctypes.c_float))
        self._read()

    def _read(self):
        self.L.ref_cartpole_read(self.h, _p(self.state, ctypes.c_float), _p(self.reward, ctypes.c_float),
                                 _p(self.done, ctypes.c_int32))


class RefBalance(_Ref):
    game = "balance"

    def __init__(self, num_worlds, first_episode=0, fill=0x00, construct=False):
        self.L = lib(self.game)
        self.N = N = int(num_worlds)
        self._act_shape = (2, N)
        self.obs = np.zeros((2, N, 7), np.int32)
        self.loc = np.zeros((2, N), np.int32)
        self.time = np.zeros((N,), np.int32)
        self.reward = np.zeros((2, N), np.float32)
        self.done = np.zeros((N,), np.int32)
        self._fin(self.L.ref_balance_create(N, int(first_episode) & 0xFFFFFFFF, fill, int(construct)))
        self._read()

    def _read(self):
        self.L.ref_balance_read(self.h, _p(self.obs, ctypes.c_int32), _p(self.loc, ctypes.c_int32),
                                _p(self.time, ctypes.c_int32), _p(self.reward, ctypes.c_float),
                                _p(self.done, ctypes.c_int32))
