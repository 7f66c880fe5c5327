"""TEST INFRASTRUCTURE ONLY -- ctypes front end of oracle/_ref/libref_{hanabi,cartpole,balance,overcooked,
simplecooked}.so: the reference's own sim.cpp of five games (Hanabi, Cartpole, the balance beam, Overcooked and
Simplecooked), compiled unchanged against the Madrona stand-in (oracle/madrona_standin, oracle/ref_driver_*.cpp,
oracle/Makefile.ref).  The classes mirror the oracle's (oracle/oracle.py) but copy their outputs out on every read.

The kitchens take two more options, for what Madrona leaves open: ``graph_order`` (0: the task graph's nodes in
insertion order, 1: a second topological order) and ``reverse_entities`` (a node visits its entities in descending
creation order); see madrona_standin/madrona/taskgraph_builder.hpp.  A configuration the C++ cannot hold raises
ValueError: Overcooked above 255 cells or 64 players, Simplecooked above 100 cells or with any player count but two
(with one player its dish-pickup shaping reads a second agent that was never created), Hanabi outside the HIP library's
ranges or with fewer than ten cards (oracle.check_hanabi_config: decided in Python, the C++ is never entered).

``build(reference_dir)`` runs the recipe; ``require()`` is what a test calls first: it skips (with the
reason) when oracle/_ref/BUILD_INFO is missing, i.e. the reference tree was never there to build from, and
fails when BUILD_INFO exists but a library is missing or does not load.
"""
import ctypes
import os
import subprocess

import numpy as np

from oracle.oracle import HANABI_MOVES, HANABI_OBS, HANABI_STATE, HanabiConfig, check_hanabi_config

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
BUILD_INFO = os.path.join(REF_DIR, "BUILD_INFO")
GAMES = ("hanabi", "cartpole", "balance", "overcooked", "simplecooked")
SOURCE_DIRS = ("hanabi_env", "cartpole_env", "balance_beam_env", "overcooked_env", "overcooked2_env")
FILLS = (0x00, 0xA5)
# guard-hit rows (world, entity, type code, offset, value); Hanabi type codes as ref_hanabi_guards numbers them
GUARD_OBSERVATION, GUARD_STATE = 0, 1
# ... and the kitchens' (ref_driver_kitchen.hpp)
GUARD_LOCATION_OBSERVATION, GUARD_LOCATION_DATA, GUARD_PLAYER_STATE, GUARD_WORLD_STATE = 0, 1, 2, 3
NUM_RECIPES = 16
_libs = {}


def default_reference_dir():
    """MRL_REFERENCE_DIR, else a reference checkout next to this repository."""
    return os.environ.get("MRL_REFERENCE_DIR") or os.path.join(os.path.dirname(_HERE), "..", "reference")


def reference_present(reference_dir=None):
    d = reference_dir or default_reference_dir()
    return all(os.path.isfile(os.path.join(d, "src", sub, "sim.cpp"))
               for sub in SOURCE_DIRS)


def build(reference_dir=None):
    """Compile the five reference libraries and BUILD_INFO with oracle/Makefile.ref (g++)."""
    d = os.path.abspath(reference_dir or default_reference_dir())
    proc = subprocess.run(["make", "-C", _HERE, "-f", "Makefile.ref", "REF=" + d], capture_output=True, text=True)
    if proc.returncode != 0:
        raise RuntimeError("oracle/Makefile.ref failed:\n" + proc.stdout[-4000:] + proc.stderr[-4000:])
    return REF_DIR


def require():
    """Skip when _ref was never built (no BUILD_INFO); otherwise load all five libraries or fail."""
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
    elif game == "balance":
        create.argtypes = [u32, u32, u32, ctypes.c_int]
        getattr(L, pre + "read").argtypes = [vp, i32p, i32p, i32p, f32p, i32p]
    else:
        create.argtypes = [ctypes.POINTER(ctypes.c_int64), u8p, u8p, u8p, u8p, u8p, u32, u32] + [ctypes.c_int] * 3
        getattr(L, pre + "read").argtypes = [vp, u8p, i32p, i32p, u8p, u8p, i32p] + [i32p] * (game == "simplecooked")
        getattr(L, pre + "node_order").restype = u32
        getattr(L, pre + "node_order").argtypes = [vp, ctypes.c_int, ctypes.POINTER(u32), u32]
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
        check_hanabi_config(config)  # sim.cpp takes anything and indexes out of bounds with a negative deck
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


class _RefKitchen(_Ref):
    """N worlds of a kitchen sim.cpp.  ``params``: the dict OvercookedOracle / SimplecookedOracle take.  The scalars go in
    as int64 and the arrays as bytes (value & 255), since that is what the reference's Config holds."""
    row_extra = None

    def __init__(self, params, num_worlds, fill=0x00, construct=False, graph_order=0, reverse_entities=False):
        self.L = lib(self.game)
        self.params = params
        self.N = N = int(num_worlds)
        self.P, self.H, self.W = P, H, W = int(params["num_players"]), int(params["height"]), int(params["width"])
        self.C, self.F = C, F = H * W, 5 * P + self.row_extra
        self._act_shape = (P, N)
        scalars = np.array([int(params[k]) for k in ("height", "width", "num_players", "placement_in_pot_rew",
                                                      "dish_pickup_rew", "soup_pickup_rew", "horizon")], np.int64)

        def as_bytes(key, count):
            v = np.zeros(max(count, 1), np.uint8)
            given = np.asarray(params[key], np.int64)[:count]
            v[:len(given)] = given & 255
            return v

        arrays = [as_bytes("terrain", max(C, 0)), as_bytes("start_player_x", max(P, 0)), as_bytes("start_player_y", max(P, 0)),
                  as_bytes("recipe_values", NUM_RECIPES), as_bytes("recipe_times", NUM_RECIPES)]
        create = getattr(self.L, "ref_%s_create" % self.game)
        h = create(_p(scalars, ctypes.c_int64), *[_p(a, ctypes.c_uint8) for a in arrays], N, fill, int(construct),
                   int(graph_order), int(reverse_entities))
        self._fin(h)
        self.obs = np.zeros((N, P, C, F), np.uint8)
        self.reward = np.zeros((P, N), np.int32)
        self.done = np.zeros((N,), np.int32)
        self.players = np.zeros((N, P, 6), np.uint8)
        self.objects = np.zeros((N, C, 4), np.uint8)
        self.timestep = np.zeros((N,), np.int32)
        self._read()

    def _out(self):
        return [_p(self.obs, ctypes.c_uint8), _p(self.reward, ctypes.c_int32), _p(self.done, ctypes.c_int32),
                _p(self.players, ctypes.c_uint8), _p(self.objects, ctypes.c_uint8), _p(self.timestep, ctypes.c_int32)]

    def _read(self):
        getattr(self.L, "ref_%s_read" % self.game)(self.h, *self._out())

    def node_order(self, graph_order):
        """The task graph's nodes, numbered as setupTasks adds them, in the order the stand-in runs them for graph_order."""
        out = np.zeros(64, np.uint32)
        n = int(getattr(self.L, "ref_%s_node_order" % self.game)(self.h, int(graph_order), _p(out, ctypes.c_uint32), 64))
        return out[:n].tolist()

    def dump(self):
        """The internal state in the layout of the oracle's dump(): players (N, P, 6), objects (N, C, 4), timestep (N,)."""
        return self.players.copy(), self.objects.copy(), self.timestep.copy()


class RefOvercooked(_RefKitchen):
    game = "overcooked"
    row_extra = 16


class RefSimplecooked(_RefKitchen):
    game = "simplecooked"
    row_extra = 10

    def _out(self):
        if not hasattr(self, "dishes_out"):
            self.dishes_out = np.zeros((self.N,), np.int32)
        return super()._out() + [_p(self.dishes_out, ctypes.c_int32)]

    def dump(self):
        return super().dump() + (self.dishes_out.copy(),)
