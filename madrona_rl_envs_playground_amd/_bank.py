"""What the policy banks share whatever network their members are: the dense tensor of members, the resampling of finished
worlds with its numpy twin, the workspace a simulator keeps, the buffers and checks of a rollout under a bank, and the parts of
cross-play that take the act as a callable.  The banks themselves are their networks' (``_mappo``, ``_wide``).  Every name here
is also ``simulators``'.

May import: _lib, _device, _draws, torch.
"""
import collections
import ctypes

import torch

from . import _lib
from ._device import _check_ids, _seat_mask, _stream_ptr
from ._draws import random_hash


class _PolicyBank:
    """What ``CnnPolicyBank``, ``MlpBasePolicyBank`` and ``WidePolicyBank`` share: K policies of one shape in one dense float32
    tensor ``params`` (K, num_params) whose row k is exactly a member's ``params``, and the members as views of their rows.  A
    subclass names its member class (``_member_class``) and the shape fields (``_shape``) that are the member's attributes, the
    member's leading constructor arguments and its own constructor's keywords; its constructor sets them and hands over to this one."""

    def __init__(self, num_policies, device):
        self.num_policies = int(num_policies)
        if not 1 <= self.num_policies <= _lib.CNN_BANK_MAX_POLICIES:
            raise ValueError(f"a bank holds 1 to {_lib.CNN_BANK_MAX_POLICIES} policies, not {num_policies}")
        self.num_params = self._count_params()
        self.params = torch.zeros((self.num_policies, self.num_params), dtype=torch.float32, device=torch.device(device))
        self._members = {}

    def __len__(self):
        return self.num_policies

    def _count_params(self):
        """the floats of one policy; a member of this shape (on no device) refuses, in its own words, a shape the kernels do not run"""
        return self._member_class(*[getattr(self, name) for name in self._shape], device="meta").num_params

    def policy(self, k):
        """The member (a ``_member_class``) whose ``params`` is row ``k`` of the bank (one object per row)."""
        k = int(k)
        if not 0 <= k < self.num_policies:
            raise IndexError(f"the bank holds policies 0..{self.num_policies - 1}, not {k}")
        member = self._members.get(k)
        if member is None:
            member = self._member_class.__new__(self._member_class)
            for name in self._shape:
                setattr(member, name, getattr(self, name))
            member.params = self.params[k]
            member._module = None
            self._members[k] = member
        return member

    @classmethod
    def from_policies(cls, policies, device=None):
        """A bank holding copies of ``policies`` (``_member_class`` of one shape), in that order (``device``: default the first one's)."""
        policies = list(policies)
        if not policies or not all(isinstance(p, cls._member_class) for p in policies):
            raise ValueError(f"from_policies takes a non-empty list of {cls._member_class.__name__}")
        shape = {name: getattr(policies[0], name) for name in cls._shape}
        if any(getattr(p, name) != value for p in policies for name, value in shape.items()):
            raise ValueError("the policies of a bank must have one shape")
        bank = cls(num_policies=len(policies), device=device if device is not None else policies[0].params.device, **shape)
        with torch.no_grad():
            for k, p in enumerate(policies):
                bank.params[k].copy_(p.params)
        return bank

    def _check_params(self, gpu_id):
        """``params`` is what the bank kernels take on device ``gpu_id``"""
        p = self.params
        if (not p.is_cuda or p.device.index != gpu_id or p.dtype != torch.float32 or not p.is_contiguous() or
                tuple(p.shape) != (self.num_policies, self.num_params)):
            raise ValueError(f"bank.params must be a contiguous float32 tensor (num_policies, num_params) on cuda:{gpu_id}")


def _bank_workspace(sim, attribute, size):
    """the plan's workspace a MAPPO bank act takes by default: one the simulator keeps as ``attribute``, of at least ``size`` bytes"""
    workspace = getattr(sim, attribute, None)
    if workspace is None or workspace.numel() < size:
        workspace = torch.empty(int(size), dtype=torch.uint8, device=torch.device("cuda", sim.gpu_id))
        setattr(sim, attribute, workspace)
    return workspace


CNN_RESAMPLE_MODES = {"robin": _lib.CNN_RESAMPLE_ROBIN, "random": _lib.CNN_RESAMPLE_RANDOM}


class CnnResample:
    """How finished worlds draw their next policies (``mrl_cnn_resample``): ``mode`` "robin" or "random"; ``first_id`` and
    ``num_ids`` an int or one per seat -- seat p draws from ``[first_id[p], first_id[p] + num_ids[p])``; ``seed`` for "random"."""

    def __init__(self, mode, first_id, num_ids, num_players, seed=0):
        if mode not in CNN_RESAMPLE_MODES and mode not in CNN_RESAMPLE_MODES.values():
            raise ValueError(f"mode must be one of {sorted(CNN_RESAMPLE_MODES)}, got {mode!r}")
        self.mode = CNN_RESAMPLE_MODES.get(mode, mode)
        per_seat = lambda v: [int(v)] * int(num_players) if isinstance(v, int) else [int(x) for x in v]  # noqa: E731
        self.first_id, self.num_ids = per_seat(first_id), per_seat(num_ids)
        if len(self.first_id) != int(num_players) or len(self.num_ids) != int(num_players):
            raise ValueError(f"first_id and num_ids take an int or one entry per seat ({num_players})")
        if any(f < 0 or n < 0 for f, n in zip(self.first_id, self.num_ids)):
            raise ValueError("first_id and num_ids must not be negative")
        self.seed = int(seed)
        self._first = (ctypes.c_uint32 * len(self.first_id))(*self.first_id)
        self._num = (ctypes.c_uint32 * len(self.num_ids))(*self.num_ids)
        self.struct = _lib.CnnResampleDesc(self.mode, self._first, self._num, self.seed & (2 ** 64 - 1))


def resample_twin(ids, episodes, done, mode, first_id, num_ids, players, seed=0):
    """``mrl_cnn_bank_resample`` in numpy, in place on ``ids`` (N, P) int32 and ``episodes`` (N) int32; ``done`` (N)."""
    import numpy as np
    n_players = ids.shape[1]
    finished = np.flatnonzero(np.asarray(done) != 0)
    episodes[finished] += 1
    for p in range(n_players):
        if not (players >> p) & 1:
            continue
        rows = finished[ids[finished, p] >= 0]
        first, num = np.uint32(first_id[p]), np.uint32(num_ids[p])
        old = ids[rows, p].astype(np.uint32)
        if CNN_RESAMPLE_MODES.get(mode, mode) == _lib.CNN_RESAMPLE_ROBIN:
            new = first + (old - first + np.uint32(1)) % num
        else:
            h = random_hash(seed, episodes[rows].astype(np.uint32), rows.astype(np.uint32), np.full(rows.shape, p, dtype=np.uint32))
            new = first + (((h >> np.uint32(8)).astype(np.uint64) * np.uint64(num)) >> np.uint64(24)).astype(np.uint32)
        ids[rows, p] = new.astype(np.int32)


def _bank_resample(sim, entry_point, worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed):
    """The three resamples behind their own check of the simulator: ``entry_point`` of the library on ``ids`` (worlds, seats) and
    ``episodes`` (worlds)."""
    _check_ids(sim, ids, (worlds, seats), "ids")
    _check_ids(sim, episodes, (worlds,), "episodes")
    resample = mode if isinstance(mode, CnnResample) else CnnResample(mode, first_id, num_ids, seats, seed)
    _lib.check(getattr(sim._L, entry_point)(sim._handle, _seat_mask(players, seats), ctypes.byref(resample.struct), ids.data_ptr(),
                                            episodes.data_ptr(), _stream_ptr(sim.gpu_id)))


BankResample = CnnResample  # the descriptor serves both networks' banks
CrossPlayResult = collections.namedtuple("CrossPlayResult", "mean_return episodes")  # each (Ka, Kb), on the device
BEAM_TIME = 3  # src/balance_beam_env/sim.cpp: an observation holds TIME positions per seat, an episode is at most TIME - 1 moves


def _cross_play_pairs(sim, bank, members_a, members_b, n, p):
    """What every ``cross_play`` sets up alike on ``n`` worlds of ``p`` seats: the members of both seats (default every row of the
    bank) and the worlds' pairs -> (Ka, Kb, ``pair`` (N): n mod (Ka Kb), ``ids`` int32 (N, 2): the rows world n plays under)."""
    if p != 2:
        raise ValueError(f"cross_play pairs seat 0 with seat 1: the env has {p} seats")
    a = list(range(bank.num_policies)) if members_a is None else [int(k) for k in members_a]
    b = list(range(bank.num_policies)) if members_b is None else [int(k) for k in members_b]
    if not a or not b or any(not 0 <= k < bank.num_policies for k in a + b):
        raise ValueError(f"members must name rows 0..{bank.num_policies - 1} of the bank")
    pairs = len(a) * len(b)
    if n < pairs:
        raise ValueError(f"{n} worlds cannot play {len(a)} x {len(b)} pairs")
    device = torch.device("cuda", sim.gpu_id)
    pair = torch.arange(n, device=device) % pairs
    ids = torch.stack([torch.tensor(a, device=device)[pair // len(b)], torch.tensor(b, device=device)[pair % len(b)]], dim=1).to(torch.int32).contiguous()
    return len(a), len(b), pair, ids


def _cross_play_result(ka, kb, pair, total, finished):
    """the worlds' float64 return sums and int64 episode counts reduced per pair -> ``CrossPlayResult``"""
    count = torch.zeros(ka * kb, dtype=torch.int64, device=pair.device).index_add_(0, pair, finished)
    summed = torch.zeros(ka * kb, dtype=torch.float64, device=pair.device).index_add_(0, pair, total)
    return CrossPlayResult((summed / count).view(ka, kb), count.view(ka, kb))


def _cross_play_counted(sim, bank, members_a, members_b, steps, act):
    """What ``cross_play`` shares between the games whose episodes have no fixed length (``sim``: P = 2 seats, DONE (N),
    the last-episode return (P, N)): the pairs, the restart, ``steps`` times (``act(ids, t)``, step, count) and the per-pair
    reduction.  ``act`` enqueues step t's acts of both seats under ``ids`` (N, 2)."""
    p, n = tuple(sim.observation_tensor().shape[:2])
    ka, kb, pair, ids = _cross_play_pairs(sim, bank, members_a, members_b, n, p)
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be positive")
    device = pair.device
    sim.enable_episode_stats()
    sim.reset_worlds(None)
    done = sim.done_tensor().to_torch().reshape(n)
    last = sim.last_episode_return_tensor().to_torch().reshape(p, n)[0]  # the team's return, as seat 0 received it
    total = torch.zeros(n, dtype=torch.float64, device=device)
    finished = torch.zeros(n, dtype=torch.int64, device=device)
    for t in range(steps):
        act(ids, t)
        sim.step()
        over = done != 0
        total += torch.where(over, last.to(torch.float64), torch.zeros_like(total))  # float32 returns: the float64 sums are exact
        finished += over
    return _cross_play_result(ka, kb, pair, total, finished)


def _bank_rollout_buffers(env, num_steps, seats, ids_record, episodes, resample):
    """What the two env mixins' ``rollout_bank`` set up alike -> (``ids_record``, made when ``None``; ``episodes``, with a
    ``resample`` and ``None`` the env's ``bank_episodes``, made once and kept)"""
    device = env.static_actions.device
    if ids_record is None:
        ids_record = torch.empty((int(num_steps) + 1, env.num_envs, seats), dtype=torch.int32, device=device)
    if episodes is None and resample is not None:
        episodes = getattr(env, "bank_episodes", None)
        if episodes is None:
            episodes = env.bank_episodes = torch.zeros(env.num_envs, dtype=torch.int32, device=device)
    return ids_record, episodes


def _check_bank_rollout(sim, record, cells, ids_record, resample, episodes):
    """What ``rollout_cnn_bank`` and ``rollout_mlpbase_bank`` check alike for ``cells`` = (N, P): ``ids_record`` (T + 1, N, P), the
    ``resample`` and its ``episodes`` (N)"""
    if ids_record is not None:
        _check_ids(sim, ids_record, (record.num_steps + 1,) + tuple(cells), "ids_record")
    if resample is not None and not isinstance(resample, CnnResample):
        raise ValueError("resample must be a CnnResample or None")
    if episodes is not None:
        _check_ids(sim, episodes, tuple(cells[:1]), "episodes")
    elif resample is not None:
        raise ValueError("a resample needs episodes, an int32 tensor (num_worlds,)")
