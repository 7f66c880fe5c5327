"""Python-visible simulator classes: drop-in for the reference's nanobind modules.

    reference module                            class here
    build.madrona_overcooked_example_python  -> OvercookedSimulator   (src/overcooked_env/bindings.cpp:11-84)
    build.madrona_simplecooked_example_python -> SimplecookedSimulator (src/overcooked2_env/bindings.cpp:11-84)
    build.madrona_hanabi_example_python      -> HanabiSimulator       (src/hanabi_env/bindings.cpp:8-48)
    build.madrona_cartpole_example_python    -> CartpoleSimulator     (src/cartpole_env/bindings.cpp:8-31)
    build.madrona_balance_example_python     -> BalanceBeamSimulator  (src/balance_beam_env/bindings.cpp:8-34)
    build.madrona_acrobat_example_python     -> AcrobotSimulator      (src/acrobat_env/bindings.cpp; alias AcrobatSimulator)

Same constructor keywords, same method names; every ``*_tensor()`` returns an
object whose ``to_torch()`` yields a persistent zero-copy ``torch.Tensor`` on the
simulator's GPU (the reference's ``madrona.py.Tensor.to_torch()``).  ``madrona``
below mimics the ``<module>.madrona`` submodule the wrappers reach for
(envs/overcooked_env.py:31).

Everything is computed by libmrl_envs.so (HIP, gfx950).  ``ExecMode.CPU`` raises:
the reference's CPU TaskGraph executor is out of scope, and a
silent CPU path would defeat the parity tests.
"""
import collections
import copy
import ctypes
import enum

import torch

from . import _lib
from ._lib import MrlError  # noqa: F401  (re-export)



# The raw handle of torch's current stream on a device.  ``torch.cuda.current_stream(d).cuda_stream`` builds a Stream
# object on every call (1.1 us measured, a fifth of a step call's host cost -- small batches are bound by that cost,
# tools/host_overhead.py); torch's own raw getter returns the same pointer as an int.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_ptr(device_index):
    if _raw_stream is not None:
        return _raw_stream(device_index)
    return torch.cuda.current_stream(device_index).cuda_stream


class ExecMode(enum.Enum):
    CPU = 0
    CUDA = 1
    HIP = 1  # alias: on this engine the GPU mode is HIP on MI355X


class madrona:  # noqa: N801  (mirrors `<module>.madrona.ExecMode`)
    ExecMode = ExecMode


_TORCH_DTYPE = {
    _lib.MRL_INT8: (torch.int8, "|i1", 1),
    _lib.MRL_UINT8: (torch.uint8, "|u1", 1),
    _lib.MRL_INT32: (torch.int32, "<i4", 4),
    _lib.MRL_FLOAT32: (torch.float32, "<f4", 4),
    _lib.MRL_UINT32: (torch.int32, "<i4", 4),  # torch has no general uint32; same bits
    _lib.MRL_FLOAT64: (torch.float64, "<f8", 8),
}


class _DeviceBlob:
    """Carrier for ``__cuda_array_interface__``; keeps the simulator alive."""

    def __init__(self, owner, ptr, shape, strides_bytes, typestr):
        self._owner = owner
        self.__cuda_array_interface__ = {
            "shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2,
            "strides": tuple(strides_bytes),
        }


class Tensor:
    """What ``sim.*_tensor()`` returns (stands in for ``madrona::py::Tensor``)."""

    def __init__(self, sim, slot):
        desc = _lib.TensorDesc()
        _lib.check(_lib.lib().mrl_tensor(sim._handle, slot, ctypes.byref(desc)))
        self._sim = sim
        self.ptr = desc.data
        self.dtype_code = desc.dtype
        self.shape = tuple(desc.shape[i] for i in range(desc.ndim))
        self.strides = tuple(desc.strides[i] for i in range(desc.ndim))
        self.device = desc.device
        self._torch = None

    def to_torch(self):
        if self._torch is None:
            dtype, typestr, size = _TORCH_DTYPE[self.dtype_code]
            blob = _DeviceBlob(self._sim, self.ptr, self.shape, [s * size for s in self.strides], typestr)
            t = torch.as_tensor(blob, device=torch.device("cuda", self.device))
            if t.dtype != dtype:
                t = t.view(dtype)
            if t.data_ptr() != self.ptr:
                raise MrlError("torch.as_tensor copied the exported buffer instead of aliasing it")
            self._torch = t
        return self._torch


def random_hash(seed, step, world, player):
    """The counter-based hash behind the device-side random policies (``mrl_rollout_random``;
    csrc/random_policy.hpp), restated with numpy so a stream can be replayed.  uint32 array."""
    import numpy as np
    m = np.uint64(0xFFFFFFFF)
    seed = int(seed) & (2 ** 64 - 1)
    h = (np.uint64(seed & 0xFFFFFFFF) ^ (np.uint64(step) * np.uint64(0x9E3779B9) & m) ^
         (np.asarray(world, np.uint64) * np.uint64(0x85EBCA6B) & m) ^
         ((np.asarray(player, np.uint64) + np.uint64(1)) * np.uint64(0xC2B2AE35) & m) ^
         (np.uint64(seed >> 32) * np.uint64(0x27D4EB2F) & m))
    h ^= h >> np.uint64(16)
    h = h * np.uint64(0x7FEB352D) & m
    h ^= h >> np.uint64(15)
    h = h * np.uint64(0x846CA68B) & m
    h ^= h >> np.uint64(16)
    return h.astype(np.uint32)


def sample_u(seed, step, world):
    """The uniform number behind ``rollout_policy``'s draw for (step index, world): ``(hash >> 8) * 2^-24`` with player 0,
    a multiple of 2^-24 in [0, 1) and exact in float32 (``mrl_rollout_policy``).  float32 array."""
    import numpy as np
    h = random_hash(seed, step, world, np.zeros_like(np.asarray(world)))
    return (h >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def random_action(seed, step, world, player):
    """Overcooked: ``(hash * 6) >> 32`` for (step index, world, player)."""
    import numpy as np
    return ((random_hash(seed, step, world, player).astype(np.uint64) * np.uint64(6)) >> np.uint64(32)).astype(np.int32)


def random_cartpole_action(seed, step, world):
    """Cartpole: the hash's top bit (player 0)."""
    import numpy as np
    return (random_hash(seed, step, world, np.zeros_like(np.asarray(world))) >> np.uint32(31)).astype(np.int32)


def random_acrobot_action(seed, step, world):
    """Acrobot: ``(hash * 3) >> 32`` for (step index, world, player 0)."""
    import numpy as np
    h = random_hash(seed, step, world, np.zeros_like(np.asarray(world)))
    return ((h.astype(np.uint64) * np.uint64(3)) >> np.uint64(32)).astype(np.int32)


def random_hanabi_action(seed, step, world, mover, legal_mask):
    """Hanabi: the k-th legal move of the mover, ``k = (hash * count) >> 32``.
    ``legal_mask``: (n, 20) 0/1 array of the mover's legal moves, ``mover``: (n,) 0/1."""
    import numpy as np
    legal_mask = np.asarray(legal_mask) != 0
    count = legal_mask.sum(-1).astype(np.uint64)
    k = (random_hash(seed, step, world, mover).astype(np.uint64) * count) >> np.uint64(32)
    rank = np.cumsum(legal_mask, axis=-1) - 1                      # rank of each legal move among the legal ones
    pick = legal_mask & (rank == k[:, None].astype(np.int64))
    return np.where(count > 0, pick.argmax(-1), 0).astype(np.int32)


def _mlp(inputs, hidden, outputs):
    nn = torch.nn
    return nn.Sequential(nn.Linear(inputs, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(), nn.Linear(hidden, outputs))


class MlpAgent(torch.nn.Module):
    """What ``MlpPolicy.module()`` returns: the actor-critic of the reference's trainer (scripts/cartpole_train_torch.py:105-131,
    ``Agent``) by shape and method names, for the update phase.  Initialisation is torch's default; the trainer's is its own."""

    def __init__(self, obs_dim, num_actions, hidden=64):
        super().__init__()
        self.critic = _mlp(obs_dim, hidden, 1)
        self.actor = _mlp(obs_dim, hidden, num_actions)

    def get_value(self, x):
        return self.critic(x)

    def get_action_and_value(self, x, action=None):
        dist = torch.distributions.Categorical(logits=self.actor(x))
        if action is None:
            action = dist.sample()
        return action, dist.log_prob(action), dist.entropy(), self.critic(x)


class MlpPolicy:
    """The parameters ``rollout_policy`` runs: one flat float32 tensor ``params`` in the order of
    ``parameters_to_vector(agent.parameters())`` for an agent with ``critic`` and ``actor`` =
    ``Sequential(Linear(D, 64), Tanh, Linear(64, 64), Tanh, Linear(64, 1 or A))`` (``mrl_mlp_policy``).  The kernel reads the
    tensor in place: between rollouts a trainer steps its optimizer and calls ``load_(agent)``.  ``observation``: "state"
    (the simulator's STATE row, D = 4) or "gym" (Acrobot's six values, D = 6)."""

    def __init__(self, obs_dim, num_actions, hidden=64, observation="state", device="cuda:0"):
        if observation not in ("state", "gym"):
            raise ValueError(f"observation must be 'state' or 'gym', got {observation!r}")
        self.obs_dim, self.num_actions, self.hidden, self.observation = int(obs_dim), int(num_actions), int(hidden), observation
        count = int(_lib.lib().mrl_mlp_policy_num_params(self.obs_dim, self.hidden, self.num_actions))
        self.params = torch.zeros(count, dtype=torch.float32, device=torch.device(device))

    @staticmethod
    def _shape_of(agent):
        """(obs_dim, num_actions, hidden) of an agent of the expected form; ValueError otherwise."""
        nn = torch.nn
        nets = []
        for name in ("critic", "actor"):
            net = getattr(agent, name, None)
            if (not isinstance(net, nn.Sequential) or len(net) != 5 or not all(isinstance(net[i], nn.Linear) for i in (0, 2, 4)) or
                    not all(isinstance(net[i], nn.Tanh) for i in (1, 3)) or any(net[i].bias is None for i in (0, 2, 4))):
                raise ValueError(f"agent.{name} must be Sequential(Linear, Tanh, Linear, Tanh, Linear) with biases")
            nets.append(net)
        critic, actor = nets
        d, h = critic[0].in_features, critic[0].out_features
        for net, out in ((critic, 1), (actor, actor[4].out_features)):
            shapes = [(net[i].in_features, net[i].out_features) for i in (0, 2, 4)]
            if shapes != [(d, h), (h, h), (h, out)]:
                raise ValueError(f"agent's layers are {shapes}, expected {[(d, h), (h, h), (h, out)]}")
        return d, actor[4].out_features, h

    @staticmethod
    def _flat(agent):
        return torch.cat([p.detach().reshape(-1) for net in (agent.critic, agent.actor) for p in net.parameters()])

    @classmethod
    def from_module(cls, agent, observation="state", device=None):
        """A policy of ``agent``'s shape holding a copy of its parameters (``device``: default the agent's own)."""
        d, a, h = cls._shape_of(agent)
        policy = cls(d, a, h, observation, device if device is not None else agent.critic[0].weight.device)
        return policy.load_(agent)

    def load_(self, agent):
        """One flat in-place copy of ``agent``'s parameters into ``params`` (the tensor the kernel reads does not move)."""
        if self._shape_of(agent) != (self.obs_dim, self.num_actions, self.hidden):
            raise ValueError(f"agent has (obs_dim, num_actions, hidden) = {self._shape_of(agent)}, this policy "
                             f"{(self.obs_dim, self.num_actions, self.hidden)}")
        with torch.no_grad():
            self.params.copy_(self._flat(agent))
        return self

    def module(self):
        """A new ``MlpAgent`` on ``params``' device with these parameters (a copy)."""
        agent = MlpAgent(self.obs_dim, self.num_actions, self.hidden).to(self.params.device)
        at = 0
        with torch.no_grad():
            for net in (agent.critic, agent.actor):
                for p in net.parameters():
                    p.copy_(self.params[at:at + p.numel()].view_as(p))
                    at += p.numel()
        return agent


class _CnnLayer(torch.nn.Module):
    """train/MAPPO/utils/cnn.py:11-42 for use_ReLU: ``cnn`` = Conv2d 3 x 3, ReLU, Flatten, Linear, ReLU, Linear, ReLU"""

    def __init__(self, width, height, channels, hidden):
        super().__init__()
        nn = torch.nn
        self.cnn = nn.Sequential(nn.Conv2d(channels, hidden // 2, kernel_size=3, stride=1), nn.ReLU(), nn.Flatten(),
                                 nn.Linear(hidden // 2 * (width - 2) * (height - 2), hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU())

    def forward(self, x):
        return self.cnn(x.movedim(-1, -3))


class _CnnBase(torch.nn.Module):
    def __init__(self, width, height, channels, hidden):
        super().__init__()
        self.cnn = _CnnLayer(width, height, channels, hidden)

    def forward(self, x):
        return self.cnn(x)


class _CategoricalHead(torch.nn.Module):
    def __init__(self, hidden, num_actions):
        super().__init__()
        self.linear = torch.nn.Linear(hidden, num_actions)


class _ActLayer(torch.nn.Module):
    def __init__(self, hidden, num_actions):
        super().__init__()
        self.action_out = _CategoricalHead(hidden, num_actions)


class _CnnActor(torch.nn.Module):
    """``R_Actor``'s parameters by name for the CNN, non-recurrent configuration: ``base.cnn.cnn.0/3/5``, ``act.action_out.linear``"""

    def __init__(self, width, height, channels, hidden, num_actions):
        super().__init__()
        self.base = _CnnBase(width, height, channels, hidden)
        self.act = _ActLayer(hidden, num_actions)

    def forward(self, obs):
        return self.act.action_out.linear(self.base(obs))


class _CnnCritic(torch.nn.Module):
    """``R_Critic``'s parameters by name without PopArt: ``base.cnn.cnn.0/3/5``, ``v_out``"""

    def __init__(self, width, height, channels, hidden):
        super().__init__()
        self.base = _CnnBase(width, height, channels, hidden)
        self.v_out = torch.nn.Linear(hidden, 1)

    def forward(self, state):
        return self.v_out(self.base(state))


class CnnActorCritic(torch.nn.Module):
    """MAPPO's CNN actor-critic for the two kitchens, Overcooked (``channels`` = 5P + 16) and Simplecooked (5P + 10, one or two
    players) (train/MAPPO/utils/cnn.py:26-42, r_actor_critic.py, utils/distributions.py:55-68;
    non-recurrent, no PopArt, ``hidden_size`` 64): ``actor`` and ``critic`` take the (N, W, H, F) observation as floats.  Their
    state dicts have the reference's keys, so ``actor.load_state_dict`` / ``critic.load_state_dict`` take a reference checkpoint's
    two files.  Initialisation is the reference's: orthogonal weights with the ReLU gain, 0.01 for the action head (``args.gain``),
    1 for ``v_out`` (r_actor_critic.py:136-142), zero biases."""

    def __init__(self, width, height, channels, hidden=64, num_actions=6):
        super().__init__()
        self.width, self.height, self.channels, self.hidden, self.num_actions = int(width), int(height), int(channels), int(hidden), int(num_actions)
        self.actor = _CnnActor(self.width, self.height, self.channels, self.hidden, self.num_actions)
        self.critic = _CnnCritic(self.width, self.height, self.channels, self.hidden)
        relu_gain = torch.nn.init.calculate_gain("relu")
        for net, head, head_gain in ((self.actor, self.actor.act.action_out.linear, 0.01), (self.critic, self.critic.v_out, 1.0)):
            for i in (0, 3, 5):
                torch.nn.init.orthogonal_(net.base.cnn.cnn[i].weight, gain=relu_gain)
                torch.nn.init.constant_(net.base.cnn.cnn[i].bias, 0.0)
            torch.nn.init.orthogonal_(head.weight, gain=head_gain)
            torch.nn.init.constant_(head.bias, 0.0)

    def get_value(self, state):
        return self.critic(state)

    def get_action_and_value(self, obs, action=None, deterministic=False):
        dist = torch.distributions.Categorical(logits=self.actor(obs))
        if action is None:
            action = dist.probs.argmax(dim=-1) if deterministic else dist.sample()
        return action, dist.log_prob(action), dist.entropy(), self.critic(obs)


class _FlatPolicy:
    """What ``CnnPolicy`` and ``MlpBasePolicy`` share: one flat float32 tensor ``params``, the actor's tensors and then the critic's in
    the order of ``parameters_to_vector`` of the policy's torch module, and that module with its parameters as VIEWS into ``params``.
    A subclass names its module class (``_module_class``, ``_module_name`` for messages), the shape fields that are both its own
    constructor's and the module's leading arguments (``_shape``), its ``num_params`` and what ``mappo_update`` needs of it:
    ``_mappo_workspace_bytes``, ``_mappo_check`` and ``_mappo_batch``."""

    def _allocate(self, device, supported):
        if self.num_params == 0:
            raise ValueError(supported)
        self.params = torch.zeros(self.num_params, dtype=torch.float32, device=torch.device(device))
        self._module = None

    def _check_params(self, gpu_id=None):
        """``params`` is what the kernels take (``gpu_id``: on that device; default any GPU)"""
        p = self.params
        if (not p.is_cuda or (gpu_id is not None and p.device.index != gpu_id) or p.dtype != torch.float32 or not p.is_contiguous() or
                p.numel() != self.num_params):
            where = "a GPU" if gpu_id is None else f"cuda:{gpu_id}"
            raise ValueError(f"policy.params must be a contiguous float32 tensor of num_params elements on {where}")
        return p

    @classmethod
    def from_module(cls, module, device=None):
        """A policy of ``module``'s shape holding a copy of its parameters (``device``: default its own)."""
        if not isinstance(module, cls._module_class):
            raise ValueError(f"module must be {cls._module_name}")
        own = next(module.parameters()).device
        policy = cls(*[getattr(module, name) for name in cls._shape], device if device is not None else own)
        with torch.no_grad():
            policy.params.copy_(torch.nn.utils.parameters_to_vector(module.parameters()).detach())
        return policy

    def module(self):
        """The torch module whose parameters alias ``params`` (one object per policy)."""
        if self._module is None:
            module = self._module_class(*[getattr(self, name) for name in self._shape])
            at = 0
            for p in module.parameters():  # actor first, then critic: the order of the flat array
                p.data = self.params[at:at + p.numel()].view(p.shape)
                at += p.numel()
            assert at == self.params.numel()
            self._module = module
        return self._module


class CnnPolicy(_FlatPolicy):
    """The parameters ``mrl_cnn_act`` runs on an Overcooked or a Simplecooked simulator of the policy's shape: one flat float32 tensor ``params``, the actor's eight tensors and then the critic's in
    the order of ``parameters_to_vector(CnnActorCritic.parameters())`` (``mrl_cnn_policy``).  ``module()`` returns a
    ``CnnActorCritic`` whose parameters are VIEWS into ``params``: an optimizer's in-place step on them is what the kernel reads
    next, with no copy in between (so there is no ``load_``)."""

    _module_class, _module_name, _shape = CnnActorCritic, "a CnnActorCritic", ("width", "height", "channels", "hidden", "num_actions")

    def __init__(self, width, height, channels, hidden=64, num_actions=6, device="cuda:0"):
        self.width, self.height, self.channels, self.hidden, self.num_actions = int(width), int(height), int(channels), int(hidden), int(num_actions)
        self._allocate(device, f"mrl_cnn_act runs hidden = {_lib.CNN_HIDDEN}, num_actions = {_lib.CNN_ACTIONS} and kitchens of at least 3 x 3")

    @property
    def num_params(self):
        return int(_lib.lib().mrl_cnn_policy_num_params(self.width, self.height, self.channels, self.hidden, self.num_actions))

    def desc(self):
        return _lib.CnnPolicyDesc(self.params.data_ptr(), self.hidden, 0)

    # what MappoOptimizer and mappo_update ask of a policy
    def _mappo_workspace_bytes(self, minibatch_size, num_minibatches, out, members=None):
        """``members``: for that many members of a bank in one ``mappo_update_bank``"""
        shape = (self.width, self.height, self.channels, self.hidden, minibatch_size, num_minibatches)
        if members is None:
            return _lib.lib().mrl_mappo_workspace_bytes(*shape, out)
        return _lib.lib().mrl_mappo_bank_workspace_bytes(*shape, members, out)

    def _mappo_check(self, record, ring):
        if not isinstance(record, CnnRecord):
            raise ValueError("record must be a CnnRecord")

    def _mappo_batch(self, record, ring, count):
        """-> ((entry point, the bank's), policy struct, batch struct's type, the batch's observations): the record's ring"""
        row_bytes = self.width * self.height * self.channels
        if (not isinstance(ring, torch.Tensor) or ring.device != self.params.device or ring.dtype != torch.int8 or not ring.is_contiguous() or
                ring.numel() < count * row_bytes):
            raise ValueError(f"ring must be a contiguous torch.int8 tensor on {self.params.device} of at least {count * row_bytes} elements: "
                             f"(T + 1, N, P, H, W, F) for the policy's {self.width} x {self.height} kitchen with {self.channels} channels")
        shape = _lib.MappoPolicyDesc(self.params.data_ptr(), self.hidden, 0, self.width, self.height, self.channels)
        return (_lib.lib().mrl_mappo_update, _lib.lib().mrl_mappo_bank_update), shape, _lib.MappoBatch, ring


class _MappoRecord:
    """The buffers ``CnnRecord`` and ``MlpBaseRecord`` share: torch tensors by name plus the ctypes struct over them.  ``actions``
    int32, ``logprobs``, ``rewards``, ``dones`` (T, N, P); ``values`` (T + 1, N, P), row T the closing value; ``next_done`` (N, P);
    ``logits`` (T, N, P, actions) on request.  A subclass names its struct, the struct's buffers and the width of ``logits``."""

    def __init__(self, num_steps, num_worlds, num_players, device, logits=False):
        t, n, p = int(num_steps), int(num_worlds), int(num_players)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
        self.num_steps, self.num_worlds, self.num_players = t, n, p
        self.actions = z((t, n, p), torch.int32)
        self.logprobs, self.rewards, self.dones = z((t, n, p)), z((t, n, p)), z((t, n, p))
        self.values, self.next_done = z((t + 1, n, p)), z((n, p))
        self.logits = z((t, n, p, self._actions)) if logits else None
        self._own_buffers(z, t, n, p)
        self.struct = self._struct(*[getattr(self, name).data_ptr() if getattr(self, name) is not None else None for name in self._buffers], t)

    def _own_buffers(self, z, t, n, p):
        pass

    def rollout(self):
        """The record as the ``Rollout`` that ``gae`` takes: views flattened to N * P columns, ``next_value`` = ``values[T]``."""
        t, cols = self.num_steps, self.num_worlds * self.num_players
        flat = lambda x: x.view(t, cols)  # noqa: E731
        return Rollout(None, flat(self.actions), flat(self.logprobs), self.values[:t].view(t, cols), flat(self.rewards), flat(self.dones),
                       None, self.values[t].view(cols), self.next_done.view(cols))

    @classmethod
    def _for_rollout(cls, record, num_steps, num_worlds, num_players, device):
        """``record``, or a new one when it is None, for a rollout of ``num_steps`` steps"""
        if record is None:
            record = cls(num_steps, num_worlds, num_players, device)
        if record.num_steps != int(num_steps):
            raise ValueError(f"record holds {record.num_steps} steps, asked for {num_steps}")
        return record


class CnnRecord(_MappoRecord):
    """The buffers of ``mrl_cnn_act`` / ``mrl_rollout_cnn`` (``mrl_cnn_record``): torch tensors by name plus the ctypes struct over
    them.  ``actions`` int32, ``logprobs``, ``rewards``, ``dones`` (T, N, P); ``values`` (T + 1, N, P), row T the closing value;
    ``next_done`` (N, P); ``logits`` (T, N, P, 6) on request."""

    _struct, _buffers, _actions = _lib.CnnRecordDesc, _lib.CNN_RECORD_BUFFERS, _lib.CNN_ACTIONS


def _cnn_call_args(sim, policy, players, record):
    if not isinstance(policy, CnnPolicy):
        raise ValueError("policy must be a CnnPolicy")
    p = policy._check_params(sim.gpu_id)
    shape = sim.observation_world_major_tensor().shape  # (N, P, H, W, F)
    if (policy.height, policy.width, policy.channels) != tuple(shape[2:]):
        raise ValueError(f"the policy is for a {policy.width} x {policy.height} kitchen with {policy.channels} channels, the simulator's "
                         f"is {shape[3]} x {shape[2]} with {shape[4]} (Overcooked: 5P + 16 channels, Simplecooked: 5P + 10)")
    if record is not None and (not isinstance(record, CnnRecord) or record.num_worlds != shape[0] or record.num_players != shape[1] or
                               record.actions.device != p.device):
        raise ValueError(f"record must be a CnnRecord of {shape[0]} worlds and {shape[1]} players on cuda:{sim.gpu_id}")
    return _seat_mask(players, shape[1])


def _seat_mask(players, num_players):
    """``players`` (None: every seat; a bit mask; an iterable of seats) as the C ABI's mask"""
    mask = (1 << num_players) - 1 if players is None else players
    if not isinstance(mask, int):
        mask = sum(1 << int(seat) for seat in mask)
    return mask & 0xFFFFFFFF if 0 <= mask < 2 ** 32 else 0xFFFFFFFF


def cnn_act(sim, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False, value_only=False, workspace=None):
    """``mrl_cnn_act`` on torch's current stream of the simulator's device: the seats in ``players`` (a bit mask or an iterable of
    seats; default all) of an Overcooked or Simplecooked simulator act under ``policy`` (a ``CnnPolicy``) on the observations the simulator's
    most recent step wrote, wherever that was; with ``record`` (a ``CnnRecord``) row ``row`` of its buffers is written.
    ``value_only``: the closing act at row T.  ``workspace``: default one the simulator keeps."""
    mask = _cnn_call_args(sim, policy, players, record)
    if workspace is None:
        workspace = getattr(sim, "_cnn_workspace", None)
        if workspace is None:
            size = int(sim._L.mrl_cnn_workspace_bytes(sim.num_worlds, sim.observation_world_major_tensor().shape[1]))
            workspace = sim._cnn_workspace = torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", sim.gpu_id))
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.CNN_VALUE_ONLY if value_only else 0)
    desc = policy.desc()
    rc = sim._L.mrl_cnn_act(sim._handle, mask, ctypes.byref(desc), ctypes.byref(record.struct) if record is not None else None, int(row),
                            int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, flags, workspace.data_ptr(), workspace.numel(),
                            _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


class _PolicyBank:
    """What ``CnnPolicyBank``, ``MlpBasePolicyBank`` and ``WidePolicyBank`` share: K policies of one shape in one dense float32
    tensor ``params`` (K, num_params) whose row k is exactly a member's ``params``, and the members as views of their rows.  A
    subclass names its member class (``_member_class``) and the shape fields (``_shape``) that are the member's attributes and its
    own constructor's keywords; its constructor sets them and hands over to this one; ``_count_params`` gives the floats of one
    policy and refuses a shape the kernels do not run."""

    def __init__(self, num_policies, device):
        self.num_policies = int(num_policies)
        if not 1 <= self.num_policies <= _lib.CNN_BANK_MAX_POLICIES:
            raise ValueError(f"a bank holds 1 to {_lib.CNN_BANK_MAX_POLICIES} policies, not {num_policies}")
        self.num_params = self._count_params()
        self.params = torch.zeros((self.num_policies, self.num_params), dtype=torch.float32, device=torch.device(device))
        self._members = {}

    def __len__(self):
        return self.num_policies

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


class CnnPolicyBank(_PolicyBank):
    """K ``CnnPolicy`` of one shape in one dense float32 tensor ``params`` (K, num_params) (``mrl_cnn_bank``): row k is exactly
    what a ``CnnPolicy``'s ``params`` is.  ``policy(k)`` is a ``CnnPolicy`` whose ``params`` IS row k, a contiguous view, so
    ``cnn_act``, ``MappoOptimizer``, ``mappo_update`` and ``.module()`` work on a member unchanged and training a member is what the
    next ``cnn_act_bank`` reads.  1 <= K <= 256."""

    _member_class, _shape = CnnPolicy, CnnPolicy._shape

    def __init__(self, width, height, channels, num_policies, hidden=64, num_actions=6, device="cuda:0"):
        self.width, self.height, self.channels, self.hidden, self.num_actions = int(width), int(height), int(channels), int(hidden), int(num_actions)
        super().__init__(num_policies, device)

    def _count_params(self):
        count = int(_lib.lib().mrl_cnn_policy_num_params(self.width, self.height, self.channels, self.hidden, self.num_actions))
        if count == 0:
            raise ValueError(f"mrl_cnn_act runs hidden = {_lib.CNN_HIDDEN}, num_actions = {_lib.CNN_ACTIONS} and kitchens of at least 3 x 3")
        return count

    def desc(self):
        return _lib.CnnBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.hidden, 0)


def _cnn_bank_call_args(sim, bank, ids, players, record):
    if not isinstance(bank, CnnPolicyBank):
        raise ValueError("bank must be a CnnPolicyBank")
    bank._check_params(sim.gpu_id)
    mask = _cnn_call_args(sim, bank.policy(0), players, record)
    shape = tuple(sim.observation_world_major_tensor().shape[:2])
    _check_ids(sim, ids, shape, "ids")
    return mask


def _check_ids(sim, tensor, shape, name):
    if (not isinstance(tensor, torch.Tensor) or not tensor.is_cuda or tensor.device.index != sim.gpu_id or tensor.dtype != torch.int32 or
            tuple(tensor.shape) != tuple(shape) or not tensor.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous int32 tensor of shape {tuple(shape)} on cuda:{sim.gpu_id}")


def _bank_workspace(sim, attribute, size):
    """the plan's workspace a MAPPO bank act takes by default: one the simulator keeps as ``attribute``, of at least ``size`` bytes"""
    workspace = getattr(sim, attribute, None)
    if workspace is None or workspace.numel() < size:
        workspace = torch.empty(int(size), dtype=torch.uint8, device=torch.device("cuda", sim.gpu_id))
        setattr(sim, attribute, workspace)
    return workspace


def _cnn_bank_workspace(sim, bank):
    seats = sim.observation_world_major_tensor().shape[1]
    return _bank_workspace(sim, "_cnn_bank_workspace", sim._L.mrl_cnn_bank_workspace_bytes(sim.num_worlds, seats, bank.num_policies))


def cnn_act_bank(sim, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False, value_only=False,
                 workspace=None):
    """``mrl_cnn_act_bank`` on torch's current stream: seat p of world n acts under row ``ids[n, p]`` of ``bank`` (a
    ``CnnPolicyBank``) where p is in ``players`` and the id is valid; a cell at -1 keeps its ACTION entry and its record cells.
    The plan, which sorts the cells by policy into tiles of one policy each (one launch up to 2048 cells, three beyond), then
    ``cnn_act``'s kernel body over those tiles: every output is bit for bit ``cnn_act``'s under the cell's policy.  ``ids``: int32 (N, P) on the device;
    ``ids_row``: int32 (N, P) that receives the ids as this act used them (-1 where it did not act).  The other arguments are
    ``cnn_act``'s.  ``workspace``: default one the simulator keeps (``mrl_cnn_bank_workspace_bytes``; its words are in
    include/mrl_envs.h)."""
    mask = _cnn_bank_call_args(sim, bank, ids, players, record)
    if ids_row is not None:
        _check_ids(sim, ids_row, ids.shape, "ids_row")
    if workspace is None:
        workspace = _cnn_bank_workspace(sim, bank)
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.CNN_VALUE_ONLY if value_only else 0)
    desc = bank.desc()
    rc = sim._L.mrl_cnn_act_bank(sim._handle, mask, ctypes.byref(desc), ids.data_ptr(), ctypes.byref(record.struct) if record is not None else None,
                                 ids_row.data_ptr() if ids_row is not None else None, int(row), int(seed) & (2 ** 64 - 1),
                                 int(step) & 0xFFFFFFFF, flags, workspace.data_ptr(), workspace.numel(), _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


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


def cnn_resample(sim, ids, episodes, mode, first_id, num_ids, players=None, seed=0):
    """``mrl_cnn_bank_resample`` on torch's current stream: where DONE[n] != 0 -- the world has just restarted itself --
    ``episodes[n]`` goes up by one and every seat p of ``players`` with ``ids[n, p] >= 0`` takes its next policy from
    ``[first_id[p], first_id[p] + num_ids[p])``: "robin" the next one round the range, "random" by ``random_hash(seed, episodes[n],
    n, p)`` (``resample_twin`` is the same in numpy).  ``mode`` may also be a ``CnnResample``, which then carries the rest."""
    if not isinstance(sim, OvercookedSimulator):  # (a SimplecookedSimulator is one)
        raise ValueError(f"mrl_cnn_bank_resample runs on an OvercookedSimulator or a SimplecookedSimulator, not on a {type(sim).__name__}")
    worlds, seats = sim.observation_world_major_tensor().shape[:2]
    _bank_resample(sim, "mrl_cnn_bank_resample", worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed)


CrossPlayResult = collections.namedtuple("CrossPlayResult", "mean_return episodes")  # each (Ka, Kb), on the device


def cross_play(env, bank, members_a=None, members_b=None, greedy=True, seed=0, steps=None):
    """The cross-play matrix of ``bank``'s members on one batch of worlds: world n plays pair n mod (Ka Kb), seat 0 under
    ``members_a[pair // Kb]`` and seat 1 under ``members_b[pair % Kb]`` (default every row of the bank).  All worlds are restarted, one
    horizon of (``cnn_act_bank``, step) follows, no host wait inside, and the last-episode return
    of ``enable_episode_stats`` (the team's, as seat 0 received it) is averaged per pair.  ``env``: a two-player kitchen env
    wrapper on the GPU.  Returns ``CrossPlayResult(mean_return, episodes)``, float64 and int64 (Ka, Kb) on the device;
    ``episodes`` is the number of worlds that played the pair.

    With an ``MlpBasePolicyBank`` ``env`` is a ``BalanceMadronaTorch`` on the GPU and ``steps`` (default 12, four times the beam's TIME of
    three: six episodes where nobody leaves the line) times (``mlpbase_act_bank``, step) follow the restart.  The beam's episodes have no fixed length, so every episode a
    world finishes within ``steps`` counts: behind each step the last-episode return of the worlds whose DONE is set is added to
    per-world float64 sums and counts (elementwise, no host wait), which are reduced per pair at the end -- the returns are
    float32, so the sums are exact whatever the order.  ``episodes`` is then the number of finished episodes per pair.

    With a ``WidePolicyBank`` ``env`` is a ``HanabiMadrona`` or a ``BalanceMadronaTorch`` on the GPU and a step is
    ``agent_act_bank`` for seat 0, the same for seat 1, then the simulator's step; the episodes are counted as on the beam.  A game
    of Hanabi has no length to derive a default from: ``steps`` must be given there (on the beam it defaults to 12).  The kitchens
    play one horizon and take no ``steps``."""
    if isinstance(bank, MlpBasePolicyBank):
        return _cross_play_beam(env, bank, members_a, members_b, greedy, seed, steps)
    if isinstance(bank, WidePolicyBank):
        return _cross_play_wide(env, bank, members_a, members_b, greedy, seed, steps)
    if steps is not None:
        raise ValueError("steps is the balance beam's: a kitchen's cross-play lasts one horizon")
    sim = env.sim
    n, p = tuple(sim.observation_world_major_tensor().shape[:2])
    ka, kb, pair, ids = _cross_play_pairs(sim, bank, members_a, members_b, n, p)
    sim.enable_episode_stats()
    sim.reset_worlds(None)
    for t in range(int(env.horizon)):
        cnn_act_bank(sim, bank, ids, seed=seed, step=t, greedy=greedy)
        sim.step()
    last = sim.last_episode_return_tensor().to_torch().reshape(p, n)[0].to(torch.float64)
    return _cross_play_result(ka, kb, pair, last, torch.ones_like(pair))


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


class _MlpLayer(torch.nn.Module):
    """train/MAPPO/utils/mlp.py:6-27 for use_ReLU and use_orthogonal: ``fc1``, ``fc_h`` and ``fc2``, ``layer_N`` deep copies of
    ``fc_h`` taken at construction.  ``forward`` never uses ``fc_h`` itself -- as in the reference, whose state dicts carry it."""

    def __init__(self, obs_dim, hidden, layer_N):
        super().__init__()
        nn = torch.nn
        gain = nn.init.calculate_gain("relu")

        def linear(inputs, outputs):
            layer = nn.Linear(inputs, outputs)
            nn.init.orthogonal_(layer.weight.data, gain=gain)
            nn.init.constant_(layer.bias.data, 0.0)
            return layer

        self._layer_N = int(layer_N)
        self.fc1 = nn.Sequential(linear(obs_dim, hidden), nn.ReLU(), nn.LayerNorm(hidden))
        self.fc_h = nn.Sequential(linear(hidden, hidden), nn.ReLU(), nn.LayerNorm(hidden))
        self.fc2 = nn.ModuleList([copy.deepcopy(self.fc_h) for _ in range(self._layer_N)])

    def forward(self, x):
        x = self.fc1(x)
        for i in range(self._layer_N):
            x = self.fc2[i](x)
        return x


class _MlpBase(torch.nn.Module):
    """``MLPBase`` with ``use_feature_normalization`` (mlp.py:31-58)"""

    def __init__(self, obs_dim, hidden, layer_N):
        super().__init__()
        self.feature_norm = torch.nn.LayerNorm(obs_dim)
        self.mlp = _MlpLayer(obs_dim, hidden, layer_N)

    def forward(self, x):
        return self.mlp(self.feature_norm(x))


class _MlpBaseActor(torch.nn.Module):
    """``R_Actor``'s parameters by name for a vector observation, non-recurrent: ``base.feature_norm``, ``base.mlp.fc1/fc_h/fc2``,
    ``act.action_out.linear``"""

    def __init__(self, obs_dim, hidden, layer_N, num_actions):
        super().__init__()
        self.base = _MlpBase(obs_dim, hidden, layer_N)
        self.act = _ActLayer(hidden, num_actions)

    def forward(self, obs):
        return self.act.action_out.linear(self.base(obs))


class _MlpBaseCritic(torch.nn.Module):
    """``R_Critic``'s parameters by name without PopArt: ``base...``, ``v_out``"""

    def __init__(self, obs_dim, hidden, layer_N):
        super().__init__()
        self.base = _MlpBase(obs_dim, hidden, layer_N)
        self.v_out = torch.nn.Linear(hidden, 1)

    def forward(self, state):
        return self.v_out(self.base(state))


class MlpBaseActorCritic(torch.nn.Module):
    """MAPPO's MLP actor-critic for the balance beam (train/MAPPO/utils/mlp.py, r_actor_critic.py, utils/distributions.py:55-68;
    ``use_feature_normalization``, ``use_ReLU`` and ``use_orthogonal`` at their defaults, non-recurrent, no PopArt): ``actor`` and
    ``critic`` take the (n, 7) observation as floats.  Their state dicts have the reference's keys -- ``base.mlp.fc_h`` included,
    which the reference registers and never uses --, so ``actor.load_state_dict`` / ``critic.load_state_dict`` take a reference
    checkpoint's ``actor.pt`` / ``critic.pt``.  Initialisation is the reference's: orthogonal weights with the ReLU gain, 0.01 for
    the action head (``args.gain``), 1 for ``v_out``, zero biases, LayerNorm at (1, 0).  The device path runs ``hidden`` 64 and
    ``layer_N`` 1 or 2."""

    def __init__(self, obs_dim=_lib.MLPBASE_OBS, num_actions=_lib.MLPBASE_ACTIONS, hidden=_lib.MLPBASE_HIDDEN, layer_N=2):
        super().__init__()
        self.obs_dim, self.num_actions, self.hidden, self.layer_N = int(obs_dim), int(num_actions), int(hidden), int(layer_N)
        self.actor = _MlpBaseActor(self.obs_dim, self.hidden, self.layer_N, self.num_actions)
        self.critic = _MlpBaseCritic(self.obs_dim, self.hidden, self.layer_N)
        for head, head_gain in ((self.actor.act.action_out.linear, 0.01), (self.critic.v_out, 1.0)):
            torch.nn.init.orthogonal_(head.weight, gain=head_gain)
            torch.nn.init.constant_(head.bias, 0.0)

    def get_value(self, state):
        return self.critic(state)

    def get_action_and_value(self, obs, action=None, deterministic=False):
        dist = torch.distributions.Categorical(logits=self.actor(obs))
        if action is None:
            action = dist.probs.argmax(dim=-1) if deterministic else dist.sample()
        return action, dist.log_prob(action), dist.entropy(), self.critic(obs)


class MlpBasePolicy(_FlatPolicy):
    """The parameters ``mrl_mlpbase_act`` runs on a balance-beam simulator: one flat float32 tensor ``params``, the actor's tensors
    and then the critic's in the order of ``parameters_to_vector(MlpBaseActorCritic.parameters())`` (``mrl_mlpbase_policy``; the
    unused ``fc_h`` is part of it and is never read or changed by a kernel).  ``module()`` returns an ``MlpBaseActorCritic`` whose
    parameters are VIEWS into ``params``: an in-place step on either side is what the other reads next (there is no ``load_``)."""

    _module_class, _module_name, _shape = MlpBaseActorCritic, "an MlpBaseActorCritic", ("obs_dim", "num_actions", "hidden", "layer_N")

    def __init__(self, obs_dim=_lib.MLPBASE_OBS, num_actions=_lib.MLPBASE_ACTIONS, hidden=_lib.MLPBASE_HIDDEN, layer_N=2, device="cuda:0"):
        self.obs_dim, self.num_actions, self.hidden, self.layer_N = int(obs_dim), int(num_actions), int(hidden), int(layer_N)
        self._allocate(device, f"mrl_mlpbase_act runs obs_dim = {_lib.MLPBASE_OBS}, num_actions = {_lib.MLPBASE_ACTIONS}, hidden = "
                               f"{_lib.MLPBASE_HIDDEN} and layer_N 1 or 2; got {self.obs_dim}, {self.num_actions}, {self.hidden}, {self.layer_N}")

    @property
    def num_params(self):
        return int(_lib.lib().mrl_mlpbase_policy_num_params(self.obs_dim, self.hidden, self.layer_N, self.num_actions))

    def desc(self):
        return _lib.MlpBasePolicyDesc(self.params.data_ptr(), self.hidden, self.layer_N, 0)

    # what MappoOptimizer and mappo_update ask of a policy
    def _mappo_workspace_bytes(self, minibatch_size, num_minibatches, out, members=None):
        """``members``: for that many members of a bank in one ``mappo_update_bank``"""
        shape = (self.obs_dim, self.hidden, self.layer_N, self.num_actions, minibatch_size, num_minibatches)
        if members is None:
            return _lib.lib().mrl_mappo_mlp_workspace_bytes(*shape, out)
        return _lib.lib().mrl_mappo_mlp_bank_workspace_bytes(*shape, members, out)

    def _mappo_check(self, record, ring):
        if not isinstance(record, MlpBaseRecord):
            raise ValueError("record must be an MlpBaseRecord")
        if ring is not None:
            raise ValueError("an MlpBasePolicy's batch is record.obs: ring must be None")

    def _mappo_batch(self, record, ring, count):
        """-> ((entry point, the bank's), policy struct, batch struct's type, the batch's observations): the record's ``obs``"""
        rows = count + count // max(record.num_steps, 1)
        _require_tensors([("record.obs", record.obs, torch.int32, rows * self.obs_dim)], self.params.device)
        return (_lib.lib().mrl_mappo_mlp_update, _lib.lib().mrl_mappo_mlp_bank_update), self.desc(), _lib.MappoMlpBatch, record.obs


class MlpBaseRecord(_MappoRecord):
    """The buffers of ``mrl_mlpbase_act`` / ``mrl_rollout_mlpbase`` (``mrl_mlpbase_record``): ``CnnRecord``'s arrays and row
    convention (``logits`` (T, N, P, 4) on request) and ``obs`` int32 (T + 1, N, P, 7), row k what the act at row k read."""

    _struct, _buffers, _actions = _lib.MlpBaseRecordDesc, _lib.MLPBASE_RECORD_BUFFERS, _lib.MLPBASE_ACTIONS

    def _own_buffers(self, z, t, n, p):
        self.obs = z((t + 1, n, p, _lib.MLPBASE_OBS), torch.int32)


def _mlpbase_call_args(sim, policy, players, record):
    if not isinstance(policy, MlpBasePolicy):
        raise ValueError("policy must be an MlpBasePolicy")
    if not isinstance(sim, BalanceBeamSimulator):
        raise ValueError("mrl_mlpbase_act runs on a BalanceBeamSimulator")
    p = policy._check_params(sim.gpu_id)
    seats, worlds = sim.observation_tensor().shape[:2]  # (P, N, 7)
    if record is not None and (not isinstance(record, MlpBaseRecord) or record.num_worlds != worlds or record.num_players != seats or
                               record.actions.device != p.device):
        raise ValueError(f"record must be an MlpBaseRecord of {worlds} worlds and {seats} players on cuda:{sim.gpu_id}")
    return _seat_mask(players, seats)


def mlpbase_act(sim, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False, value_only=False):
    """``mrl_mlpbase_act`` on torch's current stream of the simulator's device: the seats in ``players`` (a bit mask or an iterable
    of seats; default both) of a balance-beam simulator act under ``policy`` (an ``MlpBasePolicy``) on the simulator's own
    OBSERVATION tensor; with ``record`` (an ``MlpBaseRecord``) row ``row`` of its buffers is written, the observation rows
    included.  ``value_only``: the closing act at row T."""
    mask = _mlpbase_call_args(sim, policy, players, record)
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.MLPBASE_VALUE_ONLY if value_only else 0)
    desc = policy.desc()
    rc = sim._L.mrl_mlpbase_act(sim._handle, mask, ctypes.byref(desc), ctypes.byref(record.struct) if record is not None else None,
                                int(row), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, flags, _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


class MlpBasePolicyBank(_PolicyBank):
    """K ``MlpBasePolicy`` of one shape in one dense float32 tensor ``params`` (K, num_params) (``mrl_mlpbase_bank``), the
    counterpart of ``CnnPolicyBank`` for the balance beam: row k is exactly what an ``MlpBasePolicy``'s ``params`` is.
    ``policy(k)`` is an ``MlpBasePolicy`` whose ``params`` IS row k, a contiguous view, so ``mlpbase_act``, ``MappoOptimizer``,
    ``mappo_update`` and ``.module()`` work on a member unchanged and training a member is what the next ``mlpbase_act_bank``
    reads.  1 <= K <= 256; one ``layer_N`` for the whole bank."""

    _member_class, _shape = MlpBasePolicy, MlpBasePolicy._shape

    def __init__(self, num_policies, layer_N=2, obs_dim=_lib.MLPBASE_OBS, num_actions=_lib.MLPBASE_ACTIONS, hidden=_lib.MLPBASE_HIDDEN,
                 device="cuda:0"):
        self.obs_dim, self.num_actions, self.hidden, self.layer_N = int(obs_dim), int(num_actions), int(hidden), int(layer_N)
        super().__init__(num_policies, device)

    def _count_params(self):
        count = int(_lib.lib().mrl_mlpbase_policy_num_params(self.obs_dim, self.hidden, self.layer_N, self.num_actions))
        if count == 0:
            raise ValueError(f"mrl_mlpbase_act runs obs_dim = {_lib.MLPBASE_OBS}, num_actions = {_lib.MLPBASE_ACTIONS}, hidden = "
                             f"{_lib.MLPBASE_HIDDEN} and layer_N 1 or 2; got {self.obs_dim}, {self.num_actions}, {self.hidden}, {self.layer_N}")
        return count

    def desc(self):
        return _lib.MlpBaseBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.hidden, self.layer_N, 0)


def _mlpbase_bank_call_args(sim, bank, ids, players, record):
    if not isinstance(bank, MlpBasePolicyBank):
        raise ValueError("bank must be an MlpBasePolicyBank")
    if not isinstance(sim, BalanceBeamSimulator):
        raise ValueError("mrl_mlpbase_act_bank runs on a BalanceBeamSimulator")
    bank._check_params(sim.gpu_id)
    mask = _mlpbase_call_args(sim, bank.policy(0), players, record)
    seats, worlds = sim.observation_tensor().shape[:2]  # (P, N, 7)
    _check_ids(sim, ids, (worlds, seats), "ids")
    return mask


def _mlpbase_bank_workspace(sim, bank):
    return _bank_workspace(sim, "_mlpbase_bank_workspace", sim._L.mrl_mlpbase_bank_workspace_bytes(sim.num_worlds, bank.num_policies))


def mlpbase_act_bank(sim, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False, value_only=False,
                     workspace=None):
    """``mrl_mlpbase_act_bank`` on torch's current stream: seat p of world n of a balance-beam simulator acts under row
    ``ids[n, p]`` of ``bank`` (an ``MlpBasePolicyBank``) where p is in ``players`` and the id is valid; a cell at -1 keeps its
    ACTION entry and its record cells, ``record.obs`` included.  The plan (``cnn_act_bank``'s own), then ``mlpbase_act``'s kernel
    body over its tiles: every output is bit for bit ``mlpbase_act``'s under the cell's policy.  ``ids``: int32 (N, P) on the
    device; ``ids_row``: int32 (N, P) that receives the ids as this act used them (-1 where it did not act).  The other arguments
    are ``mlpbase_act``'s.  ``workspace``: default one the simulator keeps (``mrl_mlpbase_bank_workspace_bytes``, which is
    ``mrl_cnn_bank_workspace_bytes(N, 2, K)``; its words are in include/mrl_envs.h)."""
    mask = _mlpbase_bank_call_args(sim, bank, ids, players, record)
    if ids_row is not None:
        _check_ids(sim, ids_row, ids.shape, "ids_row")
    if workspace is None:
        workspace = _mlpbase_bank_workspace(sim, bank)
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.MLPBASE_VALUE_ONLY if value_only else 0)
    desc = bank.desc()
    rc = sim._L.mrl_mlpbase_act_bank(sim._handle, mask, ctypes.byref(desc), ids.data_ptr(),
                                     ctypes.byref(record.struct) if record is not None else None,
                                     ids_row.data_ptr() if ids_row is not None else None, int(row), int(seed) & (2 ** 64 - 1),
                                     int(step) & 0xFFFFFFFF, flags, workspace.data_ptr(), workspace.numel(), _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


BankResample = CnnResample  # the descriptor serves both networks' banks


def mlpbase_resample(sim, ids, episodes, mode, first_id=None, num_ids=None, players=None, seed=0):
    """``mrl_mlpbase_bank_resample`` on torch's current stream: ``cnn_resample`` on a balance-beam simulator -- the same kernel,
    draws and arguments (``resample_twin`` is the same in numpy).  ``mode`` may also be a ``CnnResample`` (``BankResample``), which
    then carries the rest."""
    if not isinstance(sim, BalanceBeamSimulator):
        raise ValueError("mrl_mlpbase_bank_resample runs on a BalanceBeamSimulator")
    seats, worlds = sim.observation_tensor().shape[:2]
    _bank_resample(sim, "mrl_mlpbase_bank_resample", worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed)


BEAM_TIME = 3  # src/balance_beam_env/sim.cpp: an observation holds TIME positions per seat, an episode is at most TIME - 1 moves


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


def _cross_play_beam(env, bank, members_a, members_b, greedy, seed, steps):
    """``cross_play`` for an ``MlpBasePolicyBank`` on the balance beam"""
    sim = env.sim
    if not isinstance(sim, BalanceBeamSimulator):
        raise ValueError("an MlpBasePolicyBank plays on the balance beam: env.sim must be a BalanceBeamSimulator")
    return _cross_play_counted(sim, bank, members_a, members_b, 4 * BEAM_TIME if steps is None else steps,
                               lambda ids, t: mlpbase_act_bank(sim, bank, ids, seed=seed, step=t, greedy=greedy))


def _cross_play_wide(env, bank, members_a, members_b, greedy, seed, steps):
    """``cross_play`` for a ``WidePolicyBank`` on Hanabi or the balance beam"""
    sim = getattr(env, "sim", None)
    if not isinstance(sim, (HanabiSimulator, BalanceBeamSimulator)):
        raise ValueError("a WidePolicyBank plays Hanabi or the balance beam: env.sim must be a HanabiSimulator or a BalanceBeamSimulator, "
                         f"got {type(sim).__name__}")
    if steps is None:
        if isinstance(sim, HanabiSimulator):
            raise ValueError("steps has no default for Hanabi: a game has no fixed length; give the number of steps to play")
        steps = 4 * BEAM_TIME

    def act(ids, t):
        agent_act_bank(sim, 0, bank, ids, seed=seed, step=t, greedy=greedy)
        agent_act_bank(sim, 1, bank, ids, seed=seed, step=t, greedy=greedy)

    return _cross_play_counted(sim, bank, members_a, members_b, steps, act)


def _wide_mlp(inputs, outputs, hidden=_lib.WIDE_HIDDEN):
    nn = torch.nn
    return nn.Sequential(nn.Linear(inputs, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(), nn.Linear(hidden, hidden), nn.ReLU(),
                         nn.Linear(hidden, outputs))


class WideAgent(torch.nn.Module):
    """The actor-critic of the reference's ``CleanPPOAgent`` by shape and method names (pantheonrl_extension/vectoragent.py:66-113,
    ``CleanRLNetwork``): critic from the S-wide state to one value, actor from the D-wide observation to A logits, three hidden
    ReLU layers of width 512 each.  ``orthogonal=True`` initialises like the reference (orthogonal weights of gain sqrt 2, 0.01
    for the two output layers, zero biases); otherwise torch's default."""

    def __init__(self, obs_dim, state_dim, num_actions, orthogonal=False):
        super().__init__()
        self.critic = _wide_mlp(state_dim, 1)
        self.actor = _wide_mlp(obs_dim, num_actions)
        if orthogonal:
            for net in (self.critic, self.actor):
                for i in (0, 2, 4, 6):
                    torch.nn.init.orthogonal_(net[i].weight, 0.01 if i == 6 else 2.0 ** 0.5)
                    torch.nn.init.constant_(net[i].bias, 0.0)

    def get_value(self, x):
        return self.critic(x)

    def get_action_and_value(self, x, state, action_mask, action=None):
        logits = self.actor(x).masked_fill(torch.logical_not(action_mask), -float("inf"))
        dist = torch.distributions.Categorical(logits=logits)
        if action is None:
            action = dist.sample()
        return action, dist.log_prob(action), dist.entropy(), self.critic(state)


class WidePolicy:
    """The parameters ``mrl_agent_act`` runs: one flat float32 tensor ``params`` in the order of
    ``parameters_to_vector(agent.parameters())`` for a ``WideAgent`` (``mrl_wide_policy``).  ``module()`` returns a ``WideAgent``
    whose parameters are VIEWS into ``params``: a torch optimizer's in-place step on them is what the kernels read next, with no
    copy in between (so there is no ``load_``)."""

    def __init__(self, obs_dim, state_dim, num_actions, device="cuda:0"):
        self.obs_dim, self.state_dim, self.num_actions = int(obs_dim), int(state_dim), int(num_actions)
        if not 1 <= self.num_actions <= _lib.WIDE_MAX_ACTIONS or self.obs_dim < 1 or self.state_dim < 1:
            raise ValueError(f"need 1 <= num_actions <= {_lib.WIDE_MAX_ACTIONS} and obs_dim, state_dim >= 1")
        self.params = torch.zeros(self.num_params, dtype=torch.float32, device=torch.device(device))
        self._module = None

    @property
    def num_params(self):
        return int(_lib.lib().mrl_wide_policy_num_params(self.obs_dim, self.state_dim, self.num_actions))

    @staticmethod
    def _shape_of(agent):
        """(obs_dim, state_dim, num_actions) of an agent of the expected form; ValueError otherwise."""
        nn, h = torch.nn, _lib.WIDE_HIDDEN
        for name in ("critic", "actor"):
            net = getattr(agent, name, None)
            if (not isinstance(net, nn.Sequential) or len(net) != 7 or not all(isinstance(net[i], nn.Linear) for i in (0, 2, 4, 6)) or
                    not all(isinstance(net[i], nn.ReLU) for i in (1, 3, 5)) or any(net[i].bias is None for i in (0, 2, 4, 6))):
                raise ValueError(f"agent.{name} must be Sequential(Linear, ReLU, Linear, ReLU, Linear, ReLU, Linear) with biases")
            shapes = [(net[i].in_features, net[i].out_features) for i in (0, 2, 4, 6)]
            if shapes != [(shapes[0][0], h), (h, h), (h, h), (h, shapes[3][1])]:
                raise ValueError(f"agent.{name}'s layers are {shapes}; the hidden width must be {h}")
        if agent.critic[6].out_features != 1:
            raise ValueError("agent.critic must end in one value")
        return agent.actor[0].in_features, agent.critic[0].in_features, agent.actor[6].out_features

    @classmethod
    def from_module(cls, agent, device=None):
        """A policy of ``agent``'s shape holding a copy of its parameters (``device``: default the agent's own)."""
        d, s, a = cls._shape_of(agent)
        policy = cls(d, s, a, device if device is not None else agent.critic[0].weight.device)
        with torch.no_grad():
            policy.params.copy_(torch.cat([p.detach().reshape(-1) for net in (agent.critic, agent.actor) for p in net.parameters()]))
        return policy

    def module(self):
        """The ``WideAgent`` whose parameters alias ``params`` (one object per policy)."""
        if self._module is None:
            agent = WideAgent(self.obs_dim, self.state_dim, self.num_actions)
            at = 0
            for p in agent.parameters():  # critic first, then actor: the order of the flat array
                p.data = self.params[at:at + p.numel()].view(p.shape)
                at += p.numel()
            assert at == self.params.numel()
            self._module = agent
        return self._module

    def desc(self):
        return _lib.WidePolicyDesc(self.params.data_ptr(), self.obs_dim, self.state_dim, self.num_actions)


class AgentRecord:
    """The buffers of one ``CleanPPOAgent`` (``mrl_agent_record``): torch tensors by name plus the ctypes struct over them."""

    def __init__(self, num_steps, num_worlds, obs_dim, state_dim, num_actions, obs_dtype, state_dtype, device, logits=False):
        t, n = int(num_steps), int(num_worlds)
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=device)  # noqa: E731
        self.num_steps, self.num_worlds = t, n
        self.obs, self.states = z((t, n, obs_dim), obs_dtype), z((t, n, state_dim), state_dtype)
        self.action_masks, self.active = z((t, n, num_actions), torch.uint8), z((t, n), torch.uint8)
        self.actions = z((t, n), torch.int32)
        self.logprobs, self.values, self.dones, self.rewards = (z((t, n), torch.float32) for _ in range(4))
        self.last_active = z((n,), torch.int32)
        self.new_game, self.next_done = z((n,), torch.uint8), z((n,), torch.uint8)
        self.running_rewards = z((n,), torch.float32)
        self.totals = z(((n + 1023) // 1024, 4), torch.float64)
        self.next_value, self.next_active = z((n,), torch.float32), z((n,), torch.uint8)
        self.first_step = z((1,), torch.int32)
        self.logits = z((n, _lib.WIDE_MAX_ACTIONS), torch.float32) if logits else None
        self.advantages, self.returns = z((t, n), torch.float32), z((t, n), torch.float32)
        self.workspace = torch.empty(int(_lib.lib().mrl_agent_workspace_bytes(n)) if device.type == "cuda" else 0, dtype=torch.uint8,
                                     device=device)
        self.clear_totals()
        self.struct = _lib.AgentRecord(*[getattr(self, name).data_ptr() if getattr(self, name) is not None else None
                                         for name in _lib.AGENT_RECORD_BUFFERS], t, n)

    def clear_totals(self):
        self.totals[:, 0:2] = 0.0
        self.totals[:, 2] = float("inf")
        self.totals[:, 3] = -float("inf")

    def episode_totals(self):
        """(finished episodes, sum of their returns, minimum, maximum) since the last ``clear_totals`` -- one host read."""
        t = self.totals.cpu()
        return int(t[:, 0].sum()), float(t[:, 1].sum()), float(t[:, 2].min()), float(t[:, 3].max())


def agent_act(sim, player, policy, record=None, row=0, seed=0, step=0, greedy=False, all_rows=False, value_only=False, workspace=None):
    """``mrl_agent_act`` on torch's current stream of the simulator's device: player ``player`` of a Hanabi or balance-beam
    simulator acts under ``policy`` (a ``WidePolicy``) on the simulator's tensors as they stand; with ``record`` (an
    ``AgentRecord``) row ``row`` of its buffers is written.  ``workspace``: default the record's."""
    if not isinstance(policy, WidePolicy):
        raise ValueError("policy must be a WidePolicy")
    p = policy.params
    if not p.is_cuda or p.device.index != sim.gpu_id or p.dtype != torch.float32 or not p.is_contiguous() or p.numel() != policy.num_params:
        raise ValueError(f"policy.params must be a contiguous float32 tensor of num_params elements on cuda:{sim.gpu_id}")
    if workspace is None:
        if record is None:
            raise ValueError("give a workspace (uint8, mrl_agent_workspace_bytes) or a record")
        workspace = record.workspace
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.AGENT_ALL_ROWS if all_rows else 0) | (_lib.AGENT_VALUE_ONLY if value_only else 0)
    desc = policy.desc()
    rc = sim._L.mrl_agent_act(sim._handle, int(player), ctypes.byref(desc), ctypes.byref(record.struct) if record is not None else None,
                              int(row), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, flags, workspace.data_ptr(),
                              _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


class WidePolicyBank(_PolicyBank):
    """K ``WidePolicy`` of one shape in one dense float32 tensor ``params`` (K, num_params) (``mrl_wide_bank``), the counterpart of
    ``CnnPolicyBank`` and ``MlpBasePolicyBank`` for Hanabi and the balance beam: row k is exactly what a ``WidePolicy``'s ``params``
    is.  ``policy(k)`` is a ``WidePolicy`` whose ``params`` IS row k, a contiguous view, so ``agent_act``, ``WideOptimizer`` /
    ``agent_update``, ``.module()`` and a torch optimizer work on a member unchanged, and training a member is what the next
    ``agent_act_bank`` reads.  1 <= K <= 256."""

    _member_class, _shape = WidePolicy, ("obs_dim", "state_dim", "num_actions")

    def __init__(self, obs_dim, state_dim, num_actions, num_policies, device="cuda:0"):
        self.obs_dim, self.state_dim, self.num_actions = int(obs_dim), int(state_dim), int(num_actions)
        super().__init__(num_policies, device)

    def _count_params(self):
        if not 1 <= self.num_actions <= _lib.WIDE_MAX_ACTIONS or self.obs_dim < 1 or self.state_dim < 1:
            raise ValueError(f"need 1 <= num_actions <= {_lib.WIDE_MAX_ACTIONS} and obs_dim, state_dim >= 1")
        return int(_lib.lib().mrl_wide_policy_num_params(self.obs_dim, self.state_dim, self.num_actions))

    def desc(self):
        return _lib.WideBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.obs_dim, self.state_dim,
                                 self.num_actions)


def _wide_seats(sim, what):
    """(seats, worlds) of a Hanabi or balance-beam simulator; any other is refused"""
    if not isinstance(sim, (HanabiSimulator, BalanceBeamSimulator)):
        raise ValueError(f"{what} runs on a HanabiSimulator or a BalanceBeamSimulator, not on a {type(sim).__name__}")
    return tuple(sim.observation_tensor().shape[:2])


def agent_bank_workspace_bytes(num_worlds, num_policies):
    """``mrl_agent_bank_workspace_bytes``"""
    out = ctypes.c_uint64(0)
    _lib.check(_lib.lib().mrl_agent_bank_workspace_bytes(int(num_worlds), int(num_policies), ctypes.byref(out)))
    return int(out.value)


def _wide_bank_workspace(sim, bank):
    """The default workspace of ``agent_act_bank``, one per (simulator, bank): the act itself does not need that -- a call rewrites
    everything it reads of the workspace -- but two banks that act on one simulator from two streams (a population per seat) then
    never share a buffer, which one workspace per simulator, as the MAPPO banks keep it, would make them do."""
    size = agent_bank_workspace_bytes(sim.num_worlds, bank.num_policies)
    cache = sim.__dict__.setdefault("_wide_bank_workspaces", {})
    workspace = cache.get(id(bank))
    if workspace is None or workspace[0] is not bank or workspace[1].numel() < size:
        workspace = cache[id(bank)] = (bank, torch.empty(size, dtype=torch.uint8, device=torch.device("cuda", sim.gpu_id)))
    return workspace[1]


def agent_act_bank(sim, player, bank, ids, ids_row=None, seed=0, step=0, greedy=False, all_rows=False, workspace=None):
    """``mrl_agent_act_bank`` on torch's current stream: seat ``player`` of world n of a Hanabi or balance-beam simulator acts under
    row ``ids[n, player]`` of ``bank`` (a ``WidePolicyBank``) where the world is computed -- where it is ``player``'s turn, or
    everywhere with ``all_rows`` -- and gets action 0 where it is not, as ``agent_act`` writes it; a world at -1 keeps its ACTION
    entry.  The effective ids, the plan (``cnn_act_bank``'s own, over one seat), ``agent_act``'s layer kernel over the plan's tiles
    and its head: every world's logits, value and action are bit for bit ``agent_act``'s under the world's policy.  There is no
    record: a learner trains ``bank.policy(k)`` through ``agent_act``.  ``ids``: int32 (N, P) on the device; ``ids_row``: int32 (N)
    that receives k where the world acted under row k and -1 where it has a valid id and is not computed.  ``workspace``: default
    one the simulator keeps per bank (``mrl_agent_bank_workspace_bytes``; its layout is in include/mrl_envs.h)."""
    if not isinstance(bank, WidePolicyBank):
        raise ValueError("bank must be a WidePolicyBank")
    seats, worlds = _wide_seats(sim, "mrl_agent_act_bank")
    bank._check_params(sim.gpu_id)
    _check_ids(sim, ids, (worlds, seats), "ids")
    if ids_row is not None:
        _check_ids(sim, ids_row, (worlds,), "ids_row")
    if workspace is None:
        workspace = _wide_bank_workspace(sim, bank)
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (_lib.AGENT_ALL_ROWS if all_rows else 0)
    desc = bank.desc()
    rc = sim._L.mrl_agent_act_bank(sim._handle, int(player), ctypes.byref(desc), ids.data_ptr(),
                                   ids_row.data_ptr() if ids_row is not None else None, int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF,
                                   flags, workspace.data_ptr(), workspace.numel(), _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


def wide_resample(sim, ids, episodes, mode, first_id=None, num_ids=None, players=None, seed=0):
    """``mrl_agent_bank_resample`` on torch's current stream: ``cnn_resample`` on a Hanabi or balance-beam simulator -- the same
    kernel, draws and arguments (``resample_twin`` is the same in numpy).  ``mode`` may also be a ``CnnResample``
    (``BankResample``), which then carries the rest."""
    seats, worlds = _wide_seats(sim, "mrl_agent_bank_resample")
    _bank_resample(sim, "mrl_agent_bank_resample", worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed)


def agent_credit(record, rewards, dones):
    """``mrl_agent_credit``: ``rewards`` float32 (N), ``dones`` int32 (N), contiguous, on the record's GPU."""
    device = record.rewards.device
    for t, dtype in ((rewards, torch.float32), (dones, torch.int32)):
        if t.device != device or t.dtype != dtype or not t.is_contiguous() or t.numel() != record.num_worlds:
            raise ValueError("rewards / dones must be contiguous float32 / int32 tensors of num_worlds elements on the record's GPU")
    rc = _lib.lib().mrl_agent_credit(ctypes.byref(record.struct), rewards.data_ptr(), dones.data_ptr(), record.num_worlds, device.index,
                                     _stream_ptr(device.index))
    if rc:
        _lib.check(rc)


def gae_active(record, gamma, gae_lambda, next_value=None, next_active=None):
    """``mrl_gae_active`` over ``record``: fills and returns ``(record.advantages, record.returns)``; clears the ``active`` flag of the
    rows that only carried a bootstrap.  ``next_value`` / ``next_active``: default the record's own (a VALUE_ONLY act wrote them)."""
    nv = record.next_value if next_value is None else next_value
    na = record.next_active if next_active is None else next_active
    device = record.rewards.device
    if nv.dtype != torch.float32 or na.dtype != torch.uint8 or nv.device != device or na.device != device or \
            nv.numel() != record.num_worlds or na.numel() != record.num_worlds or not nv.is_contiguous() or not na.is_contiguous():
        raise ValueError("next_value / next_active must be contiguous float32 / uint8 tensors of num_worlds elements on the record's GPU")
    _lib.check(_lib.lib().mrl_gae_active(ctypes.byref(record.struct), nv.data_ptr(), na.data_ptr(), float(gamma), float(gae_lambda),
                                         record.advantages.data_ptr(), record.returns.data_ptr(), device.index,
                                         _stream_ptr(device.index)))
    return record.advantages, record.returns


# what ``rollout_policy`` fills, the names of scripts/cartpole_train_torch.py:179-192: (T, N, D), (T, N) x 5, (N, D), (N), (N)
Rollout = collections.namedtuple("Rollout", "obs actions logprobs values rewards dones next_obs next_value next_done")


def gae(rollout, gamma, gae_lambda):
    """``(advantages, returns)`` of a ``Rollout`` -- scripts/cartpole_train_torch.py:245-256 as one launch (``mrl_gae``), on
    torch's current stream of the rollout's device."""
    r = rollout
    num_steps, num_worlds = r.rewards.shape
    for t in (r.rewards, r.values, r.dones, r.next_value, r.next_done):
        if not t.is_cuda or t.device != r.rewards.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("rollout tensors must be contiguous float32 tensors on one GPU")
    if r.values.shape != r.rewards.shape or r.dones.shape != r.rewards.shape or r.next_value.numel() != num_worlds or \
            r.next_done.numel() != num_worlds:
        raise ValueError("rollout tensors must be (T, N), next_value and next_done (N)")
    advantages, returns = torch.empty_like(r.rewards), torch.empty_like(r.rewards)
    gpu = r.rewards.device.index
    _lib.check(_lib.lib().mrl_gae(r.rewards.data_ptr(), r.values.data_ptr(), r.dones.data_ptr(), r.next_value.data_ptr(),
                                  r.next_done.data_ptr(), num_steps, num_worlds, float(gamma), float(gae_lambda),
                                  advantages.data_ptr(), returns.data_ptr(), gpu, _stream_ptr(gpu)))
    return advantages, returns


class _AdamState:
    """What ``PpoOptimizer`` and ``MappoOptimizer`` share: ``exp_avg`` and ``exp_avg_sq`` over ``policy.params``, ``step``,
    ``betas``, ``eps`` and the cached scratch.  A subclass adds its learning rates and ``workspace_bytes``."""

    def __init__(self, policy, betas, eps):
        self.policy = policy
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.exp_avg = torch.zeros_like(policy.params)
        self.exp_avg_sq = torch.zeros_like(policy.params)
        self.step = 0
        self._workspace = None

    def workspace(self, minibatch_size, num_minibatches):
        """A uint8 tensor of at least ``workspace_bytes`` on the parameters' device: the cached one while it is large enough."""
        return self._cached_workspace(self.workspace_bytes(minibatch_size, num_minibatches))

    def _cached_workspace(self, need):
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != self.policy.params.device:
            self._workspace = torch.empty(need, dtype=torch.uint8, device=self.policy.params.device)
        return self._workspace


def _require_tensors(wanted, device):
    """``wanted``: (name, tensor, dtype, number of elements or None) each; raises unless every one is such a contiguous tensor on
    ``device``."""
    for name, tensor, dtype, numel in wanted:
        if (not isinstance(tensor, torch.Tensor) or tensor.device != device or tensor.dtype != dtype or not tensor.is_contiguous() or
                (numel is not None and tensor.numel() != numel)):
            raise ValueError(f"{name} must be a contiguous {dtype} tensor on {device}" + (f" of {numel} elements" if numel else ""))


def _run_update(entry, head, indices, middle, optimizer, columns, result, stats, grads):
    """The common end of ``ppo_update`` and ``mappo_update``: ``entry(*head, indices, rows, width, *middle, workspace, its bytes,
    stats, grads, gpu, stream)`` with the optimizer's scratch and fresh ``(rows, columns)`` / ``(rows, P)`` outputs where asked
    for; ``optimizer.step`` grows by the rows; returns ``result(stats, grads)``."""
    if indices.dim() != 2:
        raise ValueError("indices must be (rows, minibatch_size)")
    rows, width = indices.shape
    p = optimizer.policy.params
    workspace = optimizer.workspace(width, rows) if width else None
    out_stats = torch.empty((rows, columns), dtype=torch.float32, device=p.device) if stats else None
    out_grads = torch.empty((rows, p.numel()), dtype=torch.float32, device=p.device) if grads else None
    gpu = p.device.index
    _lib.check(entry(*head, indices.data_ptr(), rows, width, *middle, workspace.data_ptr() if workspace is not None else None,
                     workspace.numel() if workspace is not None else 0, out_stats.data_ptr() if stats else None,
                     out_grads.data_ptr() if grads else None, gpu, _stream_ptr(gpu)))
    optimizer.step += rows
    return result(out_stats, out_grads)


class PpoOptimizer(_AdamState):
    """Adam's state for ``ppo_update`` (``torch.optim.Adam(lr, betas, eps)`` without amsgrad or weight decay, as the reference's
    trainer builds it, scripts/cartpole_train_torch.py:176): ``exp_avg`` and ``exp_avg_sq`` on ``policy.params``' device, the
    number of steps taken (``step``) and the scratch ``mrl_ppo_update`` asks for, kept from call to call.  ``lr`` is an
    ordinary attribute: assign to it to anneal (:199-202)."""

    def __init__(self, policy, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(policy, MlpPolicy):
            raise ValueError("policy must be an MlpPolicy")
        super().__init__(policy, betas, eps)
        self.lr = float(lr)

    def workspace_bytes(self, minibatch_size, num_minibatches):
        """``mrl_ppo_workspace_bytes`` for this policy's shape."""
        p = self.policy
        out = ctypes.c_uint64(0)
        _lib.check(_lib.lib().mrl_ppo_workspace_bytes(p.obs_dim, p.hidden, p.num_actions, int(minibatch_size), int(num_minibatches),
                                                      ctypes.byref(out)))
        return int(out.value)


def minibatch_indices(batch_size, num_minibatches, epochs, generator=None, device="cpu"):
    """The rows ``ppo_update`` takes, (epochs * num_minibatches, batch_size // num_minibatches) int32 on ``device``: every epoch
    is one ``torch.randperm(batch_size)`` cut into ``num_minibatches`` rows (scripts/cartpole_train_torch.py:267-273).
    ``generator`` draws the permutations, on its own device."""
    batch_size, num_minibatches, epochs = int(batch_size), int(num_minibatches), int(epochs)
    if batch_size <= 0 or num_minibatches <= 0 or epochs < 0 or batch_size % num_minibatches:
        raise ValueError("batch_size must be a positive multiple of num_minibatches, epochs not negative")
    where = generator.device if generator is not None else torch.device(device)
    rows = [torch.randperm(batch_size, generator=generator, device=where).to(device=device, dtype=torch.int32)
            for _ in range(epochs)]
    width = batch_size // num_minibatches
    if not rows:
        return torch.empty((0, width), dtype=torch.int32, device=device)
    return torch.stack(rows).reshape(epochs * num_minibatches, width)


PpoResult = collections.namedtuple("PpoResult", "stats grads")  # (K, 8) in the order of ``_lib.PPO_STATS`` / (K, P), or None


def ppo_update(policy, optimizer, rollout, advantages, returns, indices, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5,
               max_grad_norm=0.5, norm_adv=True, clip_vloss=True, stats=True, grads=False):
    """One Adam step per row of ``indices`` on the PPO loss of scripts/cartpole_train_torch.py:275-315, on the device
    (``mrl_ppo_update``: three launches per row), enqueued on torch's current stream; it does not wait.  ``policy.params`` is
    updated in place -- the next ``rollout_policy`` reads it as it stands, there is no ``load_`` --, ``optimizer.step`` grows
    by the number of rows.  ``rollout`` is what ``rollout_policy`` returned (its obs, actions, logprobs and values, flattened
    to T * N samples), ``advantages`` and ``returns`` what ``gae`` returned, ``indices`` (K, B) int32 sample numbers
    (``minibatch_indices``).  Returns ``PpoResult(stats, grads)``: (K, 8) float32, columns ``_lib.PPO_STATS``, and (K, P) the
    unclipped gradients, each None unless asked for."""
    if not isinstance(policy, MlpPolicy) or not isinstance(optimizer, PpoOptimizer) or optimizer.policy is not policy:
        raise ValueError("policy must be an MlpPolicy and optimizer the PpoOptimizer made for it")
    p = policy.params
    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
        raise ValueError("policy.params must be a contiguous float32 tensor on a GPU")
    device, f32 = p.device, torch.float32
    count = rollout.values.numel()
    wanted = (("policy.params", p, f32, p.numel()), ("optimizer.exp_avg", optimizer.exp_avg, f32, p.numel()),
              ("optimizer.exp_avg_sq", optimizer.exp_avg_sq, f32, p.numel()), ("rollout.obs", rollout.obs, f32, count * policy.obs_dim),
              ("rollout.actions", rollout.actions, torch.int32, count), ("rollout.logprobs", rollout.logprobs, f32, count),
              ("rollout.values", rollout.values, f32, count), ("advantages", advantages, f32, count), ("returns", returns, f32, count),
              ("indices", indices, torch.int32, None))
    _require_tensors(wanted, device)
    shape = _lib.MlpPolicyDesc(p.data_ptr(), policy.obs_dim, policy.hidden, policy.num_actions, 0, 0)
    opt = _lib.PpoOptimizerDesc(p.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), optimizer.step)
    batch = _lib.PpoBatch(rollout.obs.data_ptr(), rollout.actions.data_ptr(), rollout.logprobs.data_ptr(), advantages.data_ptr(),
                          returns.data_ptr(), rollout.values.data_ptr(), count)
    cfg = _lib.PpoConfig(clip_coef, ent_coef, vf_coef, max_grad_norm, optimizer.lr, optimizer.betas[0], optimizer.betas[1],
                         optimizer.eps, (_lib.PPO_NORM_ADV if norm_adv else 0) | (_lib.PPO_CLIP_VLOSS if clip_vloss else 0))
    return _run_update(_lib.lib().mrl_ppo_update, (ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch)), indices,
                       (ctypes.byref(cfg),), optimizer, len(_lib.PPO_STATS), PpoResult, stats, grads)


class WideOptimizer(_AdamState):
    """Adam's state for ``agent_update`` (``torch.optim.Adam(lr, betas, eps)`` without amsgrad or weight decay, as the reference's
    ``CleanPPOAgent`` builds it, pantheonrl_extension/vectoragent.py:170) over a ``WidePolicy``'s flat parameters: the two
    moments, the number of steps taken and the cached scratch of ``mrl_agent_update``.  ``lr`` is an ordinary attribute:
    assign to it to anneal (:225-228)."""

    def __init__(self, policy, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(policy, WidePolicy):
            raise ValueError("policy must be a WidePolicy")
        super().__init__(policy, betas, eps)
        self.lr = float(lr)

    def workspace_bytes(self, capacity):
        """``mrl_agent_update_workspace_bytes`` for this policy's shape and ``capacity`` samples."""
        p = self.policy
        out = ctypes.c_uint64(0)
        _lib.check(_lib.lib().mrl_agent_update_workspace_bytes(p.obs_dim, p.state_dim, p.num_actions, int(capacity), ctypes.byref(out)))
        return int(out.value)

    def workspace(self, capacity):
        """The cached scratch, grown to ``workspace_bytes(capacity)`` where it is smaller."""
        return self._cached_workspace(self.workspace_bytes(capacity))


_WIDE_TYPES = {torch.int8: _lib.MRL_INT8, torch.uint8: _lib.MRL_UINT8, torch.int32: _lib.MRL_INT32, torch.float32: _lib.MRL_FLOAT32}


def agent_update(policy, optimizer, record, advantages=None, returns=None, epochs=1, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5,
                 max_grad_norm=0.5, norm_adv=True, clip_vloss=True, capacity=None, stats=True, grads=False):
    """``epochs`` whole-batch epochs of the reference's ``CleanPPOAgent`` update (pantheonrl_extension/vectoragent.py:283-323) on
    the active cells of ``record`` (an ``AgentRecord``), on the device (``mrl_agent_update``), enqueued on torch's current
    stream; it does not wait.  ``policy.params`` is updated in place.  ``advantages`` / ``returns``: (T, N) float32, default the
    record's own (what ``gae_active`` filled).  ``capacity``: the largest number of samples the scratch is sized for, default
    T * N; a batch with more active cells changes nothing and reports status 2, one with fewer than two status 1.  Returns
    ``PpoResult(stats, grads)``: (epochs, 10) float32 in the order of ``_lib.AGENT_UPDATE_STATS`` and (epochs, P) unclipped
    gradients, each None unless asked for.

    ``optimizer.step`` grows by ``epochs`` in every call: learning whether the epochs ran (status 0) would take a host read, and
    this function never waits.  A caller that reads the stats and finds a status other than 0 takes the epochs off again, as
    ``CleanPPOAgent`` does."""
    if not isinstance(policy, WidePolicy) or not isinstance(optimizer, WideOptimizer) or optimizer.policy is not policy:
        raise ValueError("policy must be a WidePolicy and optimizer the WideOptimizer made for it")
    if not isinstance(record, AgentRecord):
        raise ValueError("record must be an AgentRecord")
    p = policy.params
    if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
        raise ValueError("policy.params must be a contiguous float32 tensor on a GPU")
    advantages = record.advantages if advantages is None else advantages
    returns = record.returns if returns is None else returns
    device, f32 = p.device, torch.float32
    cells = record.num_steps * record.num_worlds
    if record.obs.dtype not in _WIDE_TYPES or record.states.dtype not in _WIDE_TYPES:
        raise ValueError("record.obs / record.states must be int8, uint8, int32 or float32")
    wanted = (("policy.params", p, f32, policy.num_params), ("optimizer.exp_avg", optimizer.exp_avg, f32, p.numel()),
              ("optimizer.exp_avg_sq", optimizer.exp_avg_sq, f32, p.numel()),
              ("record.obs", record.obs, record.obs.dtype, cells * policy.obs_dim),
              ("record.states", record.states, record.states.dtype, cells * policy.state_dim),
              ("record.action_masks", record.action_masks, torch.uint8, cells * policy.num_actions),
              ("record.active", record.active, torch.uint8, cells), ("record.actions", record.actions, torch.int32, cells),
              ("record.logprobs", record.logprobs, f32, cells), ("record.values", record.values, f32, cells),
              ("advantages", advantages, f32, cells), ("returns", returns, f32, cells))
    _require_tensors(wanted, device)
    epochs = int(epochs)
    capacity = cells if capacity is None else int(capacity)
    workspace = optimizer.workspace(capacity)
    out_stats = torch.empty((epochs, len(_lib.AGENT_UPDATE_STATS)), dtype=f32, device=device) if stats else None
    out_grads = torch.empty((epochs, p.numel()), dtype=f32, device=device) if grads else None
    desc = policy.desc()
    opt = _lib.PpoOptimizerDesc(p.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), optimizer.step)
    cfg = _lib.PpoConfig(clip_coef, ent_coef, vf_coef, max_grad_norm, optimizer.lr, optimizer.betas[0], optimizer.betas[1],
                         optimizer.eps, (_lib.PPO_NORM_ADV if norm_adv else 0) | (_lib.PPO_CLIP_VLOSS if clip_vloss else 0))
    gpu = device.index
    _lib.check(_lib.lib().mrl_agent_update(ctypes.byref(desc), ctypes.byref(opt), ctypes.byref(record.struct),
                                           _WIDE_TYPES[record.obs.dtype], _WIDE_TYPES[record.states.dtype], advantages.data_ptr(),
                                           returns.data_ptr(), epochs, ctypes.byref(cfg), capacity, workspace.data_ptr(),
                                           workspace.numel(), out_stats.data_ptr() if stats else None,
                                           out_grads.data_ptr() if grads else None, gpu, _stream_ptr(gpu)))
    optimizer.step += epochs
    return PpoResult(out_stats, out_grads)


class ValueNorm:
    """The reference's ``ValueNorm`` (train/MAPPO/utils/valuenorm.py, scalar values, ``per_element_update`` off) as the three
    device floats ``mrl_mappo_update`` keeps up to date: ``state`` = (running_mean, running_mean_sq, debiasing_term).  The
    methods are torch ops on device tensors with the reference's formulas; none of them waits for the device."""

    def __init__(self, device, beta=0.99999, epsilon=1e-5):
        self.beta, self.epsilon = float(beta), float(epsilon)
        self.state = torch.zeros(3, dtype=torch.float32, device=torch.device(device))

    def running_mean_var(self):
        floor = self.state[2].clamp(min=self.epsilon)
        mean = self.state[0] / floor
        return mean, (self.state[1] / floor - mean ** 2).clamp(min=1e-2)

    def update(self, x):
        """One ``ValueNorm.update`` in torch, as the reference runs it (``mappo_update`` does this on the device per row)."""
        x = x.to(torch.float32)
        self.state[0].mul_(self.beta).add_(x.mean() * (1.0 - self.beta))
        self.state[1].mul_(self.beta).add_((x ** 2).mean() * (1.0 - self.beta))
        self.state[2].mul_(self.beta).add_(1.0 * (1.0 - self.beta))

    def normalize(self, x):
        mean, var = self.running_mean_var()
        return (x.to(torch.float32) - mean) / torch.sqrt(var)

    def denormalize(self, x):
        mean, var = self.running_mean_var()
        return x.to(torch.float32) * torch.sqrt(var) + mean


class MappoOptimizer(_AdamState):
    """The state of MAPPO's two Adam optimizers for a ``CnnPolicy`` or an ``MlpBasePolicy`` (``R_MAPPOPolicy``: ``torch.optim.Adam(lr, eps=opti_eps,
    weight_decay=0)`` for the actor and for the critic): ``exp_avg`` and ``exp_avg_sq`` over the whole flat tensor, the number
    of steps both have taken (``step``) and the scratch ``mrl_mappo_update`` asks for, kept from call to call.  ``lr`` and
    ``critic_lr`` are ordinary attributes: assign to them for the reference's ``lr_decay``."""

    def __init__(self, policy, lr=5e-4, critic_lr=5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(policy, (CnnPolicy, MlpBasePolicy)):
            raise ValueError("policy must be a CnnPolicy or an MlpBasePolicy")
        super().__init__(policy, betas, eps)
        self.lr, self.critic_lr = float(lr), float(critic_lr)

    def workspace_bytes(self, minibatch_size, num_minibatches):
        """``mrl_mappo_workspace_bytes`` (``mrl_mappo_mlp_workspace_bytes`` for an ``MlpBasePolicy``) for this policy's shape."""
        out = ctypes.c_uint64(0)
        _lib.check(self.policy._mappo_workspace_bytes(int(minibatch_size), int(num_minibatches), ctypes.byref(out)))
        return int(out.value)


def mappo_advantages(record, value_norm=None, gamma=0.99, gae_lambda=0.95, seats=None):
    """``(advantages, returns)`` of a ``CnnRecord`` (Overcooked's or Simplecooked's, P = 1 included), each (T, N, P), as ``R_MAPPO.train`` and ``SharedReplayBuffer.compute_returns``
    form them (train/MAPPO/r_mappo.py:174-182, utils/shared_buffer.py:216-228 with ``use_gae``; every active mask one): the
    record's values denormalised when a ``ValueNorm`` is given, ``gae`` on those (``mrl_gae``: the reference's recurrence with
    ``masks[t + 1] = 1 - dones[t + 1]``), then ``(A - mean) / (std + 1e-5)`` over the whole buffer with torch's unbiased std.
    ``returns`` are in the denormalised scale, as the reference's buffer holds them.  It runs once per update, so apart from
    ``mrl_gae`` it is a handful of torch ops on the record's device; it does not wait.
    ``seats`` (default ``None``: as above): a list of seats; the mean and the std are then taken over those seats' columns only and
    only those columns are normalised -- the others keep their raw GAE advantages.  That is what an ego trained against frozen
    partners of a ``CnnPolicyBank`` needs: the partners' columns hold values of other critics."""
    if not isinstance(record, _MappoRecord):
        raise ValueError("record must be a CnnRecord or an MlpBaseRecord")
    if seats is not None:
        seats = sorted({int(seat) for seat in seats})
        if not seats or seats[0] < 0 or seats[-1] >= record.num_players:
            raise ValueError(f"seats must name some of the record's seats 0..{record.num_players - 1}")
    rollout = record.rollout()
    if value_norm is not None:
        t, cols = record.num_steps, record.num_worlds * record.num_players
        values = value_norm.denormalize(record.values).contiguous()
        rollout = rollout._replace(values=values[:t].view(t, cols), next_value=values[t].view(cols))
    advantages, returns = gae(rollout, gamma, gae_lambda)
    shape = (record.num_steps, record.num_worlds, record.num_players)
    if seats is None:
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-5)
        return advantages.view(shape), returns.view(shape)
    advantages = advantages.view(shape).clone()
    own = advantages[:, :, seats]
    advantages[:, :, seats] = (own - own.mean()) / (own.std() + 1e-5)
    return advantages, returns.view(shape)


MappoResult = collections.namedtuple("MappoResult", "stats grads")  # (K, 8) in the order of ``_lib.MAPPO_STATS`` / (K, P), or None


def _mappo_config(optimizer, value_norm, clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta, use_huber_loss,
                  use_clipped_value_loss, use_max_grad_norm):
    """``mrl_mappo_config`` of ``mappo_update`` and ``mappo_update_bank``: the loss options, the optimizer's numbers and the
    constants of ``value_norm`` (a ``ValueNorm``, a ``ValueNormBank`` or None)"""
    beta = value_norm.beta if value_norm is not None else 0.99999
    flags = ((_lib.MAPPO_VALUENORM if value_norm is not None else 0) | (_lib.MAPPO_HUBER_LOSS if use_huber_loss else 0) |
             (_lib.MAPPO_CLIPPED_VALUE_LOSS if use_clipped_value_loss else 0) | (_lib.MAPPO_MAX_GRAD_NORM if use_max_grad_norm else 0))
    # torch multiplies a float32 tensor by the Python floats beta and 1.0 - beta rounded to float32, each on its own
    return _lib.MappoConfig(clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta, optimizer.lr, optimizer.critic_lr,
                            optimizer.betas[0], optimizer.betas[1], optimizer.eps, beta, 1.0 - beta,
                            value_norm.epsilon if value_norm is not None else 1e-5, flags)


def mappo_update(policy, optimizer, record, ring, advantages, returns, indices, value_norm=None, clip_param=0.2, entropy_coef=0.01,
                 value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, use_huber_loss=True, use_clipped_value_loss=True,
                 use_max_grad_norm=True, stats=True, grads=False):
    """One actor and one critic Adam step per row of ``indices`` on MAPPO's losses (``R_MAPPO.ppo_update``,
    train/MAPPO/r_mappo.py:91-164, feed-forward networks), on the device (``mrl_mappo_update``: three launches per row),
    enqueued on torch's current stream; it does not wait.  ``policy.params`` is updated in place -- the next ``rollout`` or
    ``cnn_act`` reads it as it stands --, ``optimizer.step`` grows by the number of rows, and with ``value_norm`` (a
    ``ValueNorm``: the reference's ``use_valuenorm``) its state takes one update per row.  ``record`` and ``ring`` are what
    ``rollout_cnn`` filled, of either kitchen (the call takes the shape from ``policy``): sample ``(t N + n) P + p`` is row t, world n, seat p, and its observation is ring slot t, read as
    int8 in place.  ``advantages`` and ``returns`` (T, N, P) are ``mappo_advantages``'; ``indices`` (K, B) int32 sample
    numbers (``minibatch_indices``).  The defaults are the reference's (train/config.py).  Returns ``MappoResult(stats,
    grads)``: (K, 8) float32, columns ``_lib.MAPPO_STATS``, and (K, P) the unclipped gradients, each None unless asked for.
    For an ``MlpBasePolicy`` (the balance beam; ``mrl_mappo_mlp_update``) ``record`` is an ``MlpBaseRecord``, the batch is its
    ``obs`` and ``ring`` must be ``None``.
    Not built: active masks, PopArt, recurrent policies, ``update_actor=False``, weight decay."""
    if not isinstance(policy, (CnnPolicy, MlpBasePolicy)) or not isinstance(optimizer, MappoOptimizer) or optimizer.policy is not policy:
        raise ValueError("policy must be a CnnPolicy or an MlpBasePolicy and optimizer the MappoOptimizer made for it")
    policy._mappo_check(record, ring)  # the record is the policy's kind, and so is the ring
    if value_norm is not None and not isinstance(value_norm, ValueNorm):
        raise ValueError("value_norm must be a ValueNorm or None")
    p = policy._check_params()
    device, f32 = p.device, torch.float32
    count = record.num_steps * record.num_worlds * record.num_players
    # views of the record's first T rows: contiguous, because the rows are the leading dimension
    wanted = [("policy.params", p, f32, p.numel()), ("optimizer.exp_avg", optimizer.exp_avg, f32, p.numel()),
              ("optimizer.exp_avg_sq", optimizer.exp_avg_sq, f32, p.numel()), ("record.actions", record.actions, torch.int32, count),
              ("record.logprobs", record.logprobs, f32, count), ("record.values", record.values, f32, count + count // max(record.num_steps, 1)),
              ("advantages", advantages, f32, count), ("returns", returns, f32, count), ("indices", indices, torch.int32, None)]
    if value_norm is not None:
        wanted.append(("value_norm.state", value_norm.state, f32, 3))
    _require_tensors(wanted, device)
    (entry, _), shape, batch_type, obs = policy._mappo_batch(record, ring, count)  # the policy's own entry point and batch
    opt = _lib.MappoOptimizerDesc(p.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), optimizer.step)
    batch = batch_type(obs.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(), returns.data_ptr(),
                       advantages.data_ptr(), count)
    cfg = _mappo_config(optimizer, value_norm, clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta, use_huber_loss,
                        use_clipped_value_loss, use_max_grad_norm)
    return _run_update(entry, (ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch)), indices,
                       (ctypes.byref(cfg), value_norm.state.data_ptr() if value_norm is not None else None), optimizer,
                       len(_lib.MAPPO_STATS), MappoResult, stats, grads)


class ValueNormBank:
    """One ``ValueNorm`` per member of a policy bank in one tensor: ``state`` (K, 3) float32, row k the three running floats of
    bank row k (``mrl_mappo_bank_update``'s ``value_norm_state``).  ``member(k)`` is a ``ValueNorm`` whose ``state`` IS row k, a
    view: the plain ``mappo_update`` and ``mappo_advantages`` take it, and what either call leaves the other reads."""

    def __init__(self, num_policies, device, beta=0.99999, epsilon=1e-5):
        self.num_policies = int(num_policies)
        if not 1 <= self.num_policies <= _lib.CNN_BANK_MAX_POLICIES:
            raise ValueError(f"a bank holds 1 to {_lib.CNN_BANK_MAX_POLICIES} policies, not {num_policies}")
        self.beta, self.epsilon = float(beta), float(epsilon)
        self.state = torch.zeros((self.num_policies, 3), dtype=torch.float32, device=torch.device(device))

    def __len__(self):
        return self.num_policies

    def member(self, k):
        k = int(k)
        if not 0 <= k < self.num_policies:
            raise IndexError(f"the bank holds policies 0..{self.num_policies - 1}, not {k}")
        member = ValueNorm.__new__(ValueNorm)
        member.beta, member.epsilon, member.state = self.beta, self.epsilon, self.state[k]
        return member


class MappoBankOptimizer(_AdamState):
    """``MappoOptimizer`` for every member of a ``CnnPolicyBank`` or an ``MlpBasePolicyBank`` at once (``mrl_mappo_bank_optimizer``):
    ``exp_avg`` and ``exp_avg_sq`` (K, num_params), row k the moments of bank row k, ONE ``step`` -- every member has taken the same
    number of Adam steps -- and one ``lr`` / ``critic_lr`` (assignable, as ``MappoOptimizer``'s).  ``member(k)`` is a
    ``MappoOptimizer`` for ``bank.policy(k)`` whose moments are VIEWS of row k and whose ``step`` is this one's at the time of the
    call: the plain ``mappo_update`` steps that member alone (the bank's ``step`` does not follow)."""

    def __init__(self, bank, lr=5e-4, critic_lr=5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(bank, (CnnPolicyBank, MlpBasePolicyBank)):
            raise ValueError("bank must be a CnnPolicyBank or an MlpBasePolicyBank")
        super().__init__(bank, betas, eps)  # (the moments take bank.params' shape)
        self.bank = bank
        self.lr, self.critic_lr = float(lr), float(critic_lr)

    def member(self, k):
        member = MappoOptimizer(self.bank.policy(k), self.lr, self.critic_lr, self.betas, self.eps)
        member.exp_avg, member.exp_avg_sq, member.step = self.exp_avg[int(k)], self.exp_avg_sq[int(k)], self.step
        return member

    def workspace_bytes(self, minibatch_size, num_minibatches, num_members=1):
        """``mrl_mappo_bank_workspace_bytes`` (``mrl_mappo_mlp_bank_workspace_bytes`` for an ``MlpBasePolicyBank``): ``num_members``
        times the plain call's."""
        out = ctypes.c_uint64(0)
        _lib.check(self.bank.policy(0)._mappo_workspace_bytes(int(minibatch_size), int(num_minibatches), ctypes.byref(out), int(num_members)))
        return int(out.value)

    def workspace(self, minibatch_size, num_minibatches, num_members=1):
        return self._cached_workspace(self.workspace_bytes(minibatch_size, num_minibatches, num_members))


def member_samples(owner, members, num_steps):
    """The sample numbers of each member's cells in a record of ``num_steps`` rows -> int32 (M, S) on ``owner``'s device.
    ``owner``: int32 (N, P), the bank row that owns each (world, seat) cell -- the ``ids`` of a ``rollout_bank`` without a
    resample; ``members``: the bank rows wanted.  Row z holds ``(t N + n) P + p`` for every t < ``num_steps`` and every cell with
    ``owner[n, p] == members[z]``, ascending: member z's own batch, S = ``num_steps`` times its cells.  Raises unless every member
    owns the same number (at least one) of cells: ``mappo_update_bank`` takes one B for all.  Looks at ``owner`` on the host, so it
    is called once, outside the training loop."""
    if not isinstance(owner, torch.Tensor) or owner.dim() != 2 or owner.dtype != torch.int32:
        raise ValueError("owner must be an int32 tensor (num_worlds, num_players)")
    members, t = [int(k) for k in members], int(num_steps)
    cells, flat = owner.numel(), owner.reshape(-1).cpu()
    if not members or t < 1 or t * cells >= 2 ** 31:
        raise ValueError("member_samples needs at least one member, one step and fewer than 2^31 samples")
    own = [torch.nonzero(flat == k).view(-1) for k in members]  # ascending
    counts = [int(c.numel()) for c in own]
    if counts[0] == 0 or any(c != counts[0] for c in counts):
        raise ValueError(f"the members must own the same number of cells, at least one each; members {members} own {counts}")
    rows = torch.arange(t, dtype=torch.int64).view(t, 1) * cells
    return torch.stack([(rows + c.view(1, -1)).view(-1) for c in own]).to(torch.int32).to(owner.device)


def mappo_advantages_bank(record, cells, value_norms=None, gamma=0.99, gae_lambda=0.95, first_member=0):
    """``mappo_advantages`` for the record of a ``rollout_bank`` whose cells are owned by different members -> (advantages,
    returns), each (T, N, P).  ``cells``: ``member_samples``' (M, S) for the record's T, row z the cells of bank row ``first_member``
    + z.  With ``value_norms`` (a ``ValueNormBank``) each member's values, the closing ones included, are denormalised with its own
    row's statistics; then ONE ``mrl_gae`` over the whole record (a column's recurrence reads that column alone); then ``(A -
    mean) / (std + 1e-5)`` per member over that member's cells only -- for each member what ``mappo_advantages`` gives on a record
    of its worlds alone.  Cells of no member keep their values as recorded and their raw advantages.  A loop of torch ops over the
    members on the record's device; it does not wait."""
    if not isinstance(record, _MappoRecord):
        raise ValueError("record must be a CnnRecord or an MlpBaseRecord")
    if value_norms is not None and not isinstance(value_norms, ValueNormBank):
        raise ValueError("value_norms must be a ValueNormBank or None")
    t, cols = record.num_steps, record.num_worlds * record.num_players
    if (not isinstance(cells, torch.Tensor) or cells.dim() != 2 or cells.dtype != torch.int32 or cells.device != record.values.device or
            t < 1 or cells.shape[1] == 0 or cells.shape[1] % t):
        raise ValueError(f"cells must be member_samples' int32 (members, samples) on {record.values.device} for the record's {t} steps")
    at = cells.to(torch.int64)
    each = cells.shape[1] // t  # a member's cells: the head of its row is its samples of row 0
    rollout = record.rollout()
    if value_norms is not None:
        values = record.values.clone()
        flat = values.view(-1)
        for z in range(cells.shape[0]):
            own = torch.cat([at[z], at[z, :each] + t * cols])  # rows 0 .. T - 1, then the closing row T
            flat[own] = value_norms.member(int(first_member) + z).denormalize(flat[own])
        rollout = rollout._replace(values=values[:t].view(t, cols), next_value=values[t].view(cols))
    advantages, returns = gae(rollout, gamma, gae_lambda)
    shape = (record.num_steps, record.num_worlds, record.num_players)
    flat = advantages.view(-1)
    for z in range(cells.shape[0]):
        own = flat[at[z]]
        flat[at[z]] = (own - own.mean()) / (own.std() + 1e-5)
    return advantages.view(shape), returns.view(shape)


def mappo_update_bank(bank, optimizer, record, ring, advantages, returns, indices, value_norms=None, first_member=0, clip_param=0.2,
                      entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, use_huber_loss=True,
                      use_clipped_value_loss=True, use_max_grad_norm=True, stats=True, grads=False):
    """``mappo_update`` for M members of ``bank`` (a ``CnnPolicyBank`` or an ``MlpBasePolicyBank``) in one call
    (``mrl_mappo_bank_update`` / ``mrl_mappo_mlp_bank_update``: 2 + 3 R launches whatever M is), enqueued on torch's current
    stream; it does not wait.  ``indices``: int32 (M, R, B); member z is bank row ``first_member`` + z and takes, for r < R, one
    actor and one critic Adam step on the samples ``indices[z, r]`` -- sample numbers of the shared ``record`` (and ``ring``),
    ``advantages`` and ``returns``, normally a permutation of ``member_samples``' row z cut into rows.  ``optimizer``: the
    ``MappoBankOptimizer`` made for ``bank``; its ``step`` grows by R.  ``value_norms``: a ``ValueNormBank`` of the bank's size
    or None.  The loss options are ``mappo_update``'s.  Bank row ``first_member`` + z, its moments, its ValueNorm row, ``stats[z]``
    and ``grads[z]`` are bit for bit what ``mappo_update`` leaves for ``bank.policy(first_member + z)`` with
    ``optimizer.member(...)``, ``value_norms.member(...)`` and ``indices[z]``; no other row of the bank is read or written.
    Returns ``MappoResult(stats, grads)``: (M, R, 8) and (M, R, P), each None unless asked for."""
    if (not isinstance(bank, (CnnPolicyBank, MlpBasePolicyBank)) or not isinstance(optimizer, MappoBankOptimizer) or
            optimizer.bank is not bank):
        raise ValueError("bank must be a CnnPolicyBank or an MlpBasePolicyBank and optimizer the MappoBankOptimizer made for it")
    policy = bank.policy(0)
    policy._mappo_check(record, ring)
    if value_norms is not None and (not isinstance(value_norms, ValueNormBank) or len(value_norms) != len(bank)):
        raise ValueError("value_norms must be a ValueNormBank of the bank's size or None")
    if not isinstance(indices, torch.Tensor) or indices.dim() != 3:
        raise ValueError("indices must be (members, rows, minibatch_size)")
    members, rows, width = indices.shape
    first = int(first_member)
    if members < 1 or first < 0 or first + members > len(bank):
        raise ValueError(f"members {first}..{first + members - 1} are not rows of a bank of {len(bank)}")
    p = bank.params
    if not p.is_cuda:
        raise ValueError("bank.params must be on a GPU")
    bank._check_params(p.device.index)
    device, f32 = p.device, torch.float32
    count = record.num_steps * record.num_worlds * record.num_players
    wanted = [("optimizer.exp_avg", optimizer.exp_avg, f32, p.numel()), ("optimizer.exp_avg_sq", optimizer.exp_avg_sq, f32, p.numel()),
              ("record.actions", record.actions, torch.int32, count), ("record.logprobs", record.logprobs, f32, count),
              ("record.values", record.values, f32, count + count // max(record.num_steps, 1)), ("advantages", advantages, f32, count),
              ("returns", returns, f32, count), ("indices", indices, torch.int32, None)]
    if value_norms is not None:
        wanted.append(("value_norms.state", value_norms.state, f32, 3 * len(bank)))
    _require_tensors(wanted, device)
    (_, entry), shape, batch_type, obs = policy._mappo_batch(record, ring, count)  # row 0's struct: its params are the bank's base
    opt = _lib.MappoBankOptimizerDesc(p.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), 4 * p.stride(0), len(bank),
                                      first, members, optimizer.step)
    batch = batch_type(obs.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(), returns.data_ptr(),
                       advantages.data_ptr(), count)
    cfg = _mappo_config(optimizer, value_norms, clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta, use_huber_loss,
                        use_clipped_value_loss, use_max_grad_norm)
    workspace = optimizer.workspace(width, rows, members) if width else None
    out_stats = torch.empty((members, rows, len(_lib.MAPPO_STATS)), dtype=f32, device=device) if stats else None
    out_grads = torch.empty((members, rows, bank.num_params), dtype=f32, device=device) if grads else None
    gpu = device.index
    _lib.check(entry(ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), rows, width, ctypes.byref(cfg),
                     value_norms.state.data_ptr() if value_norms is not None else None,
                     workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0,
                     out_stats.data_ptr() if stats else None, out_grads.data_ptr() if grads else None, gpu, _stream_ptr(gpu)))
    optimizer.step += rows
    return MappoResult(out_stats, out_grads)


def totals_of(totals):
    """The column sums of a TOTALS tensor (float64, (blocks, 2 + players)) as ``episode_totals`` returns them."""
    sums = totals.sum(dim=0).tolist()  # (the host waits here)
    return {"episodes": int(round(sums[0])), "steps": int(round(sums[1])), "returns": [float(v) for v in sums[2:]]}


class EpisodeStats:
    """What ``env.episode_stats`` is for an env wrapper built with ``record_episode_statistics=True``: the five tensors of
    ``mrl_enable_episode_stats`` as persistent torch views on the simulator's GPU."""

    def __init__(self, sim):
        sim.enable_episode_stats()
        self.episode_return = sim.episode_return_tensor().to_torch()
        self.episode_steps = sim.episode_steps_tensor().to_torch()
        self.last_return = sim.last_episode_return_tensor().to_torch()
        self.last_steps = sim.last_episode_steps_tensor().to_torch()
        self.totals = sim.episode_totals_tensor().to_torch()


class RecordsEpisodeStatistics:
    """Mixin of the env wrappers (``self.sim`` is the simulator): the ``record_episode_statistics`` keyword.  ``infos`` stays
    as it is -- per-world dicts would mean a host synchronisation per step; the numbers are tensors and one call."""

    episode_stats = None

    def _record_episode_statistics(self, record):
        if record:
            self.episode_stats = EpisodeStats(self.sim)

    def _recording(self):
        if self.episode_stats is None:
            raise MrlError("this environment was built without record_episode_statistics=True")

    def episode_totals(self):
        """``sim.episode_totals()``: episodes finished since the last clear, their steps and returns (waits for the GPU)."""
        self._recording()
        return self.sim.episode_totals()

    def clear_episode_totals(self):
        self._recording()
        self.sim.clear_episode_totals()


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


class ActsWithCnnPolicy:
    """Mixin of the two kitchen env wrappers (``envs/overcooked_env.py``, ``envs/overcooked2_env.py``; ``self.sim``, ``static_actions``,
    ``static_world_major_observations``, ``num_envs`` and ``num_players`` are the wrapper's): MAPPO's CNN actor-critic on the device."""

    def act(self, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False):
        """The seats in ``players`` (default all) act under ``policy`` (a ``simulators.CnnPolicy``) on the device, one launch
        (``mrl_cnn_act``): the actions are in ``static_actions``, which is returned; with ``record`` (a ``CnnRecord``) row ``row``
        also takes log-probs, values and the bookkeeping.  The observations read are those of the most recent step, also where
        ``n_step(out=...)`` sent them."""
        cnn_act(self.sim, policy, players, record, row=row, seed=seed, step=step, greedy=greedy)
        return self.static_actions

    def rollout(self, policy, num_steps, seed=0, first_step=0, players=None, record=None, ring=None, greedy=False):
        """``num_steps`` steps under ``policy`` without the host in the loop (``mrl_rollout_cnn``) -> (record, ring): a ``CnnRecord``
        and the observation ring (T + 1, N, P, H, W, F) whose slot k is what the act of step k saw.  ``record`` / ``ring``: an
        earlier call's, filled again.  Afterwards the observations of the state reached (slot T) are also where the simulator's output
        pointed before the call -- ``static_world_major_observations`` unless ``n_step(out=...)`` redirected it -- so rollouts chain.  ``simulators.gae(record.rollout(), gamma, gae_lambda)`` gives the advantages."""
        device = self.static_actions.device
        record = CnnRecord._for_rollout(record, num_steps, self.num_envs, self.num_players, device)
        if ring is None:
            ring = torch.empty((int(num_steps) + 1,) + tuple(self.static_world_major_observations.shape), dtype=torch.int8, device=device)
        self.sim.rollout_cnn(policy, record, ring, players=players, seed=seed, first_step=first_step, greedy=greedy)
        return record, ring

    def act_bank(self, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False):
        """``act`` with a policy per (world, seat) cell: seat p of world n acts under row ``ids[n, p]`` of ``bank`` (a
        ``simulators.CnnPolicyBank``), cells at -1 keep their actions (``mrl_cnn_act_bank``: the plan and the act, every output bit for bit
        ``act``'s under the cell's policy).  ``ids``: int32 (N, P) on the device.  Returns ``static_actions``."""
        cnn_act_bank(self.sim, bank, ids, players, record, ids_row, row=row, seed=seed, step=step, greedy=greedy)
        return self.static_actions

    def rollout_bank(self, bank, ids, num_steps, episodes=None, resample=None, seed=0, first_step=0, players=None, record=None, ring=None,
                     ids_record=None, greedy=False):
        """``rollout`` under a bank (``mrl_rollout_cnn_bank``) -> (record, ring, ids_record): ``ids_record`` int32 (T + 1, N, P) holds
        the ids each act used (-1 where it did not act).  ``resample`` (a ``simulators.CnnResample``) runs behind every step: worlds
        that have just restarted draw their next policies into ``ids`` and count in ``episodes`` (int32 (N), made when ``None`` and
        then kept by the env as ``bank_episodes``)."""
        device = self.static_actions.device
        record = CnnRecord._for_rollout(record, num_steps, self.num_envs, self.num_players, device)
        if ring is None:
            ring = torch.empty((int(num_steps) + 1,) + tuple(self.static_world_major_observations.shape), dtype=torch.int8, device=device)
        ids_record, episodes = _bank_rollout_buffers(self, num_steps, self.num_players, ids_record, episodes, resample)
        self.sim.rollout_cnn_bank(bank, ids, record, ring, episodes=episodes, resample=resample, ids_record=ids_record, players=players,
                                  seed=seed, first_step=first_step, greedy=greedy)
        return record, ring, ids_record


class ActsWithMlpBasePolicy:
    """Mixin of the balance-beam env wrapper (``envs/balance_beam_env.py``; ``self.sim``, ``static_actions``, ``num_envs`` and
    ``n_players`` are the wrapper's): MAPPO's MLP actor-critic on the device, one policy for the batch or a bank's member per cell."""

    def act(self, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False):
        """The seats in ``players`` (default both) act under ``policy`` (a ``simulators.MlpBasePolicy``) on the device, one launch
        (``mrl_mlpbase_act``): the actions are in ``static_actions``, which is returned; with ``record`` (an ``MlpBaseRecord``)
        row ``row`` also takes log-probs, values, the observation rows and the bookkeeping."""
        mlpbase_act(self.sim, policy, players, record, row=row, seed=seed, step=step, greedy=greedy)
        return self.static_actions

    def rollout(self, policy, num_steps, seed=0, first_step=0, players=None, record=None, greedy=False):
        """``num_steps`` steps under ``policy`` without the host in the loop (``mrl_rollout_mlpbase``) -> an ``MlpBaseRecord``
        whose ``obs[k]`` is what the act of step k saw.  ``record``: an earlier call's, filled again.  Rollouts chain: the next one
        acts on the state this one reached.  ``simulators.mappo_advantages(record)`` gives the advantages."""
        record = MlpBaseRecord._for_rollout(record, num_steps, self.num_envs, self.n_players, self.static_actions.device)
        self.sim.rollout_mlpbase(policy, record, players=players, seed=seed, first_step=first_step, greedy=greedy)
        return record

    def act_bank(self, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False):
        """``act`` with a policy per (world, seat) cell: seat p of world n acts under row ``ids[n, p]`` of ``bank`` (a
        ``simulators.MlpBasePolicyBank``), cells at -1 keep their actions (``mrl_mlpbase_act_bank``: the plan and the act, every
        output bit for bit ``act``'s under the cell's policy).  ``ids``: int32 (N, P) on the device.  Returns ``static_actions``."""
        mlpbase_act_bank(self.sim, bank, ids, players, record, ids_row, row=row, seed=seed, step=step, greedy=greedy)
        return self.static_actions

    def rollout_bank(self, bank, ids, num_steps, episodes=None, resample=None, seed=0, first_step=0, players=None, record=None,
                     ids_record=None, greedy=False):
        """``rollout`` under a bank (``mrl_rollout_mlpbase_bank``) -> (record, ids_record): ``ids_record`` int32 (T + 1, N, P) holds
        the ids each act used (-1 where it did not act).  ``resample`` (a ``simulators.CnnResample``) runs behind every step: worlds
        that have just restarted draw their next policies into ``ids`` and count in ``episodes`` (int32 (N), made when ``None`` and
        then kept by the env as ``bank_episodes``)."""
        record = MlpBaseRecord._for_rollout(record, num_steps, self.num_envs, self.n_players, self.static_actions.device)
        ids_record, episodes = _bank_rollout_buffers(self, num_steps, self.n_players, ids_record, episodes, resample)
        self.sim.rollout_mlpbase_bank(bank, ids, record, episodes=episodes, resample=resample, ids_record=ids_record, players=players,
                                      seed=seed, first_step=first_step, greedy=greedy)
        return record, ids_record


class _Simulator:
    """Shared handle management for the three games."""

    _SLOTS = {}

    def __init__(self, exec_mode, gpu_id):
        mode = getattr(exec_mode, "name", str(exec_mode))
        if mode == "CPU" or exec_mode == 0:
            raise NotImplementedError(
                "ExecMode.CPU: this engine has only the HIP (MI355X) step kernels; the reference's CPU "
                "TaskGraph executor is not reproduced (the test-only CPU oracle lives in oracle/).")
        self._L = _lib.lib()
        self._handle = ctypes.c_void_p()
        self.gpu_id = int(gpu_id)
        self._tensors = {}

    # --- reference API -------------------------------------------------
    def step(self):
        """One environment step for all worlds, enqueued on torch's current stream
        (Manager::step; no host synchronisation)."""
        stream = _stream_ptr(self.gpu_id)
        rc = self._L.mrl_step(self._handle, stream)
        if rc:
            _lib.check(rc)

    # --- extensions ----------------------------------------------------
    def _action_pointer(self, actions, steps=None):
        """Every entry point that hands the library a caller-owned action array goes through here: the
        library reads raw int32 words, so dtype, layout, device and size are checked on this side."""
        if not isinstance(actions, torch.Tensor) or not actions.is_cuda or actions.device.index != self.gpu_id:
            raise ValueError(f"actions must be a tensor on cuda:{self.gpu_id} (the simulator's device)")
        if actions.dtype != torch.int32 or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous int32 tensor on the simulator's device")
        expect = self._action_numel if steps is None else steps * self._action_numel
        if actions.numel() != expect:
            raise ValueError(f"actions has {actions.numel()} elements, expected {expect}")
        return actions.data_ptr()

    def step_with_actions(self, actions):
        """Step reading actions from ``actions`` (int32, the ACTION tensor's shape,
        contiguous, on this GPU) instead of the ACTION tensor."""
        ptr = self._action_pointer(actions)
        stream = _stream_ptr(self.gpu_id)
        rc = self._L.mrl_step_with_actions(self._handle, ptr, stream)
        if rc:
            _lib.check(rc)

    def step_with_actions_i64(self, actions):
        """Step reading ``actions`` as int64 (the ACTION tensor's shape, contiguous, on this GPU): the step kernel narrows
        them itself and mirrors them into the ACTION tensor (``mrl_step_with_actions_i64``; Overcooked, Simplecooked)."""
        if (not isinstance(actions, torch.Tensor) or not actions.is_cuda or actions.device.index != self.gpu_id or
                actions.dtype != torch.int64 or not actions.is_contiguous() or actions.numel() != self._action_numel):
            raise ValueError("actions must be a contiguous int64 tensor of the ACTION tensor's size on the simulator's device")
        self._step_i64_checked(actions.data_ptr())

    def _step_i64_checked(self, ptr):
        """``mrl_step_with_actions_i64`` on a pointer the caller has already validated (the env wrappers check the
        harness's tensor once, not twice: every microsecond of host work per call shows at small batches)."""
        rc = self._L.mrl_step_with_actions_i64(self._handle, ptr, _stream_ptr(self.gpu_id))
        if rc:
            _lib.check(rc)

    def step_sequence(self, actions):
        """One step per leading index of ``actions`` (int32, shape (K,) + ACTION tensor's shape, contiguous,
        on this GPU): same results as K ``step_with_actions`` calls (``mrl_step_sequence``)."""
        if not isinstance(actions, torch.Tensor) or actions.dim() < 1:
            raise ValueError("actions must hold K consecutive ACTION tensors")
        ptr = self._action_pointer(actions, steps=int(actions.shape[0]))
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_step_sequence(self._handle, ptr, int(actions.shape[0]), stream))

    def rollout_random(self, num_steps, seed=0, first_step=0):
        """``num_steps`` steps under the uniform random policy, actions drawn on the
        device (``mrl_rollout_random``; see ``random_action`` for the stream)."""
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_rollout_random(self._handle, int(num_steps), int(seed) & (2 ** 64 - 1), int(first_step),
                                              stream))

    def rollout_policy(self, policy, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``num_steps`` steps under ``policy`` (an ``MlpPolicy`` on this GPU) with the host out of the loop: observe, both
        nets, draw, log-prob, value, step and record, two launches per step (``mrl_rollout_policy``; Cartpole and Acrobot).
        Returns a ``Rollout`` of tensors on this GPU -- new ones, or ``out`` (an earlier call's result) filled again.  The
        draw of (step index ``first_step + k``, world) uses ``sample_u``; ``greedy`` takes the first arg-max instead."""
        if not isinstance(policy, MlpPolicy):
            raise ValueError("policy must be an MlpPolicy")
        p = policy.params
        if not p.is_cuda or p.device.index != self.gpu_id or p.dtype != torch.float32 or not p.is_contiguous():
            raise ValueError(f"policy.params must be a contiguous float32 tensor on cuda:{self.gpu_id} (the simulator's device)")
        if p.numel() != int(self._L.mrl_mlp_policy_num_params(policy.obs_dim, policy.hidden, policy.num_actions)):
            raise ValueError("policy.params does not have mrl_mlp_policy_num_params elements")
        t, n, d = int(num_steps), self.num_worlds, policy.obs_dim
        if t < 0:
            raise ValueError("num_steps must not be negative")
        f32, device = torch.float32, torch.device("cuda", self.gpu_id)
        shapes = Rollout((t, n, d), (t, n), (t, n), (t, n), (t, n), (t, n), (n, d), (n,), (n,))
        if out is None:
            out = Rollout(*[torch.empty(shape, dtype=torch.int32 if name == "actions" else f32, device=device)
                            for name, shape in zip(Rollout._fields, shapes)])
        else:
            for name, tensor, shape in zip(Rollout._fields, out, shapes):
                if (not isinstance(tensor, torch.Tensor) or tensor.device != device or tuple(tensor.shape) != shape or
                        tensor.dtype != (torch.int32 if name == "actions" else f32) or not tensor.is_contiguous()):
                    raise ValueError(f"out.{name} must be a contiguous {shape} tensor on cuda:{self.gpu_id}")
        desc = _lib.MlpPolicyDesc(p.data_ptr(), d, policy.hidden, policy.num_actions,
                                  _lib.OBS_ACROBOT_GYM if policy.observation == "gym" else _lib.OBS_RAW,
                                  _lib.POLICY_GREEDY if greedy else 0)
        buffers = _lib.RolloutBuffers(*[tensor.data_ptr() for tensor in out], t)
        _lib.check(self._L.mrl_rollout_policy(self._handle, ctypes.byref(desc), ctypes.byref(buffers),
                                              int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(self.gpu_id)))
        return out

    def rollout_cnn(self, policy, record, obs_ring, players=None, seed=0, first_step=0, greedy=False):
        """``record.num_steps`` steps under ``policy`` (a ``CnnPolicy``) for the seats in ``players`` with the host out of the loop
        (``mrl_rollout_cnn``; Overcooked and Simplecooked): ``obs_ring`` is int8 (T + 1, N, P, H, W, F), contiguous; slot 0 receives the current
        observations, the act of step k reads slot k and the step writes slot k + 1.  Afterwards the observation output is what
        it was before and holds slot T, the observations of the state the simulator is in: the next act or rollout goes on from
        there.  ``greedy`` travels in the policy descriptor's flags.  The draw of (step index ``first_step + k``, world, seat) is ``random_hash``'s."""
        mask = _cnn_call_args(self, policy, players, record)
        if record is None:
            raise ValueError("rollout_cnn needs a CnnRecord")
        want = (record.num_steps + 1,) + tuple(self.observation_world_major_tensor().shape)
        if (not isinstance(obs_ring, torch.Tensor) or not obs_ring.is_cuda or obs_ring.device.index != self.gpu_id or
                obs_ring.dtype not in (torch.int8, torch.uint8) or tuple(obs_ring.shape) != want or not obs_ring.is_contiguous()):
            raise ValueError(f"obs_ring must be a contiguous int8 tensor of shape {want} on cuda:{self.gpu_id}")
        desc = policy.desc()
        desc.flags = _lib.POLICY_GREEDY if greedy else 0
        _lib.check(self._L.mrl_rollout_cnn(self._handle, mask, ctypes.byref(desc), ctypes.byref(record.struct), obs_ring.data_ptr(),
                                           int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(self.gpu_id)))

    def rollout_cnn_bank(self, bank, ids, record, obs_ring, episodes=None, resample=None, ids_record=None, players=None, seed=0,
                         first_step=0, greedy=False, workspace=None):
        """``rollout_cnn`` with ``cnn_act_bank`` in place of ``cnn_act`` (``mrl_rollout_cnn_bank``): ``ids`` int32 (N, P) assigns a
        row of ``bank`` (a ``CnnPolicyBank``) to every cell; with ``resample`` (a ``CnnResample``) ``cnn_resample`` runs behind every
        step on ``ids`` and ``episodes`` (int32 (N)); ``ids_record`` int32 (T + 1, N, P) receives the ids each act used.  No host
        wait inside; two rollouts of T equal one of 2 T, ``ids`` and ``episodes`` included."""
        mask = _cnn_bank_call_args(self, bank, ids, players, record)
        if record is None:
            raise ValueError("rollout_cnn_bank needs a CnnRecord")
        cells = tuple(self.observation_world_major_tensor().shape)
        want = (record.num_steps + 1,) + cells
        if (not isinstance(obs_ring, torch.Tensor) or not obs_ring.is_cuda or obs_ring.device.index != self.gpu_id or
                obs_ring.dtype not in (torch.int8, torch.uint8) or tuple(obs_ring.shape) != want or not obs_ring.is_contiguous()):
            raise ValueError(f"obs_ring must be a contiguous int8 tensor of shape {want} on cuda:{self.gpu_id}")
        _check_bank_rollout(self, record, cells[:2], ids_record, resample, episodes)
        if workspace is None:
            workspace = _cnn_bank_workspace(self, bank)
        desc = bank.desc()
        desc.flags = _lib.POLICY_GREEDY if greedy else 0
        _lib.check(self._L.mrl_rollout_cnn_bank(
            self._handle, mask, ctypes.byref(desc), ids.data_ptr(), episodes.data_ptr() if episodes is not None else None,
            ctypes.byref(resample.struct) if resample is not None else None, ctypes.byref(record.struct),
            ids_record.data_ptr() if ids_record is not None else None, obs_ring.data_ptr(), int(seed) & (2 ** 64 - 1),
            int(first_step) & 0xFFFFFFFF, workspace.data_ptr(), workspace.numel(), _stream_ptr(self.gpu_id)))

    def rollout_mlpbase(self, policy, record, players=None, seed=0, first_step=0, greedy=False):
        """``record.num_steps`` steps under ``policy`` (an ``MlpBasePolicy``) for the seats in ``players`` with the host out of the
        loop (``mrl_rollout_mlpbase``; the balance beam): the act of step k reads OBSERVATION in place and copies its rows into
        ``record.obs[k]``, the closing value-only act fills row T.  ``greedy`` travels in the policy descriptor's flags.  The draw
        of (step index ``first_step + k``, world, seat) is ``random_hash``'s."""
        mask = _mlpbase_call_args(self, policy, players, record)
        if record is None:
            raise ValueError("rollout_mlpbase needs an MlpBaseRecord")
        desc = policy.desc()
        desc.flags = _lib.POLICY_GREEDY if greedy else 0
        _lib.check(self._L.mrl_rollout_mlpbase(self._handle, mask, ctypes.byref(desc), ctypes.byref(record.struct),
                                               int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(self.gpu_id)))

    def rollout_mlpbase_bank(self, bank, ids, record, episodes=None, resample=None, ids_record=None, players=None, seed=0, first_step=0,
                             greedy=False, workspace=None):
        """``rollout_mlpbase`` with ``mlpbase_act_bank`` in place of ``mlpbase_act`` (``mrl_rollout_mlpbase_bank``): ``ids`` int32
        (N, P) assigns a row of ``bank`` (an ``MlpBasePolicyBank``) to every cell; with ``resample`` (a ``CnnResample``)
        ``mlpbase_resample`` runs behind every step on ``ids`` and ``episodes`` (int32 (N)); ``ids_record`` int32 (T + 1, N, P)
        receives the ids each act used.  No host wait inside; two rollouts of T equal one of 2 T, ``ids`` and ``episodes`` included."""
        mask = _mlpbase_bank_call_args(self, bank, ids, players, record)
        if record is None:
            raise ValueError("rollout_mlpbase_bank needs an MlpBaseRecord")
        _check_bank_rollout(self, record, ids.shape, ids_record, resample, episodes)
        if workspace is None:
            workspace = _mlpbase_bank_workspace(self, bank)
        desc = bank.desc()
        desc.flags = _lib.POLICY_GREEDY if greedy else 0
        _lib.check(self._L.mrl_rollout_mlpbase_bank(
            self._handle, mask, ctypes.byref(desc), ids.data_ptr(), episodes.data_ptr() if episodes is not None else None,
            ctypes.byref(resample.struct) if resample is not None else None, ctypes.byref(record.struct),
            ids_record.data_ptr() if ids_record is not None else None, int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF,
            workspace.data_ptr(), workspace.numel(), _stream_ptr(self.gpu_id)))

    def reset_worlds(self, mask=None):
        """Restart the worlds whose ``mask`` entry is nonzero (``None``: every world) as fresh episodes, enqueued on torch's
        current stream (``mrl_reset_worlds``).  ``mask``: (num_worlds,) of bool, uint8 or any integer type, on any device;
        it is copied into a uint8 buffer on the simulator's device that the simulator keeps.  Hanabi, Cartpole and the
        balance beam number the restarted episodes from their episode counter as if those worlds had finished in a step;
        Overcooked and Simplecooked put them back into the start state.  DONE, REWARD and the other per-step outputs keep
        the last step's values."""
        stream = _stream_ptr(self.gpu_id)
        if mask is None:
            _lib.check(self._L.mrl_reset_worlds(self._handle, None, stream))
            return
        if not isinstance(mask, torch.Tensor):
            mask = torch.as_tensor(mask)
        if mask.dim() != 1 or mask.numel() != self.num_worlds:
            raise ValueError(f"mask must have shape ({self.num_worlds},) (one entry per world), got {tuple(mask.shape)}")
        if mask.dtype.is_floating_point or mask.dtype.is_complex:
            raise ValueError(f"mask must be a bool or integer tensor, got {mask.dtype}")
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask != 0
        if getattr(self, "_reset_mask", None) is None:
            self._reset_mask = torch.empty(self.num_worlds, dtype=torch.uint8, device=torch.device("cuda", self.gpu_id))
        with torch.cuda.device(self.gpu_id):
            self._reset_mask.copy_(mask, non_blocking=True)
        self._reset_mask_source = mask  # a pinned host mask is still read by the copy after this returns
        _lib.check(self._L.mrl_reset_worlds(self._handle, self._reset_mask.data_ptr(), stream))

    def step_phase1(self, actions=None):
        ptr = self._action_pointer(actions) if actions is not None else None
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_step_phase1(self._handle, ptr, stream))

    def _word_pointer(self, words, count, what):
        """A caller-owned array of ``count`` 32-bit words the library reads on the device (episode base, gathered
        shard counts): checked here like the action arrays, the C ABI takes a raw pointer."""
        if (not isinstance(words, torch.Tensor) or not words.is_cuda or words.device.index != self.gpu_id or
                words.dtype not in (torch.int32, torch.uint32) or not words.is_contiguous() or words.numel() != count):
            raise ValueError(f"{what} must be a contiguous int32 tensor of {count} element(s) on cuda:{self.gpu_id}")
        return words.data_ptr()

    def step_phase2(self, episode_base=None):
        """``episode_base``: 1-element int32/uint32 CUDA tensor, or None for the
        simulator's own counter."""
        stream = _stream_ptr(self.gpu_id)
        ptr = self._word_pointer(episode_base, 1, "episode_base") if episode_base is not None else None
        _lib.check(self._L.mrl_step_phase2(self._handle, ptr, stream))

    def step_phase2_gathered(self, counts, rank):
        """Phase 2 of rank ``rank`` of a sharded batch: ``counts`` = every rank's SHARD_COUNT of this step (int32 CUDA
        tensor, one element per rank, what an all-gather of ``shard_count_tensor()`` delivers).  The re-seeding launch
        works out its own episode base and advances the simulator's counter (``mrl_step_phase2_gathered``)."""
        if not isinstance(counts, torch.Tensor):
            raise ValueError("counts must be a tensor")
        ptr = self._word_pointer(counts, counts.numel(), "counts")
        _lib.check(self._L.mrl_step_phase2_gathered(self._handle, ptr, int(counts.numel()), int(rank), _stream_ptr(self.gpu_id)))

    def exchange_create(self, num_ranks, rank):
        """This rank's mailbox of the collective-free shard exchange (``mrl_exchange_create``) -> its IPC handle (64 bytes),
        to be handed to every rank."""
        buf = ctypes.create_string_buffer(_lib.IPC_HANDLE_BYTES)
        _lib.check(self._L.mrl_exchange_create(self._handle, int(num_ranks), int(rank), buf))
        return buf.raw

    def exchange_connect(self, handles):
        """``handles``: the IPC handles of all ranks, in rank order (``mrl_exchange_connect``)."""
        blob = b"".join(handles)
        if len(blob) % _lib.IPC_HANDLE_BYTES:
            raise ValueError("handles must be 64 bytes each")
        _lib.check(self._L.mrl_exchange_connect(self._handle, blob))

    def step_exchanged(self, actions=None):
        """One step of a shard whose ranks exchange their finished counts through the mailboxes (``mrl_step_exchanged``):
        phase 1, count + publish, phase 2 polling -- no collective, no host call in between."""
        ptr = None if actions is None else self._action_pointer(actions)
        _lib.check(self._L.mrl_step_exchanged(self._handle, ptr, _stream_ptr(self.gpu_id)))

    def set_observation_output(self, out):
        """Later steps write their observations into ``out`` -- an int8 CUDA tensor of the world-major shape
        (N, P, H, W, F), contiguous, e.g. one slot of a rollout buffer -- instead of the simulator's own tensor; ``None``
        hands the output back (``mrl_set_observation_output``; Overcooked and Simplecooked).  The caller keeps ``out``
        alive while steps that write to it are in flight."""
        if out is None:
            _lib.check(self._L.mrl_set_observation_output(self._handle, None, 0))
            return
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.gpu_id or
                out.dtype not in (torch.int8, torch.uint8) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int8 tensor on cuda:{self.gpu_id}")
        _lib.check(self._L.mrl_set_observation_output(self._handle, out.data_ptr(), out.numel()))

    def prepare_graph_capture(self):
        """Makes this simulator's steps capturable in a HIP graph (``torch.cuda.graph``): Hanabi, Cartpole and the balance beam
        move their launch-to-launch counter state into device memory (``mrl_prepare_graph_capture``; one extra one-thread
        launch per step from then on); nothing to do for Overcooked and Simplecooked.  Call it outside the capture."""
        _lib.check(self._L.mrl_prepare_graph_capture(self._handle, _stream_ptr(self.gpu_id)))

    def set_observation_ring(self, ring):
        """``ring``: an int8 CUDA tensor (T, N, P, H, W, F) whose slots ``ring[s]`` are contiguous -- a rollout buffer.  Step
        number k from this call on writes its observations to ``ring[k % T]``, whether it is a call of its own or step k of
        ``rollout_random`` / ``step_sequence`` (``mrl_set_observation_ring``); ``None`` hands the output back."""
        if ring is None:
            _lib.check(self._L.mrl_set_observation_ring(self._handle, None, 0, 0))
            return
        if (not isinstance(ring, torch.Tensor) or not ring.is_cuda or ring.device.index != self.gpu_id or ring.dim() < 2 or
                ring.dtype not in (torch.int8, torch.uint8) or not ring[0].is_contiguous()):
            raise ValueError(f"ring must be an int8 tensor (T, N, P, H, W, F) on cuda:{self.gpu_id} with contiguous slots")
        _lib.check(self._L.mrl_set_observation_ring(self._handle, ring.data_ptr(), int(ring.stride(0)), int(ring.shape[0])))

    # --- episode returns and lengths on the device (mrl_enable_episode_stats) ---
    def enable_episode_stats(self):
        """From now on every completed step also keeps the worlds' episode returns and lengths, on the device
        (``mrl_enable_episode_stats``: five more tensors, for the rest of the simulator's life; a second call does nothing).
        Call it outside a graph capture."""
        _lib.check(self._L.mrl_enable_episode_stats(self._handle, _stream_ptr(self.gpu_id)))

    def clear_episode_totals(self):
        """Zeroes ``episode_totals_tensor()`` and nothing else (``mrl_clear_episode_totals``); enqueued, no host sync."""
        _lib.check(self._L.mrl_clear_episode_totals(self._handle, _stream_ptr(self.gpu_id)))

    def episode_return_tensor(self): return self._tensor(_lib.STATS_EPISODE_RETURN)  # float32, REWARD's shape
    def episode_steps_tensor(self): return self._tensor(_lib.STATS_EPISODE_STEPS)  # int32, DONE's shape
    def last_episode_return_tensor(self): return self._tensor(_lib.STATS_LAST_RETURN)
    def last_episode_steps_tensor(self): return self._tensor(_lib.STATS_LAST_STEPS)
    def episode_totals_tensor(self): return self._tensor(_lib.STATS_TOTALS)  # float64 (ceil(N / 1024), 2 + players)

    def episode_totals(self):
        """``{"episodes": int, "steps": int, "returns": [float] * players}`` of the episodes finished since the last
        ``clear_episode_totals``: the column sums of ``episode_totals_tensor()``.  The one call here that waits for the GPU."""
        return totals_of(self.episode_totals_tensor().to_torch())

    @property
    def scan_timed_out(self):
        """True once a bounded in-kernel wait has expired (``mrl_scan_timed_out``); every later step raises."""
        return bool(self._L.mrl_scan_timed_out(self._handle))

    def reseed_shard(self, world_offset, num_worlds_total):
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_reseed_shard(self._handle, int(world_offset), int(num_worlds_total), stream))

    def set_episode_counter(self, next_episode):
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_set_episode_counter(self._handle, int(next_episode), stream))

    @property
    def kernel_name(self):
        return self._L.mrl_kernel_name(self._handle).decode()

    @property
    def rollout_kernel_name(self):
        """The kernel the next ``rollout_random`` runs (a persistent one, or the step kernel once per step)."""
        return self._L.mrl_rollout_kernel_name(self._handle).decode()

    @property
    def bytes_per_world_step(self):
        return int(self._L.mrl_bytes_per_world_step(self._handle))

    @property
    def launch_shape(self):
        """(workgroups, threads per workgroup, LDS bytes per workgroup, worlds per wavefront) of the step kernel."""
        out = (ctypes.c_uint32 * 4)()
        _lib.check(self._L.mrl_launch_shape(self._handle, ctypes.byref(out)))
        return tuple(int(v) for v in out)

    @property
    def num_worlds(self):
        return int(self._L.mrl_num_worlds(self._handle))

    def _tensor(self, slot):
        if slot not in self._tensors:
            self._tensors[slot] = Tensor(self, slot)
        return self._tensors[slot]

    def close(self):
        """Destroys the simulator.  Raises ``MrlError`` if one of its steps ran into SCAN_TIMEOUT (the
        results since then carry unspecified episode numbers) -- after freeing it all the same."""
        if getattr(self, "_handle", None) is not None and self._handle.value:
            bad = bool(self._L.mrl_scan_timed_out(self._handle))
            self._L.mrl_destroy(self._handle)
            self._handle = ctypes.c_void_p()
            if bad:
                raise MrlError("an in-kernel wait expired during this simulator's life (SCAN_TIMEOUT): "
                               "episode numbers since then are unspecified")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OvercookedSimulator(_Simulator):
    """Signature of src/overcooked_env/bindings.cpp:14-71."""

    _create = "mrl_overcooked_create"

    def __init__(self, exec_mode, gpu_id, num_worlds, terrain, height, width, num_players, start_player_x,
                 start_player_y, placement_in_pot_rew, dish_pickup_rew, soup_pickup_rew, recipe_values, recipe_times,
                 horizon, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        if len(terrain) < height * width:
            raise ValueError("terrain shorter than height*width")
        if len(start_player_x) < num_players or len(start_player_y) < num_players:
            raise ValueError("fewer start positions than players")
        if len(recipe_values) < 16 or len(recipe_times) < 16:
            raise ValueError("recipe tables need 16 entries")
        keep = [_lib.i64_array(terrain), _lib.i64_array(start_player_x), _lib.i64_array(start_player_y),
                _lib.i64_array(recipe_values), _lib.i64_array(recipe_times)]
        cfg = _lib.OvercookedConfig(int(height), int(width), int(num_players), int(placement_in_pot_rew),
                                    int(dish_pickup_rew), int(soup_pickup_rew), int(horizon), *keep)
        _lib.check(getattr(self._L, self._create)(ctypes.byref(cfg), int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self.num_players, self.height, self.width = int(num_players), int(height), int(width)
        self._action_numel = int(num_players) * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def agent_state_tensor(self): return self._tensor(3)  # alias, bindings.cpp:77
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def location_world_id_tensor(self): return self._tensor(8)
    def location_id_tensor(self): return self._tensor(9)
    # world-major views of this engine (no reference counterpart)
    def observation_world_major_tensor(self): return self._tensor(10)
    def state_players_tensor(self): return self._tensor(11)
    def state_objects_tensor(self): return self._tensor(12)
    def state_timestep_tensor(self): return self._tensor(13)


STEP_MANY_MAX = 8  # simulators per launch (the kernel arguments hold that many parameter blocks: mrl_step_many)


def can_step_with_others(sim):
    """May ``sim`` take part in ``step_many``?  Overcooked simulators whose workgroups share one copy of a world's state
    (a large layout that does not fit one tile, with fewer than 8192 worlds: ``mrl_overcooked_step_team``) step alone."""
    return type(sim) is OvercookedSimulator and "step_team" not in sim.kernel_name


def step_many(sims, actions=None):
    """One launch for several ``OvercookedSimulator``s on one GPU -- any mix of layouts and world counts (``mrl_step_many``).
    ``actions``: None (every simulator's ACTION tensor) or one int32 tensor per simulator (an entry may be None)."""
    if not sims:
        return
    if any(type(s) is not OvercookedSimulator for s in sims):
        raise ValueError("step_many takes OvercookedSimulator instances")
    handles = (ctypes.c_void_p * len(sims))(*[s._handle for s in sims])
    ptrs = None
    if actions is not None:
        if len(actions) != len(sims):
            raise ValueError("one action tensor (or None) per simulator")
        ptrs = (ctypes.c_void_p * len(sims))(*[None if a is None else s._action_pointer(a) for s, a in zip(sims, actions)])
    _lib.check(sims[0]._L.mrl_step_many(handles, len(sims), ptrs, _stream_ptr(sims[0].gpu_id)))


class SimplecookedSimulator(OvercookedSimulator):
    """Signature of src/overcooked2_env/bindings.cpp:14-71 ("Simplecooked": the world the reference's trainer
    uses, train/env_utils.py:3).  Same keyword arguments and tensor getters as ``OvercookedSimulator``; terrain
    values follow overcooked2's enum (tomato source last), rows are 5P + 10 bytes, at most 2 players, 100 cells."""

    _create = "mrl_simplecooked_create"

    def dishes_out_tensor(self): return self._tensor(14)  # WorldState.num_dishes_out, int32 (N)


class HanabiSimulator(_Simulator):
    """Signature of src/hanabi_env/bindings.cpp:10-36."""

    def __init__(self, exec_mode, gpu_id, num_worlds, colors, ranks, players, max_information_tokens,
                 max_life_tokens, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        cfg = _lib.HanabiConfig(int(colors), int(ranks), int(players), int(max_information_tokens),
                                int(max_life_tokens))
        _lib.check(self._L.mrl_hanabi_create(ctypes.byref(cfg), int(gpu_id), int(num_worlds),
                                             ctypes.byref(self._handle)))
        self._action_numel = 2 * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def agent_state_tensor(self): return self._tensor(8)
    def game_tensor(self): return self._tensor(9)
    def reset_count_tensor(self): return self._tensor(10)
    def scan_timeout_tensor(self): return self._tensor(11)
    def shard_count_tensor(self): return self._tensor(12)


class CartpoleSimulator(_Simulator):
    """Signature of src/cartpole_env/bindings.cpp:11-24."""

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_cartpole_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = int(num_worlds)

    def reset_tensor(self): return self._tensor(0)
    def action_tensor(self): return self._tensor(1)
    def observation_tensor(self): return self._tensor(2)
    def reward_tensor(self): return self._tensor(3)
    def world_id_tensor(self): return self._tensor(4)
    def reset_count_tensor(self): return self._tensor(5)
    def scan_timeout_tensor(self): return self._tensor(6)
    def shard_count_tensor(self): return self._tensor(7)


class AcrobotSimulator(_Simulator):
    """Signature of src/acrobat_env/bindings.cpp (``AcrobatSimulator`` there).  ``observation_tensor`` is the raw state
    (theta1, theta2, omega1, omega2); ``episode_length_tensor`` is this engine's per-world episode length (the reference
    keeps one length for all worlds: include/mrl_envs.h)."""

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_acrobot_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = int(num_worlds)

    def reset_tensor(self): return self._tensor(0)
    def action_tensor(self): return self._tensor(1)
    def observation_tensor(self): return self._tensor(2)
    def reward_tensor(self): return self._tensor(3)
    def world_id_tensor(self): return self._tensor(4)
    def reset_count_tensor(self): return self._tensor(5)
    def scan_timeout_tensor(self): return self._tensor(6)
    def shard_count_tensor(self): return self._tensor(7)
    def episode_length_tensor(self): return self._tensor(8)


AcrobatSimulator = AcrobotSimulator  # the reference's binding name


class BalanceBeamSimulator(_Simulator):
    """Signature of src/balance_beam_env/bindings.cpp:10-24."""

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_balance_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = 2 * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def agent_state_tensor(self): return self._tensor(3)  # alias, bindings.cpp:29
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def reset_count_tensor(self): return self._tensor(8)
    def shard_count_tensor(self): return self._tensor(9)


def random_balance_action(seed, step, world, player):
    """Balance beam: ``(hash * 4) >> 32`` for (step index, world, player)."""
    import numpy as np
    return ((random_hash(seed, step, world, player).astype(np.uint64) * np.uint64(4)) >> np.uint64(32)).astype(np.int32)
