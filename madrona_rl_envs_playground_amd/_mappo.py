"""MAPPO's two networks on the device, the kitchens' CNN and the balance beam's MLPBase: the policies, records and banks, ONE act
and rollout path for both (``_Family``: what differs is stated once per network; ``cnn_act``, ``mlpbase_act``, the simulators'
``rollout_*`` and the env mixins are thin callers of ``_act``, ``_act_bank``, ``_rollout`` and ``_rollout_bank``), and the learner
of one policy.  Every name here is also ``simulators``'.

May import: _lib, _device, _bank, _ppo, _mappo_nets, torch.
"""
import collections
import ctypes

import torch

from . import _lib
from ._bank import _PolicyBank, _bank_resample, _bank_rollout_buffers, _bank_workspace, _check_bank_rollout
from ._device import _check_ids, _require_tensors, _seat_mask, _stream_ptr
from ._mappo_nets import CnnActorCritic, MlpBaseActorCritic, MlpBaseGruActorCritic
from ._ppo import Rollout, _AdamState, _aliased, _run_update, gae, minibatch_indices


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
            self._module = _aliased(self._module_class(*[getattr(self, name) for name in self._shape]), self.params)
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


class CnnPolicyBank(_PolicyBank):
    """K ``CnnPolicy`` of one shape in one dense float32 tensor ``params`` (K, num_params) (``mrl_cnn_bank``): row k is exactly
    what a ``CnnPolicy``'s ``params`` is.  ``policy(k)`` is a ``CnnPolicy`` whose ``params`` IS row k, a contiguous view, so
    ``cnn_act``, ``MappoOptimizer``, ``mappo_update`` and ``.module()`` work on a member unchanged and training a member is what the
    next ``cnn_act_bank`` reads.  1 <= K <= 256."""

    _member_class, _shape = CnnPolicy, CnnPolicy._shape

    def __init__(self, width, height, channels, num_policies, hidden=64, num_actions=6, device="cuda:0"):
        self.width, self.height, self.channels, self.hidden, self.num_actions = int(width), int(height), int(channels), int(hidden), int(num_actions)
        super().__init__(num_policies, device)

    def desc(self):
        return _lib.CnnBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.hidden, 0)


def _cnn_bank_workspace(sim, bank):
    seats = sim.observation_world_major_tensor().shape[1]
    return _bank_workspace(sim, "_cnn_bank_workspace", sim._L.mrl_cnn_bank_workspace_bytes(sim.num_worlds, seats, bank.num_policies))


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


class MlpBaseGruState:
    """The running GRU states of a ``MlpBaseGruPolicy`` on a simulator of ``num_worlds`` worlds: ``actor`` and ``critic``, float32
    (N, P, 64), zero at first; the acts read and write them in place (``mrl_mlpbase_gru_policy``'s ``h_actor`` / ``h_critic``).
    ``zero_(worlds=None)`` zeroes every row, or the rows of ``worlds`` (indices or a bool mask over N) -- after ``n_reset``, say;
    episodes that end on their own need nothing: the act masks the state where DONE is set."""

    def __init__(self, num_worlds, device, num_players=2, hidden=_lib.MLPBASE_HIDDEN):
        shape = (int(num_worlds), int(num_players), int(hidden))
        self.num_worlds, self.num_players = shape[0], shape[1]
        self.actor = torch.zeros(shape, dtype=torch.float32, device=torch.device(device))
        self.critic = torch.zeros_like(self.actor)

    def zero_(self, worlds=None):
        for h in (self.actor, self.critic):
            if worlds is None:
                h.zero_()
            else:
                h[worlds] = 0.0
        return self

    def clone(self):
        other = MlpBaseGruState(self.num_worlds, self.actor.device, self.num_players, self.actor.shape[2])
        other.actor.copy_(self.actor)
        other.critic.copy_(self.critic)
        return other


class MlpBaseGruPolicy(MlpBasePolicy):
    """The parameters and the running state ``mrl_mlpbase_act`` runs for the RECURRENT actor-critic (``mrl_mlpbase_gru_policy``,
    ``MRL_MLPBASE_RECURRENT``): ``params`` is the flat tensor of ``parameters_to_vector(MlpBaseGruActorCritic.parameters())`` --
    per net ``base.*`` as in ``MlpBasePolicy``, then the GRU's four tensors and its LayerNorm, then the head: 77 537 floats for
    ``layer_N`` 2, 68 961 for 1.  ``module()`` returns a ``MlpBaseGruActorCritic`` over VIEWS of ``params``.
    ``state(num_worlds)`` makes a zeroed ``MlpBaseGruState`` and BINDS it: ``mlpbase_act``, ``rollout_mlpbase`` and the env's
    ``act`` / ``rollout``, whose signatures are the plain policy's, run on the bound state ``running`` (``bind(state)`` switches
    to another one).  EVERY act and rollout of this policy depends on that binding: callers that share one policy -- a trainer
    and a partner agent, two environments -- must each ``bind`` their own state before each of their calls, or keep a policy
    object each over the same ``params`` (``MlpBasePolicyAgent`` binds its own state for its call and puts the previous one back).
    The banks and ``mappo_update_bank`` do not take a recurrent policy."""

    _module_class, _module_name, _shape = MlpBaseGruActorCritic, "an MlpBaseGruActorCritic", ("layer_N",)
    _desc_flags = _lib.MLPBASE_RECURRENT  # the bit every descriptor of this kind of policy carries, a rollout's included

    def __init__(self, layer_N=2, device="cuda:0"):
        self.running = None
        super().__init__(layer_N=layer_N, device=device)

    @property
    def num_params(self):
        return int(_lib.lib().mrl_mlpbase_policy_num_params(self.obs_dim, self.hidden, self.layer_N + _lib.MLPBASE_GRU_LAYERS, self.num_actions))

    def state(self, num_worlds):
        """A zeroed ``MlpBaseGruState`` on the parameters' device, bound as ``running``."""
        return self.bind(MlpBaseGruState(num_worlds, self.params.device))

    def bind(self, state):
        if not isinstance(state, MlpBaseGruState):
            raise ValueError("state must be an MlpBaseGruState")
        self.running = state
        return state

    def desc(self):
        state = self.running
        if state is None:
            raise ValueError("a recurrent policy acts on a bound state: call policy.state(num_worlds) or policy.bind(state) first")
        plain = _lib.MlpBasePolicyDesc(self.params.data_ptr(), self.hidden, self.layer_N, self._desc_flags)
        return _lib.MlpBaseGruPolicyDesc(plain, state.actor.data_ptr(), state.critic.data_ptr())

    def _act_check(self, worlds, seats, record):
        """what an act or a rollout of a recurrent policy checks beyond the plain one's: the bound state and the record's kind"""
        state = self.running
        if state is None:
            raise ValueError("a recurrent policy acts on a bound state: call policy.state(num_worlds) or policy.bind(state) first")
        _require_tensors([("state.actor", state.actor, torch.float32, worlds * seats * self.hidden),
                          ("state.critic", state.critic, torch.float32, worlds * seats * self.hidden)], self.params.device)
        if tuple(state.actor.shape) != (worlds, seats, self.hidden) or tuple(state.critic.shape) != (worlds, seats, self.hidden):
            raise ValueError(f"the bound state must hold ({worlds}, {seats}, {self.hidden}) rows per net")
        if record is not None and not isinstance(record, MlpBaseGruRecord):
            raise ValueError("a recurrent policy's record must be an MlpBaseGruRecord")

    # what MappoOptimizer and mappo_update ask of a policy
    def _mappo_workspace_bytes(self, minibatch_size, num_minibatches, out, members=None):
        if members is not None:
            raise ValueError("mappo_update_bank does not take a recurrent policy")
        return _lib.lib().mrl_mappo_mlp_workspace_bytes(self.obs_dim, self.hidden, self.layer_N + _lib.MLPBASE_GRU_LAYERS, self.num_actions,
                                                        minibatch_size, num_minibatches, out)

    def _mappo_check(self, record, ring):
        if not isinstance(record, MlpBaseGruRecord):
            raise ValueError("record must be an MlpBaseGruRecord")
        if ring is not None:
            raise ValueError("an MlpBaseGruPolicy's batch is record.obs: ring must be None")

    def _mappo_batch(self, record, ring, count):
        """-> ((entry point, None), policy struct, the batch struct's maker, the batch's observations).  ``indices`` are CHUNK ids
        (``chunk_indices``); the policy struct carries no state: the update starts every chunk from the record's ``h0``."""
        rows = count + count // max(record.num_steps, 1)
        cells = record.num_worlds * record.num_players * self.hidden
        chunks = record.num_steps // record.chunk_length
        _require_tensors([("record.obs", record.obs, torch.int32, rows * self.obs_dim), ("record.dones", record.dones, torch.float32, count),
                          ("record.h0_actor", record.h0_actor, torch.float32, chunks * cells),
                          ("record.h0_critic", record.h0_critic, torch.float32, chunks * cells)], self.params.device)
        plain = _lib.MlpBasePolicyDesc(self.params.data_ptr(), self.hidden, self.layer_N, _lib.MLPBASE_RECURRENT)
        shape = _lib.MlpBaseGruPolicyDesc(plain, None, None)

        def batch(*plain_fields):
            return _lib.MappoMlpGruBatch(_lib.MappoMlpBatch(*plain_fields), record.h0_actor.data_ptr(), record.h0_critic.data_ptr(),
                                         record.dones.data_ptr(), record.chunk_length, record.num_worlds, record.num_players)

        return (_lib.lib().mrl_mappo_mlp_update, None), shape, batch, record.obs


class MlpBaseGruRecord(MlpBaseRecord):
    """The buffers of a recurrent act or rollout (``mrl_mlpbase_gru_record``): ``MlpBaseRecord``'s and, for chunks of
    ``chunk_length`` = L steps (the reference's ``data_chunk_length``, default 10; it must divide ``num_steps``), ``h0_actor`` and
    ``h0_critic`` float32 (T / L, N, P, 64): row j holds the states the act at row j L came in with, before its mask -- where the
    update's chunk j starts."""

    def __init__(self, num_steps, num_worlds, num_players, device, chunk_length=10, logits=False):
        self.chunk_length = int(chunk_length)
        if self.chunk_length < 1 or int(num_steps) % self.chunk_length:
            raise ValueError(f"chunk_length {chunk_length} must be at least 1 and divide num_steps {num_steps}")
        super().__init__(num_steps, num_worlds, num_players, device, logits)
        self.struct = _lib.MlpBaseGruRecordDesc(self.struct, self.h0_actor.data_ptr(), self.h0_critic.data_ptr(), self.chunk_length)

    def _own_buffers(self, z, t, n, p):
        super()._own_buffers(z, t, n, p)
        self.h0_actor = z((t // self.chunk_length, n, p, _lib.MLPBASE_HIDDEN))
        self.h0_critic = z((t // self.chunk_length, n, p, _lib.MLPBASE_HIDDEN))

    @property
    def num_chunks(self):
        return self.num_steps // self.chunk_length * self.num_worlds * self.num_players


MlpBaseGruPolicy._record_class = MlpBaseGruRecord


def chunk_indices(record, num_mini_batch, epochs, generator=None, device="cpu"):
    """The rows ``mappo_update`` takes for a recurrent policy, (epochs * num_mini_batch, Bc) int32 CHUNK ids on ``device``: every
    epoch is one permutation of the record's (T / L) N P chunks cut into ``num_mini_batch`` rows, as ``recurrent_generator`` draws
    it (utils/shared_buffer.py; chunk c = (j N + n) P + p covers rows j L .. j L + L - 1 of world n, seat p)."""
    if not isinstance(record, MlpBaseGruRecord):
        raise ValueError("record must be an MlpBaseGruRecord")
    return minibatch_indices(record.num_chunks, num_mini_batch, epochs, generator, device)


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

    def desc(self):
        return _lib.MlpBaseBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.hidden, self.layer_N, 0)


def _mlpbase_bank_workspace(sim, bank):
    return _bank_workspace(sim, "_mlpbase_bank_workspace", sim._L.mrl_mlpbase_bank_workspace_bytes(sim.num_worlds, bank.num_policies))


def _kitchen_cells(sim, policy=None):
    shape = sim.observation_world_major_tensor().shape  # (N, P, H, W, F)
    if policy is not None and (policy.height, policy.width, policy.channels) != tuple(shape[2:]):
        raise ValueError(f"the policy is for a {policy.width} x {policy.height} kitchen with {policy.channels} channels, the simulator's "
                         f"is {shape[3]} x {shape[2]} with {shape[4]} (Overcooked: 5P + 16 channels, Simplecooked: 5P + 10)")
    return shape[0], shape[1]


class _Family:
    """What differs between MAPPO's two networks on the act and rollout side, stated once per network (``_CNN``, ``_MLPBASE``) as
    ``BankFamily`` states it in capi_internal.hpp and the policies' ``_mappo_*`` hooks state it for the update.  ``name`` gives the four
    entry points (``act``, ``act_bank``, ``rollout``, ``rollout_bank``: ``mrl_<name>_act`` ... ``mrl_rollout_<name>_bank``), ``article``
    the nouns of the messages.  ``game``: the marker an act demands of the simulator, ``None`` where it asks only for the shape.
    ``cells(sim, policy=None)`` -> (worlds, seats), after the network's own shape check when there is a policy.  ``act_workspace``:
    (the attribute under which the simulator keeps the act's workspace, its sizer) or ``None`` where the act takes none;
    ``bank_workspace(sim, bank)``.  ``ring``: do the rollouts take an observation ring."""

    def __init__(self, name, article, policy, bank, record, value_only, game, cells, act_workspace, bank_workspace, ring):
        self.policy, self.bank, self.record = policy, bank, record
        self.policy_noun, self.bank_noun, self.record_noun = (f"{article} {cls.__name__}" for cls in (policy, bank, record))
        self.act, self.act_bank, self.rollout, self.rollout_bank = (f"mrl_{name}_act", f"mrl_{name}_act_bank", f"mrl_rollout_{name}",
                                                                    f"mrl_rollout_{name}_bank")
        self.value_only, self.game, self.cells, self.ring = value_only, game, cells, ring
        self.act_workspace, self.bank_workspace = act_workspace, bank_workspace


_CNN = _Family("cnn", "a", CnnPolicy, CnnPolicyBank, CnnRecord, _lib.CNN_VALUE_ONLY, None, _kitchen_cells,
               ("_cnn_workspace", "mrl_cnn_workspace_bytes"), _cnn_bank_workspace, True)
_MLPBASE = _Family("mlpbase", "an", MlpBasePolicy, MlpBasePolicyBank, MlpBaseRecord, _lib.MLPBASE_VALUE_ONLY, "beam",
                   lambda sim, policy=None: tuple(sim.observation_tensor().shape[1::-1]), None, _mlpbase_bank_workspace, False)  # (P, N, 7)


def _call_args(family, sim, policy, players, record):
    """What every act and rollout of either network checks first, in this order: the policy's type, the simulator's game, ``params``,
    the network's own shape, the record -> (seat mask, worlds, seats)"""
    if not isinstance(policy, family.policy):
        raise ValueError(f"policy must be {family.policy_noun}")
    if family.game is not None and getattr(sim, "_game", None) != family.game:
        raise ValueError(f"{family.act} runs on a BalanceBeamSimulator")
    p = policy._check_params(sim.gpu_id)
    worlds, seats = family.cells(sim, policy)
    if record is not None and (not isinstance(record, family.record) or record.num_worlds != worlds or record.num_players != seats or
                               record.actions.device != p.device):
        raise ValueError(f"record must be {family.record_noun} of {worlds} worlds and {seats} players on cuda:{sim.gpu_id}")
    own_check = getattr(policy, "_act_check", None)  # a recurrent policy's: its bound state, its kind of record
    if own_check is not None:
        own_check(worlds, seats, record)
    return _seat_mask(players, seats), worlds, seats


def _bank_call_args(family, sim, bank, ids, players, record):
    """``_call_args`` under a bank: the bank's type, the simulator's game, the bank's ``params``, then member 0 as the policy, then
    ``ids`` -> (seat mask, worlds, seats)"""
    if not isinstance(bank, family.bank):
        raise ValueError(f"bank must be {family.bank_noun}")
    if family.game is not None and getattr(sim, "_game", None) != family.game:
        raise ValueError(f"{family.act_bank} runs on a BalanceBeamSimulator")
    bank._check_params(sim.gpu_id)
    mask, worlds, seats = _call_args(family, sim, bank.policy(0), players, record)
    _check_ids(sim, ids, (worlds, seats), "ids")
    return mask, worlds, seats


def _cnn_call_args(sim, policy, players, record):
    return _call_args(_CNN, sim, policy, players, record)[0]


def _mlpbase_call_args(sim, policy, players, record):
    return _call_args(_MLPBASE, sim, policy, players, record)[0]


def _cnn_bank_call_args(sim, bank, ids, players, record):
    return _bank_call_args(_CNN, sim, bank, ids, players, record)[0]


def _mlpbase_bank_call_args(sim, bank, ids, players, record):
    return _bank_call_args(_MLPBASE, sim, bank, ids, players, record)[0]


def _act(family, sim, policy, players, record, row, seed, step, greedy, value_only, workspace):
    """``cnn_act`` and ``mlpbase_act``: ``family.act`` on torch's current stream of the simulator's device"""
    mask, _, seats = _call_args(family, sim, policy, players, record)
    scratch = ()
    if family.act_workspace is not None:
        if workspace is None:
            attribute, sizer = family.act_workspace
            workspace = getattr(sim, attribute, None)
            if workspace is None:  # made once: its size depends on the simulator alone
                workspace = _bank_workspace(sim, attribute, getattr(sim._L, sizer)(sim.num_worlds, seats))
        scratch = (workspace.data_ptr(), workspace.numel())
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (family.value_only if value_only else 0)
    desc = policy.desc()
    rc = getattr(sim._L, family.act)(sim._handle, mask, _lib.base_ref(desc), _lib.base_ref(record.struct) if record is not None else None,
                                     int(row), int(seed) & (2 ** 64 - 1), int(step) & 0xFFFFFFFF, flags, *scratch, _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


def _act_bank(family, sim, bank, ids, players, record, ids_row, row, seed, step, greedy, value_only, workspace):
    """``cnn_act_bank`` and ``mlpbase_act_bank``: ``family.act_bank`` on torch's current stream of the simulator's device"""
    mask, _, _ = _bank_call_args(family, sim, bank, ids, players, record)
    if ids_row is not None:
        _check_ids(sim, ids_row, ids.shape, "ids_row")
    if workspace is None:
        workspace = family.bank_workspace(sim, bank)
    flags = (_lib.POLICY_GREEDY if greedy else 0) | (family.value_only if value_only else 0)
    desc = bank.desc()
    rc = getattr(sim._L, family.act_bank)(sim._handle, mask, ctypes.byref(desc), ids.data_ptr(),
                                          ctypes.byref(record.struct) if record is not None else None,
                                          ids_row.data_ptr() if ids_row is not None else None, int(row), int(seed) & (2 ** 64 - 1),
                                          int(step) & 0xFFFFFFFF, flags, workspace.data_ptr(), workspace.numel(), _stream_ptr(sim.gpu_id))
    if rc:
        _lib.check(rc)


def _ring_pointer(family, sim, record, obs_ring):
    """``(obs_ring's pointer,)`` once it is the ring a rollout of ``record``'s steps takes; ``()`` for the network without a ring"""
    if not family.ring:
        return ()
    want = (record.num_steps + 1,) + tuple(sim.observation_world_major_tensor().shape)
    if (not isinstance(obs_ring, torch.Tensor) or not obs_ring.is_cuda or obs_ring.device.index != sim.gpu_id or
            obs_ring.dtype not in (torch.int8, torch.uint8) or tuple(obs_ring.shape) != want or not obs_ring.is_contiguous()):
        raise ValueError(f"obs_ring must be a contiguous int8 tensor of shape {want} on cuda:{sim.gpu_id}")
    return (obs_ring.data_ptr(),)


def _rollout(family, sim, policy, record, obs_ring, players, seed, first_step, greedy):
    """``rollout_cnn`` and ``rollout_mlpbase``: ``family.rollout``; ``greedy`` travels in the descriptor's flags"""
    mask, _, _ = _call_args(family, sim, policy, players, record)
    if record is None:
        raise ValueError(f"{family.rollout[4:]} needs {family.record_noun}")
    ring = _ring_pointer(family, sim, record, obs_ring)
    desc = policy.desc()
    # (a recurrent policy's struct begins with the plain one; the bits a kind of policy always carries are the class's)
    getattr(desc, "base", desc).flags = getattr(policy, "_desc_flags", 0) | (_lib.POLICY_GREEDY if greedy else 0)
    _lib.check(getattr(sim._L, family.rollout)(sim._handle, mask, _lib.base_ref(desc), _lib.base_ref(record.struct), *ring,
                                               int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(sim.gpu_id)))


def _rollout_bank(family, sim, bank, ids, record, obs_ring, episodes, resample, ids_record, players, seed, first_step, greedy, workspace):
    """``rollout_cnn_bank`` and ``rollout_mlpbase_bank``: ``family.rollout_bank``; ``greedy`` travels in the descriptor's flags"""
    mask, worlds, seats = _bank_call_args(family, sim, bank, ids, players, record)
    if record is None:
        raise ValueError(f"{family.rollout_bank[4:]} needs {family.record_noun}")
    ring = _ring_pointer(family, sim, record, obs_ring)
    _check_bank_rollout(sim, record, (worlds, seats), ids_record, resample, episodes)
    if workspace is None:
        workspace = family.bank_workspace(sim, bank)
    desc = bank.desc()
    desc.flags = _lib.POLICY_GREEDY if greedy else 0
    _lib.check(getattr(sim._L, family.rollout_bank)(
        sim._handle, mask, ctypes.byref(desc), ids.data_ptr(), episodes.data_ptr() if episodes is not None else None,
        ctypes.byref(resample.struct) if resample is not None else None, ctypes.byref(record.struct),
        ids_record.data_ptr() if ids_record is not None else None, *ring, int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF,
        workspace.data_ptr(), workspace.numel(), _stream_ptr(sim.gpu_id)))


def cnn_act(sim, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False, value_only=False, workspace=None):
    """``mrl_cnn_act`` on torch's current stream of the simulator's device: the seats in ``players`` (a bit mask or an iterable of
    seats; default all) of an Overcooked or Simplecooked simulator act under ``policy`` (a ``CnnPolicy``) on the observations the simulator's
    most recent step wrote, wherever that was; with ``record`` (a ``CnnRecord``) row ``row`` of its buffers is written.
    ``value_only``: the closing act at row T.  ``workspace``: default one the simulator keeps."""
    _act(_CNN, sim, policy, players, record, row, seed, step, greedy, value_only, workspace)


def mlpbase_act(sim, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False, value_only=False):
    """``mrl_mlpbase_act`` on torch's current stream of the simulator's device: the seats in ``players`` (a bit mask or an iterable
    of seats; default both) of a balance-beam simulator act under ``policy`` (an ``MlpBasePolicy``) on the simulator's own
    OBSERVATION tensor; with ``record`` (an ``MlpBaseRecord``) row ``row`` of its buffers is written, the observation rows
    included.  ``value_only``: the closing act at row T."""
    _act(_MLPBASE, sim, policy, players, record, row, seed, step, greedy, value_only, None)


def cnn_act_bank(sim, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False, value_only=False,
                 workspace=None):
    """``mrl_cnn_act_bank`` on torch's current stream: seat p of world n acts under row ``ids[n, p]`` of ``bank`` (a
    ``CnnPolicyBank``) where p is in ``players`` and the id is valid; a cell at -1 keeps its ACTION entry and its record cells.
    The plan, which sorts the cells by policy into tiles of one policy each (one launch up to 2048 cells, three beyond), then
    ``cnn_act``'s kernel body over those tiles: every output is bit for bit ``cnn_act``'s under the cell's policy.  ``ids``: int32 (N, P) on the device;
    ``ids_row``: int32 (N, P) that receives the ids as this act used them (-1 where it did not act).  The other arguments are
    ``cnn_act``'s.  ``workspace``: default one the simulator keeps (``mrl_cnn_bank_workspace_bytes``; its words are in
    include/mrl_envs.h)."""
    _act_bank(_CNN, sim, bank, ids, players, record, ids_row, row, seed, step, greedy, value_only, workspace)


def mlpbase_act_bank(sim, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False, value_only=False,
                     workspace=None):
    """``mrl_mlpbase_act_bank`` on torch's current stream: seat p of world n of a balance-beam simulator acts under row
    ``ids[n, p]`` of ``bank`` (an ``MlpBasePolicyBank``) where p is in ``players`` and the id is valid; a cell at -1 keeps its
    ACTION entry and its record cells, ``record.obs`` included.  The plan (``cnn_act_bank``'s own), then ``mlpbase_act``'s kernel
    body over its tiles: every output is bit for bit ``mlpbase_act``'s under the cell's policy.  ``ids`` and ``ids_row`` are
    ``cnn_act_bank``'s, the other arguments ``mlpbase_act``'s.  ``workspace``: default one the simulator keeps
    (``mrl_mlpbase_bank_workspace_bytes``, which is ``mrl_cnn_bank_workspace_bytes(N, 2, K)``)."""
    _act_bank(_MLPBASE, sim, bank, ids, players, record, ids_row, row, seed, step, greedy, value_only, workspace)


class _MappoRollouts:
    """What ``_Simulator`` inherits of this layer: the rollouts of both networks as methods of every simulator (``self``: the
    simulator; one of the wrong game is refused as the acts refuse it)."""

    def rollout_cnn(self, policy, record, obs_ring, players=None, seed=0, first_step=0, greedy=False):
        """``record.num_steps`` steps under ``policy`` (a ``CnnPolicy``) for the seats in ``players`` with the host out of the loop
        (``mrl_rollout_cnn``; Overcooked and Simplecooked): ``obs_ring`` is int8 (T + 1, N, P, H, W, F), contiguous; slot 0 receives the current
        observations, the act of step k reads slot k and the step writes slot k + 1.  Afterwards the observation output is what
        it was before and holds slot T, the observations of the state the simulator is in: the next act or rollout goes on from
        there.  ``greedy`` travels in the policy descriptor's flags.  The draw of (step index ``first_step + k``, world, seat) is ``random_hash``'s."""
        _rollout(_CNN, self, policy, record, obs_ring, players, seed, first_step, greedy)

    def rollout_cnn_bank(self, bank, ids, record, obs_ring, episodes=None, resample=None, ids_record=None, players=None, seed=0,
                         first_step=0, greedy=False, workspace=None):
        """``rollout_cnn`` with ``cnn_act_bank`` in place of ``cnn_act`` (``mrl_rollout_cnn_bank``): ``ids`` int32 (N, P) assigns a
        row of ``bank`` (a ``CnnPolicyBank``) to every cell; with ``resample`` (a ``CnnResample``) ``cnn_resample`` runs behind every
        step on ``ids`` and ``episodes`` (int32 (N)); ``ids_record`` int32 (T + 1, N, P) receives the ids each act used.  No host
        wait inside; two rollouts of T equal one of 2 T, ``ids`` and ``episodes`` included."""
        _rollout_bank(_CNN, self, bank, ids, record, obs_ring, episodes, resample, ids_record, players, seed, first_step, greedy, workspace)

    def rollout_mlpbase(self, policy, record, players=None, seed=0, first_step=0, greedy=False):
        """``record.num_steps`` steps under ``policy`` (an ``MlpBasePolicy``) for the seats in ``players`` with the host out of the
        loop (``mrl_rollout_mlpbase``; the balance beam): the act of step k reads OBSERVATION in place and copies its rows into
        ``record.obs[k]``, the closing value-only act fills row T.  ``greedy`` travels in the policy descriptor's flags.  The draw
        of (step index ``first_step + k``, world, seat) is ``random_hash``'s."""
        _rollout(_MLPBASE, self, policy, record, None, players, seed, first_step, greedy)

    def rollout_mlpbase_bank(self, bank, ids, record, episodes=None, resample=None, ids_record=None, players=None, seed=0, first_step=0,
                             greedy=False, workspace=None):
        """``rollout_mlpbase`` with ``mlpbase_act_bank`` in place of ``mlpbase_act`` (``mrl_rollout_mlpbase_bank``): ``rollout_cnn_bank``
        without the ring, for a ``bank`` that is an ``MlpBasePolicyBank`` and with ``mlpbase_resample`` behind every step."""
        _rollout_bank(_MLPBASE, self, bank, ids, record, None, episodes, resample, ids_record, players, seed, first_step, greedy, workspace)


def cnn_resample(sim, ids, episodes, mode, first_id, num_ids, players=None, seed=0):
    """``mrl_cnn_bank_resample`` on torch's current stream: where DONE[n] != 0 -- the world has just restarted itself --
    ``episodes[n]`` goes up by one and every seat p of ``players`` with ``ids[n, p] >= 0`` takes its next policy from
    ``[first_id[p], first_id[p] + num_ids[p])``: "robin" the next one round the range, "random" by ``random_hash(seed, episodes[n],
    n, p)`` (``resample_twin`` is the same in numpy).  ``mode`` may also be a ``CnnResample``, which then carries the rest."""
    if getattr(sim, "_game", None) != "kitchen":  # (the marker of an OvercookedSimulator, which a SimplecookedSimulator is)
        raise ValueError(f"mrl_cnn_bank_resample runs on an OvercookedSimulator or a SimplecookedSimulator, not on a {type(sim).__name__}")
    worlds, seats = _CNN.cells(sim)
    _bank_resample(sim, "mrl_cnn_bank_resample", worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed)


def mlpbase_resample(sim, ids, episodes, mode, first_id=None, num_ids=None, players=None, seed=0):
    """``mrl_mlpbase_bank_resample`` on torch's current stream: ``cnn_resample`` on a balance-beam simulator -- the same kernel,
    draws and arguments (``resample_twin`` is the same in numpy).  ``mode`` may also be a ``CnnResample`` (``BankResample``), which
    then carries the rest."""
    if getattr(sim, "_game", None) != "beam":
        raise ValueError("mrl_mlpbase_bank_resample runs on a BalanceBeamSimulator")
    worlds, seats = _MLPBASE.cells(sim)
    _bank_resample(sim, "mrl_mlpbase_bank_resample", worlds, seats, ids, episodes, mode, first_id, num_ids, players, seed)


class _ActsWithMappoPolicy:
    """What the two env mixins below share (``self.sim``, ``static_actions`` and ``num_envs`` are the wrapper's): MAPPO's
    actor-critic on the device, under one policy or under a bank's member per (world, seat).  A mixin names its network
    (``_family``) and the wrapper's attribute that holds the number of seats (``_seats``)."""

    def act(self, policy, players=None, record=None, row=0, seed=0, step=0, greedy=False):
        """The seats in ``players`` (default all) act under ``policy`` (a ``simulators.CnnPolicy`` in a kitchen, a
        ``simulators.MlpBasePolicy`` on the beam) on the device, one launch (``mrl_cnn_act`` / ``mrl_mlpbase_act``): the actions are
        in ``static_actions``, which is returned; with ``record`` (a ``CnnRecord`` / an ``MlpBaseRecord``) row ``row`` also takes
        log-probs, values and the bookkeeping, on the beam the observation rows too.  A kitchen's observations are those of the most
        recent step, also where ``n_step(out=...)`` sent them."""
        _act(self._family, self.sim, policy, players, record, row, seed, step, greedy, False, None)
        return self.static_actions

    def act_bank(self, bank, ids, players=None, record=None, ids_row=None, row=0, seed=0, step=0, greedy=False):
        """``act`` with a policy per (world, seat) cell: seat p of world n acts under row ``ids[n, p]`` of ``bank`` (a
        ``simulators.CnnPolicyBank`` / ``simulators.MlpBasePolicyBank``), cells at -1 keep their actions (``mrl_cnn_act_bank`` /
        ``mrl_mlpbase_act_bank``: the plan and the act, every output bit for bit ``act``'s under the cell's policy).  ``ids``: int32
        (N, P) on the device.  Returns ``static_actions``."""
        _act_bank(self._family, self.sim, bank, ids, players, record, ids_row, row, seed, step, greedy, False, None)
        return self.static_actions

    def _run(self, method, head, num_steps, record, ring, **options):
        """``rollout`` and ``rollout_bank`` of either mixin: the buffers, each made when ``None``, then the simulator's ``method``
        -> (record, in a kitchen the ring, under a bank ``ids_record``)"""
        family, device, seats = self._family, self.static_actions.device, getattr(self, self._seats)
        record_class = getattr(head[0], "_record_class", family.record)  # (a recurrent policy's record carries the chunks' states)
        filled = (record_class._for_rollout(record, num_steps, self.num_envs, seats, device),)
        if family.ring:
            if ring is None:
                ring = torch.empty((int(num_steps) + 1,) + tuple(self.static_world_major_observations.shape), dtype=torch.int8, device=device)
            filled += (ring,)
        if "ids_record" not in options:
            getattr(self.sim, method)(*head, *filled, **options)
            return filled
        ids_record, options["episodes"] = _bank_rollout_buffers(self, num_steps, seats, options.pop("ids_record"), options["episodes"],
                                                                options["resample"])
        getattr(self.sim, method)(*head, *filled, ids_record=ids_record, **options)
        return filled + (ids_record,)


class ActsWithCnnPolicy(_ActsWithMappoPolicy):
    """Mixin of the two kitchen env wrappers (``envs/overcooked_env.py``, ``envs/overcooked2_env.py``; ``self.sim``, ``static_actions``,
    ``static_world_major_observations``, ``num_envs`` and ``num_players`` are the wrapper's): MAPPO's CNN actor-critic on the device."""

    _family, _seats = _CNN, "num_players"

    def rollout(self, policy, num_steps, seed=0, first_step=0, players=None, record=None, ring=None, greedy=False):
        """``num_steps`` steps under ``policy`` without the host in the loop (``mrl_rollout_cnn``) -> (record, ring): a ``CnnRecord``
        and the observation ring (T + 1, N, P, H, W, F) whose slot k is what the act of step k saw.  ``record`` / ``ring``: an
        earlier call's, filled again.  Afterwards the observations of the state reached (slot T) are also where the simulator's output
        pointed before the call -- ``static_world_major_observations`` unless ``n_step(out=...)`` redirected it -- so rollouts chain.  ``simulators.gae(record.rollout(), gamma, gae_lambda)`` gives the advantages."""
        return self._run("rollout_cnn", (policy,), num_steps, record, ring, players=players, seed=seed, first_step=first_step, greedy=greedy)

    def rollout_bank(self, bank, ids, num_steps, episodes=None, resample=None, seed=0, first_step=0, players=None, record=None, ring=None,
                     ids_record=None, greedy=False):
        """``rollout`` under a bank (``mrl_rollout_cnn_bank``) -> (record, ring, ids_record): ``ids_record`` int32 (T + 1, N, P) holds
        the ids each act used (-1 where it did not act).  ``resample`` (a ``simulators.CnnResample``) runs behind every step: worlds
        that have just restarted draw their next policies into ``ids`` and count in ``episodes`` (int32 (N), made when ``None`` and
        then kept by the env as ``bank_episodes``)."""
        return self._run("rollout_cnn_bank", (bank, ids), num_steps, record, ring, episodes=episodes, resample=resample, ids_record=ids_record,
                         players=players, seed=seed, first_step=first_step, greedy=greedy)


class ActsWithMlpBasePolicy(_ActsWithMappoPolicy):
    """Mixin of the balance-beam env wrapper (``envs/balance_beam_env.py``; ``self.sim``, ``static_actions``, ``num_envs`` and
    ``n_players`` are the wrapper's): MAPPO's MLP actor-critic on the device, one policy for the batch or a bank's member per cell."""

    _family, _seats = _MLPBASE, "n_players"

    def rollout(self, policy, num_steps, seed=0, first_step=0, players=None, record=None, greedy=False):
        """``num_steps`` steps under ``policy`` without the host in the loop (``mrl_rollout_mlpbase``) -> an ``MlpBaseRecord``
        whose ``obs[k]`` is what the act of step k saw.  ``record``: an earlier call's, filled again.  Rollouts chain: the next one
        acts on the state this one reached.  ``simulators.mappo_advantages(record)`` gives the advantages."""
        return self._run("rollout_mlpbase", (policy,), num_steps, record, None, players=players, seed=seed, first_step=first_step,
                         greedy=greedy)[0]

    def rollout_bank(self, bank, ids, num_steps, episodes=None, resample=None, seed=0, first_step=0, players=None, record=None,
                     ids_record=None, greedy=False):
        """``rollout`` under a bank (``mrl_rollout_mlpbase_bank``) -> (record, ids_record): ``ids_record``, ``resample`` and
        ``episodes`` are what they are for ``ActsWithCnnPolicy.rollout_bank``; there is no ring."""
        return self._run("rollout_mlpbase_bank", (bank, ids), num_steps, record, None, episodes=episodes, resample=resample,
                         ids_record=ids_record, players=players, seed=seed, first_step=first_step, greedy=greedy)


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
    For an ``MlpBaseGruPolicy`` (the recurrent actor-critic) ``record`` is an ``MlpBaseGruRecord`` and ``indices`` (K, Bc) are CHUNK
    ids (``chunk_indices``): every mean runs over the Bc L samples of the row's chunks, each chunk's forward pass starts from the
    record's ``h0`` and applies ``1 - record.dones`` at every step, and the gradient goes back through the chunk's L steps.
    Not built: active masks, PopArt, ``update_actor=False``, weight decay."""
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
    return _run_update(entry, (_lib.base_ref(shape), ctypes.byref(opt), _lib.base_ref(batch)), indices,
                       (ctypes.byref(cfg), value_norm.state.data_ptr() if value_norm is not None else None), optimizer,
                       len(_lib.MAPPO_STATS), MappoResult, stats, grads)
