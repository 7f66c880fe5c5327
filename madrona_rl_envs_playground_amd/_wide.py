"""The wide agent of Hanabi and the balance beam (the reference's ``CleanPPOAgent``): the policy, its per-player act, its bank
with resampling and cross-play, GAE over the active cells and the update.  Every name here is also ``simulators``'.

May import: _lib, _device, _bank, _ppo, torch.
"""
import ctypes

import torch

from . import _lib
from ._bank import BEAM_TIME, _PolicyBank, _bank_resample, _cross_play_counted
from ._device import _check_ids, _require_tensors, _stream_ptr
from ._ppo import PpoResult, _AdamState, _aliased, _critic_then_actor, _layer_shapes


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
        h = _lib.WIDE_HIDDEN
        for name in ("critic", "actor"):
            shapes = _layer_shapes(agent, name, torch.nn.ReLU, 4)
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
            policy.params.copy_(_critic_then_actor(agent))
        return policy

    def module(self):
        """The ``WideAgent`` whose parameters alias ``params`` (one object per policy)."""
        if self._module is None:
            self._module = _aliased(WideAgent(self.obs_dim, self.state_dim, self.num_actions), self.params)
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

    def desc(self):
        return _lib.WideBankDesc(self.params.data_ptr(), self.num_policies, self.params.stride(0), self.obs_dim, self.state_dim,
                                 self.num_actions)


def _wide_seats(sim, what):
    """(seats, worlds) of a Hanabi or balance-beam simulator; any other is refused"""
    if getattr(sim, "_game", None) not in ("hanabi", "beam"):  # (the marker the game classes carry, subclasses included)
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


def _cross_play_wide(env, bank, members_a, members_b, greedy, seed, steps):
    """``cross_play`` for a ``WidePolicyBank`` on Hanabi or the balance beam"""
    sim = getattr(env, "sim", None)
    if getattr(sim, "_game", None) not in ("hanabi", "beam"):
        raise ValueError("a WidePolicyBank plays Hanabi or the balance beam: env.sim must be a HanabiSimulator or a BalanceBeamSimulator, "
                         f"got {type(sim).__name__}")
    if steps is None:
        if sim._game == "hanabi":
            raise ValueError("steps has no default for Hanabi: a game has no fixed length; give the number of steps to play")
        steps = 4 * BEAM_TIME

    def act(ids, t):
        agent_act_bank(sim, 0, bank, ids, seed=seed, step=t, greedy=greedy)
        agent_act_bank(sim, 1, bank, ids, seed=seed, step=t, greedy=greedy)

    return _cross_play_counted(sim, bank, members_a, members_b, steps, act)


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
