"""Agent interface the vector envs drive their partner players through
(/root/reference/pantheonrl_extension/vectoragent.py:9-41)."""
from abc import ABC, abstractmethod

import torch

from .vectorobservation import VectorObservation


class VectorAgent(ABC):
    @abstractmethod
    def get_action(self, obs: VectorObservation, record: bool = True) -> torch.Tensor:
        """Actions for all N worlds given this agent's observation."""

    @abstractmethod
    def update(self, rewards: torch.Tensor, dones: torch.Tensor) -> None:
        """Reward / done feedback for the most recent recorded ``get_action``."""


class RandomVectorAgent(VectorAgent):
    """Calls ``sampler()`` for every action (the reference's random partner)."""

    def __init__(self, sampler):
        self.sampler = sampler

    def get_action(self, obs: VectorObservation, record: bool = True) -> torch.Tensor:
        return self.sampler()

    def update(self, rewards: torch.Tensor, dones: torch.Tensor) -> None:
        return None


class _DevicePolicyAgent(VectorAgent):
    """What the agents that act under a MAPPO policy on the device share: the seat -- ``player_num``, set by
    ``env.add_partner_agent``, or, while that is ``None``, the env's ``ego_ind`` --, the count of draws that numbers the steps and
    an ``update`` that does nothing.  A subclass has ``_check_env()``, which returns the env's simulator or raises ``TypeError``,
    and ``_act(mask)``, its one launch for the seats in ``mask``."""

    def __init__(self, envs, policy, seed=0, greedy=False):
        self.envs, self.policy, self.seed, self.greedy = envs, policy, int(seed), bool(greedy)
        self.player_num = None
        self._draws = 0
        self._sim = self._check_env()

    @property
    def seat(self):
        return self.envs.ego_ind if self.player_num is None else self.player_num

    def get_action(self, obs=None, record=True):
        self._act(1 << self.seat)
        self._draws += 1
        return self.envs.static_actions[self.seat]

    def update(self, rewards, dones):
        return None


class _PopulationSeat:
    """What the population agents of the two networks share, mixed in FRONT of their single-policy agent: the members, the
    resample, ``ids`` and ``episodes`` on the device, ``get_action`` as the bank act and ``update`` as the resample.  A subclass
    names its bank class (``_bank_class``, of ``simulators``) and entry point (``_entry``, for messages), and has ``_num_seats()``
    and ``_bank_calls()`` -> (the bank act, the resample)."""

    def __init__(self, envs, bank, members=None, resample="robin", seed=0, greedy=False):
        from .. import simulators
        if not isinstance(bank, getattr(simulators, self._bank_class)):
            raise TypeError(f"{type(self).__name__} acts through {self._entry}: bank must be a simulators.{self._bank_class}")
        super().__init__(envs, None, seed=seed, greedy=greedy)
        self.bank = bank
        self.members = list(range(bank.num_policies)) if members is None else [int(k) for k in members]
        if not self.members or any(not 0 <= k < bank.num_policies for k in self.members):
            raise ValueError(f"members must name rows 0..{bank.num_policies - 1} of the bank")
        if resample is not None and resample not in simulators.CNN_RESAMPLE_MODES:
            raise ValueError(f"resample must be one of {sorted(simulators.CNN_RESAMPLE_MODES)} or None, got {resample!r}")
        if resample is not None and self.members != list(range(self.members[0], self.members[0] + len(self.members))):
            raise ValueError("with a resample, members must be consecutive rows of the bank: the device draws from a range")
        self.resample = resample
        self.ids = self.episodes = None
        self._resample = None

    def _attach(self):
        from ..simulators import CnnResample
        envs, device = self.envs, self.envs.static_actions.device
        n, p = envs.num_envs, self._num_seats()
        self.ids = torch.full((n, p), -1, dtype=torch.int32, device=device)
        self.ids[:, self.seat] = torch.tensor(self.members, dtype=torch.int32, device=device)[torch.arange(n, device=device) % len(self.members)]
        self.episodes = torch.zeros(n, dtype=torch.int32, device=device)
        if self.resample is not None:
            self._resample = CnnResample(self.resample, self.members[0], len(self.members), p, self.seed)

    def _act(self, mask):
        if self.ids is None:
            self._attach()
        self._bank_calls()[0](self._sim, self.bank, self.ids, mask, seed=self.seed, step=self._draws, greedy=self.greedy)

    def update(self, rewards, dones):
        if self.ids is None:
            self._attach()
        if self._resample is not None:
            self._bank_calls()[1](self._sim, self.ids, self.episodes, self._resample, None, None, players=1 << self.seat)


class CnnPolicyAgent(_DevicePolicyAgent):
    """A player of either kitchen env (``envs.overcooked_env.OvercookedMadrona`` or the Simplecooked one of
    ``envs.overcooked2_env``) that acts under MAPPO's CNN policy on the device: ``get_action`` is ``mrl_cnn_act`` for this
    agent's seat -- ``player_num``, set by ``env.add_partner_agent``, or, while that is ``None``, the env's ``ego_ind`` -- on the
    simulator's own observations, and returns the view ``env.static_actions[seat]``.  ``policy``: a ``simulators.CnnPolicy``;
    ``seed`` seeds the draws, whose step number counts this agent's calls.  ``update`` does nothing.  Any env other than one of
    those two on the GPU is refused with a ``TypeError`` by the constructor: there is no torch fallback.  ``obs`` and
    ``record`` of ``get_action`` are the ``VectorAgent`` protocol's; the kernel reads the simulator's observations itself and this
    agent keeps no buffers."""

    def _check_env(self):
        from ..envs.overcooked2_env import OvercookedMadrona as SimplecookedMadrona
        from ..envs.overcooked_env import OvercookedMadrona
        from ..simulators import OvercookedSimulator
        envs = self.envs
        sim = getattr(envs, "sim", None)  # (SimplecookedSimulator is an OvercookedSimulator)
        if not isinstance(envs, (OvercookedMadrona, SimplecookedMadrona)) or not isinstance(sim, OvercookedSimulator):
            raise TypeError(f"{type(self).__name__} acts through mrl_cnn_act: envs must be an OvercookedMadrona of envs.overcooked_env or of "
                            "envs.overcooked2_env (Simplecooked), got "
                            f"{type(envs).__name__} over {type(sim).__name__}; there is no torch fallback")
        if envs.device.type != "cuda":
            raise TypeError(f"{type(self).__name__} needs the env on the simulator's GPU (cuda:{sim.gpu_id}); got env device {envs.device}")
        return sim

    def _act(self, mask):
        from ..simulators import cnn_act
        cnn_act(self._sim, self.policy, mask, seed=self.seed, step=self._draws, greedy=self.greedy)


class CnnPopulationAgent(_PopulationSeat, CnnPolicyAgent):
    """A partner seat of either kitchen env played by a POPULATION: every world has its own member of ``bank`` (a
    ``simulators.CnnPolicyBank``) and draws a new one when its episode ends -- the per-episode partner sampling that
    ``add_partner_agent``'s docstring describes, per world instead of for the whole batch.  World n starts with
    ``members[n % len(members)]`` (``members``: rows of the bank, default all); ``get_action`` is ``cnn_act_bank`` for this agent's
    seat; ``update(rewards, dones)`` is ``cnn_resample``: where the simulator's DONE is set the world's count in ``episodes`` goes up
    and its member is replaced, ``resample`` "robin" the next of ``members``, "random" one of them by ``random_hash(seed, episode,
    world, seat)``, ``None`` never (``members`` must then be ``range(first, first + num)``, the range the device call draws from).
    ``ids`` (N, P) int32 -- -1 in every other seat's column -- and ``episodes`` (N) int32 live on the device and exist from the
    first call on.  ``CnnPolicyAgent``'s refusals, and no torch fallback."""

    _bank_class, _entry = "CnnPolicyBank", "mrl_cnn_act_bank"

    def _num_seats(self):
        return self.envs.num_players

    def _bank_calls(self):
        from ..simulators import cnn_act_bank, cnn_resample
        return cnn_act_bank, cnn_resample


class MlpBasePolicyAgent(_DevicePolicyAgent):
    """A player of ``envs.balance_beam_env.BalanceMadronaTorch`` that acts under MAPPO's MLP policy on the device -- what the
    reference's ``CentralizedAgent`` does for the partner seat --, the counterpart of ``CnnPolicyAgent``: ``get_action`` is
    ``mrl_mlpbase_act`` for this agent's seat (``player_num``, set by ``env.add_partner_agent``, or, while that is ``None``, the
    env's ``ego_ind``) on the simulator's own observations, and returns the view ``env.static_actions[seat]``.  ``policy``: a
    ``simulators.MlpBasePolicy``, or a ``simulators.MlpBaseGruPolicy`` (recurrent), for which the agent keeps its own
    ``MlpBaseGruState`` in ``state``; ``seed`` seeds the draws, whose step number counts this agent's calls.  ``update`` does nothing.
    Any other env, or one off the GPU, is refused with a ``TypeError`` by the constructor: there is no torch fallback."""

    def _check_env(self):
        from ..envs.balance_beam_env import BalanceMadronaTorch
        from ..simulators import BalanceBeamSimulator
        envs = self.envs
        sim = getattr(envs, "sim", None)
        if not isinstance(envs, BalanceMadronaTorch) or not isinstance(sim, BalanceBeamSimulator):
            raise TypeError(f"{type(self).__name__} acts through mrl_mlpbase_act: envs must be a BalanceMadronaTorch, got "
                            f"{type(envs).__name__} over {type(sim).__name__}; there is no torch fallback")
        if envs.device.type != "cuda":
            raise TypeError(f"{type(self).__name__} needs the env on the simulator's GPU (cuda:{sim.gpu_id}); got env device {envs.device}")
        return sim

    def _act(self, mask):
        from ..simulators import MlpBaseGruPolicy, MlpBaseGruState, mlpbase_act
        if isinstance(self.policy, MlpBaseGruPolicy):
            # a recurrent policy: this agent owns the state its seat runs on (``state``, zero at first; the act masks it where an
            # episode has just ended), binds it for this call alone and puts back what was bound before, so one policy may serve
            # several agents and a trainer besides: none of them finds another's state bound
            if getattr(self, "state", None) is None:
                self.state = MlpBaseGruState(self.envs.num_envs, self.envs.static_actions.device)
            bound_before = self.policy.running
            self.policy.bind(self.state)
            try:
                mlpbase_act(self._sim, self.policy, mask, seed=self.seed, step=self._draws, greedy=self.greedy)
            finally:
                self.policy.running = bound_before
            return
        mlpbase_act(self._sim, self.policy, mask, seed=self.seed, step=self._draws, greedy=self.greedy)


class MlpBasePopulationAgent(_PopulationSeat, MlpBasePolicyAgent):
    """A partner seat of ``envs.balance_beam_env.BalanceMadronaTorch`` played by a POPULATION, the counterpart of
    ``CnnPopulationAgent``: every world has its own member of ``bank`` (a ``simulators.MlpBasePolicyBank``) and draws a new one
    when its episode ends.  World n starts with ``members[n % len(members)]`` (``members``: rows of the bank, default all);
    ``get_action`` is ``mlpbase_act_bank`` for this agent's seat; ``update(rewards, dones)`` is ``mlpbase_resample``: where the
    simulator's DONE is set the world's count in ``episodes`` goes up and its member is replaced, ``resample`` "robin" the next of
    ``members``, "random" one of them by ``random_hash(seed, episode, world, seat)``, ``None`` never (with a resample ``members``
    must be ``range(first, first + num)``, the range the device call draws from).  ``ids`` (N, P) int32 -- -1 in the other seat's
    column -- and ``episodes`` (N) int32 live on the device and exist from the first call on.  ``MlpBasePolicyAgent``'s refusals:
    any other env gets a ``TypeError``, and there is no torch fallback."""

    _bank_class, _entry = "MlpBasePolicyBank", "mrl_mlpbase_act_bank"

    def _num_seats(self):
        return self.envs.n_players

    def _bank_calls(self):
        from ..simulators import mlpbase_act_bank, mlpbase_resample
        return mlpbase_act_bank, mlpbase_resample


class WidePolicyAgent(_DevicePolicyAgent):
    """A FROZEN player of a Hanabi or balance-beam env under the wide policy -- ``CleanPPOAgent``'s two 512-wide networks -- on the
    device: ``get_action`` is ``mrl_agent_act`` without a record for this agent's seat (``player_num``, set by
    ``env.add_partner_agent``, or, while that is ``None``, the env's ``ego_ind``) on the simulator's own tensors, and returns the
    view ``env.static_actions[seat]``; worlds where it is not this seat's turn get action 0.  ``policy``: a
    ``simulators.WidePolicy``; ``seed`` seeds the draws, whose step number counts this agent's calls.  ``update`` does nothing: a
    partner that learns is a ``CleanPPOAgent``.  The agent owns its workspace.  ``envs`` must be a ``MadronaEnv`` over a Hanabi or
    balance-beam simulator on the GPU: ``TypeError`` otherwise, from the constructor; there is no torch fallback."""

    _entry = "mrl_agent_act"

    def _check_env(self):
        from ..simulators import BalanceBeamSimulator, HanabiSimulator
        from .vectorenv import MadronaEnv
        envs = self.envs
        sim = getattr(envs, "sim", None)
        if not isinstance(envs, MadronaEnv) or not isinstance(sim, (HanabiSimulator, BalanceBeamSimulator)):
            raise TypeError(f"{type(self).__name__} acts through {self._entry}: envs must be a MadronaEnv over a HanabiSimulator or a "
                            f"BalanceBeamSimulator, got {type(envs).__name__} over {type(sim).__name__}; there is no torch fallback")
        if envs.device.type != "cuda":
            raise TypeError(f"{type(self).__name__} needs the env on the simulator's GPU (cuda:{sim.gpu_id}); got env device {envs.device}")
        self._workspace = None
        return sim

    def _act(self, mask):
        from .. import _lib
        from ..simulators import agent_act
        if self._workspace is None:
            self._workspace = torch.empty(int(_lib.lib().mrl_agent_workspace_bytes(self._sim.num_worlds)), dtype=torch.uint8,
                                          device=self.envs.static_actions.device)
        agent_act(self._sim, self.seat, self.policy, seed=self.seed, step=self._draws, greedy=self.greedy, workspace=self._workspace)


class WidePopulationAgent(_PopulationSeat, WidePolicyAgent):
    """A partner seat of a Hanabi or balance-beam env played by a POPULATION under the wide policy, the counterpart of
    ``CnnPopulationAgent`` and ``MlpBasePopulationAgent``: every world has its own member of ``bank`` (a
    ``simulators.WidePolicyBank``) and draws a new one when its episode ends -- ``add_partner_agent``'s per-episode partner
    sampling, per world.  World n starts with ``members[n % len(members)]`` (``members``: rows of the bank, default all);
    ``get_action`` is ``agent_act_bank`` for this agent's seat; ``update(rewards, dones)`` is ``wide_resample``: where the
    simulator's DONE is set the world's count in ``episodes`` goes up and its member is replaced, ``resample`` "robin" the next of
    ``members``, "random" one of them by ``random_hash(seed, episode, world, seat)``, ``None`` never (with a resample ``members``
    must be ``range(first, first + num)``, the range the device call draws from).  ``ids`` (N, P) int32 -- -1 in the other seat's
    column -- and ``episodes`` (N) int32 live on the device and exist from the first call on.  The members are frozen here; train
    one through ``bank.policy(k)``.  ``WidePolicyAgent``'s refusals, and no torch fallback."""

    _bank_class, _entry = "WidePolicyBank", "mrl_agent_act_bank"

    def _num_seats(self):
        return self.envs.n_players

    def _bank_calls(self):
        from ..simulators import agent_act_bank, wide_resample

        def act(sim, bank, ids, mask, seed, step, greedy):
            agent_act_bank(sim, self.seat, bank, ids, seed=seed, step=step, greedy=greedy)

        return act, wide_resample


class CleanPPOAgent(VectorAgent):
    """The reference's PPO agent for Hanabi and the balance beam (/root/reference/pantheonrl_extension/vectoragent.py:116-372;
    built twice, ego and partner, by scripts/hanabi_train.py and scripts/balance_train.py) with its collection phase on the
    device: ``get_action`` is ``mrl_agent_act`` on the simulator's own tensors, ``update`` is ``mrl_agent_credit``, and the
    advantages at the update boundary are ``mrl_gae_active`` -- no host synchronisation per step.  The learning phase is the
    reference's, in torch autograd, on ``policy.module()``, whose parameters are views of the flat tensor the kernels read --
    or, after ``agent.device_update = True`` (extension; an attribute and not a constructor argument, because the constructor
    keeps the reference's signature), ``mrl_agent_update``: the epochs run on the device over the record as it stands (no
    boolean-mask indexing, no float copies of the rows), ``optimizer`` is a ``simulators.WideOptimizer`` and the update waits
    for the device once, to read the losses (once per epoch with ``target_kl``, the reference's own host read).  Assign it
    before the first update: the assignment builds a new optimizer, whose moments start at zero.

    Constructor arguments and defaults are the reference's; ``seed`` (extension) seeds the action draws and defaults to a value
    derived from ``name``.  ``envs`` must be a ``MadronaEnv`` over a Hanabi or balance-beam simulator on the GPU (checked at the
    first ``get_action``: ``TypeError`` otherwise; there is no torch fallback).  The agent's seat is ``player_num`` -- set by
    ``env.add_partner_agent(agent, player_num)`` -- or, while that is ``None``, the env's ``ego_ind``.

    Differences from the reference that a caller can see: the per-step ``torch.any(dones)`` is gone, so episode returns are read
    once per update from device totals (``episode_stats``: count, mean, min and max over the episodes that finished since the last
    update, where the reference averaged per-step means); worlds where this agent is not the one to act get action 0."""

    def __init__(self, envs, name, device, num_updates, verbose=True, lr=2.5e-4, num_steps=128, anneal_lr=True, gamma=0.99,
                 gae_lambda=0.95, num_minibatches=4, update_epochs=4, norm_adv=True, clip_coef=0.2, clip_vloss=True, ent_coef=0.01,
                 vf_coef=0.5, max_grad_norm=0.5, target_kl=None, seed=None):
        import time
        import zlib

        import numpy as np

        from ..simulators import WideAgent, WidePolicy
        self.envs, self.num_envs, self.name, self.device, self.verbose = envs, envs.num_envs, name, torch.device(device), verbose
        self.lr, self.num_steps, self.anneal_lr, self.gamma, self.gae_lambda = lr, num_steps, anneal_lr, gamma, gae_lambda
        self.num_minibatches, self.update_epochs, self.norm_adv = num_minibatches, update_epochs, norm_adv
        self.clip_coef, self.clip_vloss, self.ent_coef, self.vf_coef = clip_coef, clip_vloss, ent_coef, vf_coef
        self.max_grad_norm, self.target_kl = max_grad_norm, target_kl
        self.batch_size = int(self.num_envs * self.num_steps)
        self.minibatch_size = int(self.batch_size // self.num_minibatches)
        self.seed = zlib.crc32(str(name).encode()) if seed is None else int(seed)
        self.player_num = None

        self.writer = None
        if self.verbose:
            try:
                from torch.utils.tensorboard import SummaryWriter
                self.writer = SummaryWriter(f"runs/{name}")
            except ImportError:  # tensorboard is optional here
                self.writer = None

        obs_dim = int(np.prod(envs.observation_space.shape))
        state_dim = int(np.prod(envs.share_observation_space.shape))
        self.policy = WidePolicy.from_module(WideAgent(obs_dim, state_dim, envs.action_space.n, orthogonal=True), device=self.device)
        self.agent = self.policy.module()
        self.optimizer = torch.optim.Adam(self.agent.parameters(), lr=self.lr, eps=1e-5)
        self._device_update = False

        self._obs_dim, self._state_dim = obs_dim, state_dim
        self._sim = self.record = None  # bound at the first get_action / update, where an unsupported env is refused

        self.global_step, self.step, self.updates, self.num_updates = 0, 0, 1, num_updates
        self._draws = 0
        self.start_time = time.time()
        self.episode_stats = {"episodes": 0, "mean": float("nan"), "min": float("nan"), "max": float("nan")}
        self.last_losses = {}

    @property
    def device_update(self):
        """Whether the epochs run on the device (``mrl_agent_update``) and ``optimizer`` is a ``WideOptimizer``; False: torch's."""
        return self._device_update

    @device_update.setter
    def device_update(self, on):
        from ..simulators import WideOptimizer
        if bool(on) == self._device_update:
            return
        self._device_update = bool(on)
        if self._device_update:
            self.optimizer = WideOptimizer(self.policy, lr=self.lr, eps=1e-5)
        else:
            self.optimizer = torch.optim.Adam(self.agent.parameters(), lr=self.lr, eps=1e-5)

    def use_policy(self, policy):
        """(extension) Learn ``policy`` -- a ``simulators.WidePolicy`` of this agent's shape, for example a member of a
        ``WidePolicyBank`` -- in place from now on, instead of the policy the constructor made.  The optimizer starts anew."""
        from ..simulators import WidePolicy
        mine = self.policy
        if not isinstance(policy, WidePolicy) or (policy.obs_dim, policy.state_dim, policy.num_actions) != (mine.obs_dim, mine.state_dim,
                                                                                                           mine.num_actions):
            raise ValueError(f"policy must be a WidePolicy of shape ({mine.obs_dim}, {mine.state_dim}, {mine.num_actions})")
        self.policy, self.agent = policy, policy.module()
        on, self._device_update = self._device_update, not self._device_update
        self.device_update = on  # the setter builds the optimizer of that kind over the new parameters

    def _attach(self):
        self._sim = self._check_env()
        envs = self.envs
        from ..simulators import AgentRecord
        self.record = AgentRecord(self.num_steps, self.num_envs, self._obs_dim, self._state_dim, envs.action_space.n,
                                  envs.static_observations.dtype, envs.static_agent_states.dtype, self.device)

    def _check_env(self):
        from ..simulators import BalanceBeamSimulator, HanabiSimulator
        from .vectorenv import MadronaEnv
        envs = self.envs
        sim = getattr(envs, "sim", None)
        if not isinstance(envs, MadronaEnv) or not isinstance(sim, (HanabiSimulator, BalanceBeamSimulator)):
            raise TypeError("CleanPPOAgent acts through mrl_agent_act: envs must be a MadronaEnv over a HanabiSimulator or a "
                            f"BalanceBeamSimulator, got {type(envs).__name__} over {type(sim).__name__}; there is no torch fallback")
        if envs.device.type != "cuda" or self.device.type != "cuda" or self.device.index not in (None, sim.gpu_id):
            raise TypeError(f"CleanPPOAgent needs the env and the agent on the simulator's GPU (cuda:{sim.gpu_id}); got env device "
                            f"{envs.device} and agent device {self.device}")
        return sim

    @property
    def seat(self):
        return self.envs.ego_ind if self.player_num is None else self.player_num

    def update(self, rewards, dones):
        from ..simulators import agent_credit
        if self.record is None:
            self._attach()
        rewards = rewards.reshape(-1)
        if rewards.dtype != torch.float32 or not rewards.is_contiguous():
            rewards = rewards.to(torch.float32).contiguous()
        dones = dones.reshape(-1)
        if dones.dtype != torch.int32 or not dones.is_contiguous():
            dones = dones.to(torch.int32).contiguous()
        agent_credit(self.record, rewards, dones)
        self.step += 1
        self.global_step += 1

    def get_action(self, obs, record=True):
        from ..simulators import agent_act
        if self.record is None:
            self._attach()
        if self.global_step > 0 and self.global_step % self.num_steps == 0 and record:
            self.step = 0
            self._learn()
        agent_act(self._sim, self.seat, self.policy, self.record if record else None, row=self.step, seed=self.seed,
                  step=self._draws, workspace=self.record.workspace)
        self._draws += 1
        return self.envs.static_actions[self.seat]

    def _learn(self):
        """The update boundary: bootstrap value, advantages (both on the device), then the epochs."""
        from ..simulators import agent_act, gae_active
        r = self.record
        if self.anneal_lr:
            lrnow = (1.0 - (self.updates - 1.0) / self.num_updates) * self.lr
            if self.device_update:
                self.optimizer.lr = lrnow
            else:
                self.optimizer.param_groups[0]["lr"] = lrnow
        agent_act(self._sim, self.seat, self.policy, r, value_only=True)
        advantages, returns = gae_active(r, self.gamma, self.gae_lambda)
        if self.device_update:
            self._learn_device(advantages, returns)
        else:
            self._learn_torch(advantages, returns)

    def _learn_torch(self, advantages, returns):
        """The reference's epochs (:268-330) in torch autograd on the module whose parameters alias ``policy.params``."""
        import numpy as np
        r = self.record
        active = r.active.bool()
        b_obs, b_states = r.obs[active].float(), r.states[active].float()
        b_masks, b_actions = r.action_masks[active].bool(), r.actions[active].long()
        b_logprobs, b_values = r.logprobs[active], r.values[active]
        b_advantages, b_returns = advantages[active], returns[active]
        clipfracs = []
        size = b_values.size(0)
        v_loss = pg_loss = entropy_loss = old_approx_kl = approx_kl = torch.zeros((), device=self.device)
        for _ in range(self.update_epochs if size > 1 else 0):
            inds = torch.randperm(size, device=self.device)  # the reference trains on the whole batch per epoch (:280-283)
            _, newlogprob, entropy, newvalue = self.agent.get_action_and_value(b_obs[inds], b_states[inds], b_masks[inds], b_actions[inds])
            logratio = newlogprob - b_logprobs[inds]
            ratio = logratio.exp()
            with torch.no_grad():
                old_approx_kl = (-logratio).mean()
                approx_kl = ((ratio - 1) - logratio).mean()
                clipfracs.append(((ratio - 1.0).abs() > self.clip_coef).float().mean())
            adv = b_advantages[inds]
            if self.norm_adv:
                adv = (adv - adv.mean()) / (adv.std() + 1e-8)
            pg_loss = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1 - self.clip_coef, 1 + self.clip_coef)).mean()
            newvalue = newvalue.view(-1)
            if self.clip_vloss:
                unclipped = (newvalue - b_returns[inds]) ** 2
                clipped = b_values[inds] + torch.clamp(newvalue - b_values[inds], -self.clip_coef, self.clip_coef)
                v_loss = 0.5 * torch.max(unclipped, (clipped - b_returns[inds]) ** 2).mean()
            else:
                v_loss = 0.5 * ((newvalue - b_returns[inds]) ** 2).mean()
            entropy_loss = entropy.mean()
            loss = pg_loss - self.ent_coef * entropy_loss + v_loss * self.vf_coef
            self.optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(self.agent.parameters(), self.max_grad_norm)
            self.optimizer.step()
            if self.target_kl is not None and approx_kl > self.target_kl:
                break

        # the one host read of the update: losses and the episode totals the credit launches kept
        y_pred, y_true = b_values.cpu().numpy(), b_returns.cpu().numpy()
        var_y = np.var(y_true) if size else 0.0
        episodes, total, low, high = r.episode_totals()
        r.clear_totals()
        if episodes:
            self.episode_stats = {"episodes": episodes, "mean": total / episodes, "min": low, "max": high}
        self.last_losses = {
            "value_loss": float(v_loss.detach()), "policy_loss": float(pg_loss.detach()), "entropy": float(entropy_loss.detach()),
            "old_approx_kl": float(old_approx_kl), "approx_kl": float(approx_kl),
            "clipfrac": float(torch.stack(clipfracs).mean()) if clipfracs else 0.0,
            "explained_variance": float("nan") if var_y == 0 else float(1 - np.var(y_true - y_pred) / var_y),
            "learning_rate": self.optimizer.param_groups[0]["lr"], "samples": size,
        }
        self._log_update(episodes, total, low, high)

    def _learn_device(self, advantages, returns):
        """The epochs as ``mrl_agent_update`` and the update's one host read: the stats rows, the explained variance's three
        sums over the (T, N) arrays and the episode totals travel in one tensor."""
        from .. import _lib
        from ..simulators import agent_update
        r, opt = self.record, self.optimizer
        terms = dict(clip_coef=self.clip_coef, ent_coef=self.ent_coef, vf_coef=self.vf_coef, max_grad_norm=self.max_grad_norm,
                     norm_adv=self.norm_adv, clip_vloss=self.clip_vloss)
        col = {name: i for i, name in enumerate(_lib.AGENT_UPDATE_STATS)}
        if self.target_kl is None:
            rows = agent_update(self.policy, opt, r, advantages, returns, epochs=self.update_epochs, **terms).stats
        else:
            each = []
            for _ in range(self.update_epochs):
                each.append(agent_update(self.policy, opt, r, advantages, returns, epochs=1, **terms).stats)
                status, approx_kl = (float(x) for x in each[-1][0, [col["status"], col["approx_kl"]]].cpu())
                if status != 0 or approx_kl > self.target_kl:
                    break
            rows = torch.cat(each)
        # np.var(y_true) and np.var(y_true - y_pred) over the active cells, as masked sums on the device
        w = r.active.double()
        n = w.sum()
        y_true, diff = returns.double(), returns.double() - r.values.double()
        var = [(((y - (y * w).sum() / n) ** 2) * w).sum() / n for y in (y_true, diff)]
        packed = torch.cat([rows.double().reshape(-1), torch.stack([n] + var), r.totals.reshape(-1)]).cpu()
        rows = packed[:rows.numel()].reshape(rows.shape)
        size, var_y, var_diff = (float(x) for x in packed[rows.numel():rows.numel() + 3])
        totals = packed[rows.numel() + 3:].reshape(r.totals.shape)
        episodes, total, low, high = int(totals[:, 0].sum()), float(totals[:, 1].sum()), float(totals[:, 2].min()), float(totals[:, 3].max())
        r.clear_totals()
        if episodes:
            self.episode_stats = {"episodes": episodes, "mean": total / episodes, "min": low, "max": high}
        done = rows[rows[:, col["status"]] == 0]
        opt.step -= len(rows) - len(done)  # agent_update counted every epoch; those with a status took no step
        last = done[-1] if len(done) else torch.zeros(len(col), dtype=torch.float64)
        self.last_losses = {
            "value_loss": float(last[col["v_loss"]]), "policy_loss": float(last[col["pg_loss"]]), "entropy": float(last[col["entropy"]]),
            "old_approx_kl": float(last[col["old_approx_kl"]]), "approx_kl": float(last[col["approx_kl"]]),
            "clipfrac": float(done[:, col["clipfrac"]].mean()) if len(done) else 0.0,
            "explained_variance": float("nan") if size == 0 or var_y == 0 else float(1 - var_diff / var_y),
            "learning_rate": opt.lr, "samples": int(size),
        }
        self._log_update(episodes, total, low, high)

    def _log_update(self, episodes, total, low, high):
        if self.writer is not None:
            import time
            if episodes:
                self.writer.add_scalar("charts/episodic_return", total / episodes, self.global_step)
                self.writer.add_scalar("charts/min_episodic_return", low, self.global_step)
                self.writer.add_scalar("charts/max_episodic_return", high, self.global_step)
            for key, value in self.last_losses.items():
                group = "charts" if key == "learning_rate" else "losses"
                self.writer.add_scalar(f"{group}/{key}", value, self.global_step)
            self.writer.add_scalar("charts/SPS", int(self.global_step / (time.time() - self.start_time)), self.global_step)
        self.updates += 1
