"""``AcrobotMadronaTorch`` / ``AcrobotMadronaNumpy`` -- Acrobot-v1 on the reference's ``src/acrobat_env`` world, shaped like
the Cartpole wrappers (``step(actions) -> (obs, rewards, dones, infos)``, ``reset()`` returns the current observations
without restarting anything).  The reference ships the world but no ``envs/`` wrapper for it.

``observation="state"`` (default) returns what the simulator exports, the raw ``(theta1, theta2, omega1, omega2)``;
``observation="gym"`` returns Gym's ``[cos theta1, sin theta1, cos theta2, sin theta2, omega1, omega2]``, computed with
torch from the state tensor (the reference's sim.hpp notes that its state "differs from observation space")."""
from math import pi

import numpy as np
import torch

from ..simulators import AcrobotSimulator, ExecMode, RecordsEpisodeStatistics
from ..spaces import Box, Discrete

MAX_VEL_1 = 4 * pi
MAX_VEL_2 = 9 * pi


class _AcrobotBase(RecordsEpisodeStatistics):
    def __init__(self, num_envs, gpu_id, debug_compile=True, use_cpu=False, use_env_cpu=False, observation="state",
                 record_episode_statistics=False):
        if observation not in ("state", "gym"):
            raise ValueError(f"observation must be 'state' or 'gym', got {observation!r}")
        self.observation = observation
        if observation == "gym":
            high = np.array([1.0, 1.0, 1.0, 1.0, MAX_VEL_1, MAX_VEL_2], dtype=np.float32)
        else:
            high = np.array([pi, pi, MAX_VEL_1, MAX_VEL_2], dtype=np.float32)
        self.num_envs = num_envs
        self.single_action_space = self.action_space = Discrete(3)
        self.single_observation_space = self.observation_space = Box(-high, high, dtype=np.float32)
        self.sim = AcrobotSimulator(exec_mode=ExecMode.CPU if use_cpu else ExecMode.CUDA, gpu_id=gpu_id,
                                    num_worlds=num_envs, debug_compile=debug_compile)
        self.static_dones = self.sim.reset_tensor().to_torch()
        self.static_actions = self.sim.action_tensor().to_torch()
        self.static_observations = self.sim.observation_tensor().to_torch()
        self.static_rewards = self.sim.reward_tensor().to_torch()
        self.device = torch.device("cpu") if use_env_cpu else self.static_observations.device
        self.infos = [{}] * self.num_envs
        self._record_episode_statistics(record_episode_statistics)

    def _observe(self):
        state = self.static_observations
        if self.observation == "state":
            return state
        return torch.stack([torch.cos(state[:, 0]), torch.sin(state[:, 0]), torch.cos(state[:, 1]), torch.sin(state[:, 1]),
                            state[:, 2], state[:, 3]], dim=1)

    def close(self, **kwargs):
        self.sim.close()


class AcrobotMadronaTorch(_AcrobotBase):
    def to_torch(self, a):
        return a.to(self.device)

    def step(self, actions):
        self.static_actions.copy_(actions[:, None].to(self.static_actions.device), non_blocking=True)
        self.sim.step()
        return (self.to_torch(self._observe()), self.to_torch(self.static_rewards),
                self.to_torch(self.static_dones[:, 0]), self.infos)

    def reset(self, worlds=None):
        """The current observations (nothing restarts by itself).  ``worlds``: a (num_envs,) bool or integer mask of
        worlds to restart first, as new episodes (``sim.reset_worlds``)."""
        if worlds is not None:
            self.sim.reset_worlds(worlds)
        return self.to_torch(self._observe())

    def rollout(self, policy, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``num_steps`` steps under ``policy`` (``simulators.MlpPolicy``) collected on the device, observing what this
        environment observes (``sim.rollout_policy``).  Returns a ``Rollout``."""
        if policy.observation != self.observation:
            raise ValueError(f"this environment observes {self.observation!r}, the policy {policy.observation!r}")
        return self.sim.rollout_policy(policy, num_steps, seed=seed, first_step=first_step, out=out, greedy=greedy)

    def rollout_bank(self, bank, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``rollout`` for the K members of ``bank`` (``simulators.MlpPolicyBank``) on this environment's N = K W worlds, member k
        on worlds ``[k W, (k + 1) W)`` (``sim.rollout_policy_bank``, extension).  Returns a ``Rollout``."""
        if bank.observation != self.observation:
            raise ValueError(f"this environment observes {self.observation!r}, the bank {bank.observation!r}")
        return self.sim.rollout_policy_bank(bank, num_steps, seed=seed, first_step=first_step, out=out, greedy=greedy)


class AcrobotMadronaNumpy(_AcrobotBase):
    def step(self, actions):
        self.static_actions.copy_(torch.from_numpy(np.asarray(actions)[:, np.newaxis]))
        self.sim.step()
        return (self._observe().cpu().numpy(), self.static_rewards.cpu().numpy(),
                self.static_dones[:, 0].cpu().numpy(), [{}] * self.num_envs)

    def reset(self, worlds=None):
        """See ``AcrobotMadronaTorch.reset``."""
        if worlds is not None:
            self.sim.reset_worlds(worlds)
        return self._observe().cpu().numpy()
