"""``OvercookedMadrona`` -- drop-in for /root/reference/envs/overcooked_env.py:18-119.

Same constructor, attributes (``static_actions``, ``static_observations``, ...,
``sim``) and return shapes.  The reference scatters a (P*C, N, 336)-strided
export into a (P*C, N, F) copy with an ``index_put`` on every step and then views
it as (P, N, W, H, F) (overcooked_env.py:92-102); the HIP kernel writes a
world-major (N, P, H, W, F) block directly, so ``get_obs`` only builds views:
``obs[:, p].transpose(1, 2)`` has the same shape, dtype and values.
"""
import numpy as np
import torch

from ..layouts import get_base_layout_params  # noqa: F401  (re-export, reference location)
from ..pantheonrl_extension.vectorenv import VectorMultiAgentEnv
from ..pantheonrl_extension.vectorobservation import VectorObservation
from ..simulators import ActsWithCnnPolicy, ExecMode, OvercookedSimulator, RecordsEpisodeStatistics
from ..spaces import Discrete, MultiBinary

NUM_ACTIONS = 6  # overcooked_ai_py Action.NUM_ACTIONS


class OvercookedMadrona(ActsWithCnnPolicy, RecordsEpisodeStatistics, VectorMultiAgentEnv):

    def __init__(self, layout_name, num_envs, gpu_id, debug_compile=True, use_cpu=False, use_env_cpu=False,
                 ego_agent_idx=0, horizon=400, num_players=None, record_episode_statistics=False):
        self.layout_name = layout_name
        self.base_layout_params = get_base_layout_params(layout_name, horizon, max_num_players=num_players)
        self.width = self.base_layout_params["width"]
        self.height = self.base_layout_params["height"]
        self.num_players = self.base_layout_params["num_players"]
        self.size = self.width * self.height
        self.horizon = horizon

        self.sim = OvercookedSimulator(exec_mode=ExecMode.CPU if use_cpu else ExecMode.CUDA, gpu_id=gpu_id,
                                       num_worlds=num_envs, debug_compile=debug_compile, **self.base_layout_params)

        full_obs_size = self.width * self.height * (5 * self.num_players + 16)
        self.obs_size = full_obs_size
        self.state_size = full_obs_size

        self.static_dones = self.sim.done_tensor().to_torch()
        self.static_active_agents = self.sim.active_agent_tensor().to_torch().to(torch.bool)
        self.static_actions = self.sim.action_tensor().to_torch()
        self.static_observations = self.sim.observation_tensor().to_torch()
        self.static_rewards = self.sim.reward_tensor().to_torch()
        # (N, P, H, W, F) int8, contiguous: what the kernel writes
        self.static_world_major_observations = self.sim.observation_world_major_tensor().to_torch()
        self.static_scattered_active_agents = self.static_active_agents
        self.static_scattered_rewards = self.static_rewards
        self.static_scattered_observations = self.static_observations

        env_device = torch.device("cpu") if use_env_cpu else self.static_dones.device
        super().__init__(num_envs, device=env_device, n_players=self.num_players)

        self.infos = [{}] * self.num_envs
        self._record_episode_statistics(record_episode_statistics)
        self.ego_ind = ego_agent_idx
        self.observation_space = self._setup_observation_space()
        self.share_observation_space = self.observation_space
        self.action_space = Discrete(NUM_ACTIONS)
        # per-player (N, W, H, F) views are persistent: build them once
        self._player_views = [self.static_world_major_observations[:, i].transpose(1, 2)
                              for i in range(self.num_players)]
        # On the simulator's own device ``.to(device)`` hands back the very same tensors: what get_obs / n_step return is
        # then put together once (the per-call host work is what bounds small batches, tools/host_overhead.py)
        self._resident = env_device == self.static_dones.device
        self._obs_parts = [(self.static_active_agents[i], self._player_views[i]) for i in range(self.num_players)]
        self._n_actions = self.static_actions.numel()
        self._redirected_to = 0  # data pointer the simulator's observation output is redirected to (n_step(out=...)), 0 = its own tensor
        self.n_reset()

    def _setup_observation_space(self):
        return MultiBinary(np.array([self.width, self.height, 5 * self.num_players + 16]))

    def to_torch(self, a):
        return a.to(self.device)

    def get_obs(self):
        if self._resident:
            return [VectorObservation(active, view) for active, view in self._obs_parts]
        return [VectorObservation(self.to_torch(active), self.to_torch(view)) for active, view in self._obs_parts]

    def n_step(self, actions, out=None):
        """``out`` (extension, no reference counterpart): an int8 CUDA tensor of shape (N, P, H, W, F) -- one slot of a
        rollout buffer.  The step kernel then writes this step's observations THERE instead of the simulator's own tensor
        and the returned observations are views of ``out``: the per-step clone + insert of the reference's trainer
        (train/MAPPO/main_player.py:245-247, utils/shared_buffer.py:115) disappears, same bytes written.  ``static_observations``
        is not refreshed by such a step."""
        if out is not None:
            if out.shape != self.static_world_major_observations.shape:
                raise ValueError(f"out must have the world-major shape {tuple(self.static_world_major_observations.shape)}, got {tuple(out.shape)}")
            if out.data_ptr() != self._redirected_to:
                self.sim.set_observation_output(out)
                self._redirected_to = out.data_ptr()
        elif self._redirected_to:
            self.sim.set_observation_output(None)
            self._redirected_to = 0
        # (P, N, 1) int64/int32 on any device -> the simulator's int32 action tensor
        if (actions.dtype == torch.int64 and actions.device == self.static_actions.device and actions.is_contiguous() and
                actions.shape == self.static_actions.shape):
            # what the reference's harness passes (randint_like of a long tensor): the step kernel reads it as it is and
            # mirrors it into static_actions, which the reference fills with a copy kernel of its own (overcooked_env.py:107)
            self.sim._step_i64_checked(actions.data_ptr())
        else:
            self.static_actions.copy_(actions.to(self.static_actions.device), non_blocking=True)
            self.sim.step()
        if out is not None:
            obs = [VectorObservation(self.static_active_agents[i], out[:, i].transpose(1, 2)) for i in range(self.num_players)]
            if not self._resident:
                obs = [VectorObservation(self.to_torch(o.active), self.to_torch(o.obs)) for o in obs]
        else:
            obs = self.get_obs()
        if self._resident:
            return obs, self.static_rewards, self.static_dones, self.infos
        return obs, self.to_torch(self.static_rewards), self.to_torch(self.static_dones), self.infos

    # act(policy, ...) and rollout(policy, num_steps, ...): simulators.ActsWithCnnPolicy, shared with envs/overcooked2_env.py

    def n_reset(self, worlds=None):
        """Like the reference (overcooked_env.py:115-116) ``n_reset()`` does not restart
        anything: worlds restart themselves at the horizon inside ``step``.  ``worlds`` (extension): a (num_envs,) bool or
        integer mask; those worlds restart now, at timestep 0 (``sim.reset_worlds``).  Their observations are written where
        the last step wrote them (the ``out`` of ``n_step(out=...)``, if one was given)."""
        if worlds is not None:
            self.sim.reset_worlds(worlds)
        return self.get_obs()

    def close(self, **kwargs):
        self.sim.close()
