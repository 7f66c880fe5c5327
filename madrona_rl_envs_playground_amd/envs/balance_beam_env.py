"""``BalanceMadronaTorch`` -- drop-in for /root/reference/envs/balance_beam_env.py:20-40: the generic
``MadronaEnv`` wrapper over ``BalanceBeamSimulator`` with the reference's spaces (an observation of six
positions in 0..8 -- own and partner history, shifted by BUFFER -- and the steps left) -- and ``BalanceGym``
(:46-79), its single-agent view against a uniformly random partner."""
import torch

from ..pantheonrl_extension.vectoragent import RandomVectorAgent
from ..pantheonrl_extension.vectorenv import MadronaEnv
from ..simulators import ActsWithMlpBasePolicy, BalanceBeamSimulator, ExecMode
from ..spaces import Discrete, MultiDiscrete

NUM_SPACES = 5
VALID_MOVES = [-2, -1, 1, 2]
BUFFER = 2
TIME = 3
SCALE = 0.2


class BalanceMadronaTorch(ActsWithMlpBasePolicy, MadronaEnv):
    """``act``, ``rollout``, ``act_bank`` and ``rollout_bank`` (extensions, ``simulators.ActsWithMlpBasePolicy``): MAPPO's MLP
    actor-critic on the device, under one policy or under a bank's member per (world, seat)."""

    def __init__(self, num_envs, gpu_id, debug_compile=True, use_cpu=False, use_env_cpu=False, record_episode_statistics=False):
        sim = BalanceBeamSimulator(exec_mode=ExecMode.CPU if use_cpu else ExecMode.CUDA, gpu_id=gpu_id,
                                   num_worlds=num_envs, debug_compile=debug_compile)
        device = torch.device("cpu") if use_env_cpu else None
        super().__init__(num_envs, gpu_id, sim, env_device=device, record_episode_statistics=record_episode_statistics)
        self.observation_space = MultiDiscrete([NUM_SPACES + 2 * BUFFER] * 2 * TIME + [TIME])
        self.action_space = Discrete(len(VALID_MOVES))
        self.share_observation_space = self.observation_space

    def close(self, **kwargs):
        self.sim.close()


class BalanceGym:
    """Drop-in for the reference's ``BalanceGym`` (envs/balance_beam_env.py:46-79), the single-agent view of the beam that
    scripts/balance_train_single.py trains on: the ego plays seat 0 of an inner ``BalanceMadronaTorch`` (``self.sim``, as there)
    and a ``RandomVectorAgent`` plays seat 1 with ``torch.randint_like(static_actions[0], high=4)`` from torch's generator.
    ``step(actions)`` takes (N,) actions and returns ``(obs.float(), reward, done, infos)``, ``reset()`` the (N, 7) float32
    observations.  ``record_episode_statistics`` as the other env wrappers have it."""

    # the same for every instance, so they are the class's (and can be read without a GPU)
    single_observation_space = observation_space = MultiDiscrete([NUM_SPACES + 2 * BUFFER] * 2 * TIME + [TIME])
    single_action_space = action_space = Discrete(len(VALID_MOVES))

    def __init__(self, num_envs, gpu_id, debug_compile=True, record_episode_statistics=False):
        self.num_envs = num_envs
        self.sim = BalanceMadronaTorch(num_envs, gpu_id, debug_compile, record_episode_statistics=record_episode_statistics)
        self.sim.add_partner_agent(RandomVectorAgent(lambda: torch.randint_like(self.sim.static_actions[0], high=len(VALID_MOVES))))
        self.episode_stats = self.sim.episode_stats
        self.infos = [{}] * self.num_envs

    def step(self, actions):
        obs, rew, done, info = self.sim.step(actions[:, None])
        return obs.obs.float(), rew, done, info

    def reset(self):
        return self.sim.reset().obs.float()

    def rollout(self, policy, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``num_steps`` steps under ``policy`` (``simulators.MlpPolicy`` with ``observation="beam"``) collected on the device
        (``sim.rollout_policy``, extension).  Returns a ``Rollout`` whose ``obs`` is (T, N, 7) float32.  A stated departure
        from ``step``: on this path the partner's moves come from the replayable hash
        (``random_balance_action(seed, first_step + k, world, 1)``), not from torch's generator; the distribution, uniform
        over the four moves, is the same."""
        if policy.observation != "beam":
            raise ValueError(f"this environment observes 'beam', the policy {policy.observation!r}")
        return self.sim.sim.rollout_policy(policy, num_steps, seed=seed, first_step=first_step, out=out, greedy=greedy)

    def rollout_bank(self, bank, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``rollout`` for the K members of ``bank`` (``simulators.MlpPolicyBank``) on this environment's N = K W worlds, member k
        on worlds ``[k W, (k + 1) W)`` (``sim.rollout_policy_bank``, extension).  Returns a ``Rollout``."""
        if bank.observation != "beam":
            raise ValueError(f"this environment observes 'beam', the bank {bank.observation!r}")
        return self.sim.sim.rollout_policy_bank(bank, num_steps, seed=seed, first_step=first_step, out=out, greedy=greedy)

    def episode_totals(self):
        """``BalanceMadronaTorch.episode_totals`` of the inner environment."""
        return self.sim.episode_totals()

    def clear_episode_totals(self):
        self.sim.clear_episode_totals()

    def close(self, **kwargs):
        self.sim.close()
