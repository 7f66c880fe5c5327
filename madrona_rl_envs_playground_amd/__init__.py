"""MI355X-native batched RL-environment step engine (Overcooked, Hanabi,
Cartpole, balance beam, Acrobot) behind the API of willwng/madrona_rl_envs_playground.

    simulators            OvercookedSimulator / HanabiSimulator / CartpoleSimulator / AcrobotSimulator ... (+ madrona.ExecMode)
                          and every name of the private layers below it, which import one way, each only those above it here:
      _device             torch's current stream as a raw handle, the exported tensors, checks of caller-owned tensors
      _draws              numpy twins of the device's random draws
      _episode_stats      episode returns and lengths on the device, for the env wrappers
      _bank               what the three policy banks share: members, resampling, workspace, cross-play's common parts
      _ppo                the small MLP's PPO (Cartpole, Acrobot); Rollout, gae and the optimiser state every learner shares
      _wide               the wide agent (Hanabi, balance beam): policy, act, bank, update
      _mappo_nets         MAPPO's CNN and MLPBase actor-critics as torch modules
      _mappo              MAPPO's two networks on the device: one act / rollout path for both, the env mixins, the update
      _population         cross_play and MAPPO's update of every member of a bank
    envs                  OvercookedMadrona, HanabiMadrona, CartpoleMadronaTorch/Numpy, AcrobotMadronaTorch/Numpy
    pantheonrl_extension  VectorMultiAgentEnv, MadronaEnv, VectorObservation, VectorAgent
    layouts               Overcooked layout data + get_base_layout_params
    distributed           world sharding over the GPUs of a node, RCCL observation gather

All stepping is done by libmrl_envs.so (csrc/*.hip, gfx950) through the C ABI in
include/mrl_envs.h; importing a simulator without that library raises.
"""
__version__ = "0.1.0"
