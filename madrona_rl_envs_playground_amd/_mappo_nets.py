"""MAPPO's two actor-critics as torch modules with the reference's parameter names: the kitchens' CNN and the balance beam's
MLPBase.  No kernel is called from here.  Every name here is also ``simulators``'.

May import: _lib (for the shapes the device path runs), torch.
"""
import copy

import torch

from . import _lib


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


class _ActorCritic(torch.nn.Module):
    """What the two actor-critics below do alike with their ``actor`` and ``critic``"""

    def get_value(self, state):
        return self.critic(state)

    def get_action_and_value(self, obs, action=None, deterministic=False):
        dist = torch.distributions.Categorical(logits=self.actor(obs))
        if action is None:
            action = dist.probs.argmax(dim=-1) if deterministic else dist.sample()
        return action, dist.log_prob(action), dist.entropy(), self.critic(obs)


class CnnActorCritic(_ActorCritic):
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


class MlpBaseActorCritic(_ActorCritic):
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
