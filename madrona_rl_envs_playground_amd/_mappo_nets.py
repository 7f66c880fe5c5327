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


class _RnnLayer(torch.nn.Module):
    """train/MAPPO/utils/rnn.py for ``recurrent_N`` 1 and ``use_orthogonal``: ``rnn`` = one ``nn.GRU`` layer with orthogonal weights
    and zero biases, ``norm`` = LayerNorm.  ``forward(x, h, mask)`` with x (n, hidden), h (n, hidden) and mask (n) or (n, 1) is one
    step from ``h * mask`` -> (norm(h'), h'); ``chunk(x, h0, masks)`` with x (L, n, hidden) and masks (L, n) runs L such steps,
    masking at every step, which equals the segment logic of rnn.py:41-69 -> (norm of every step's h' (L, n, hidden), h_L)."""

    def __init__(self, hidden):
        super().__init__()
        self.rnn = torch.nn.GRU(hidden, hidden, num_layers=1)
        for name, param in self.rnn.named_parameters():
            if "bias" in name:
                torch.nn.init.constant_(param, 0.0)
            else:
                torch.nn.init.orthogonal_(param)
        self.norm = torch.nn.LayerNorm(hidden)

    def forward(self, x, h, mask):
        out, h = self.rnn(x.unsqueeze(0), (h * mask.reshape(-1, 1)).unsqueeze(0).contiguous())
        return self.norm(out.squeeze(0)), h.squeeze(0)

    def chunk(self, x, h, masks):
        outs = []
        for i in range(x.shape[0]):
            out, h = self.rnn(x[i:i + 1], (h * masks[i].reshape(-1, 1)).unsqueeze(0).contiguous())
            h = h.squeeze(0)
            outs.append(out)
        return self.norm(torch.cat(outs, dim=0)), h


class _MlpBaseGruActor(torch.nn.Module):
    """``R_Actor``'s parameters by name for a vector observation with ``use_recurrent_policy``: ``base...``, ``rnn.rnn.weight_ih_l0``,
    ``weight_hh_l0``, ``bias_ih_l0``, ``bias_hh_l0``, ``rnn.norm``, ``act.action_out.linear``"""

    def __init__(self, obs_dim, hidden, layer_N, num_actions):
        super().__init__()
        self.base = _MlpBase(obs_dim, hidden, layer_N)
        self.rnn = _RnnLayer(hidden)
        self.act = _ActLayer(hidden, num_actions)

    def forward(self, obs, h, mask):
        features, h = self.rnn(self.base(obs), h, mask)
        return self.act.action_out.linear(features), h

    def chunk(self, obs, h0, masks):
        """obs (L, n, 7), h0 (n, hidden), masks (L, n) -> (logits (L, n, actions), h_L)"""
        features, h = self.rnn.chunk(self.base(obs), h0, masks)
        return self.act.action_out.linear(features), h


class _MlpBaseGruCritic(torch.nn.Module):
    """``R_Critic``'s parameters by name with ``use_recurrent_policy``, without PopArt: ``base...``, ``rnn...``, ``v_out``"""

    def __init__(self, obs_dim, hidden, layer_N):
        super().__init__()
        self.base = _MlpBase(obs_dim, hidden, layer_N)
        self.rnn = _RnnLayer(hidden)
        self.v_out = torch.nn.Linear(hidden, 1)

    def forward(self, state, h, mask):
        features, h = self.rnn(self.base(state), h, mask)
        return self.v_out(features), h

    def chunk(self, state, h0, masks):
        """state (L, n, 7), h0 (n, hidden), masks (L, n) -> (values (L, n, 1), h_L)"""
        features, h = self.rnn.chunk(self.base(state), h0, masks)
        return self.v_out(features), h


class MlpBaseGruActorCritic(torch.nn.Module):
    """MAPPO's RECURRENT MLP actor-critic for the balance beam (r_actor_critic.py with ``use_recurrent_policy``, utils/rnn.py with
    ``recurrent_N`` 1): ``MlpBaseActorCritic`` with an ``RNNLayer`` -- one GRU layer of width ``hidden`` and a LayerNorm -- between the
    base and the head of both nets.  ``actor(obs, h, mask)`` / ``critic(obs, h, mask)`` take the (n, 7) observation as floats, the (n,
    hidden) state and the (n) mask (0 where the episode has just ended) and return (logits or value, new state); ``.chunk`` runs L
    steps.  The state dicts have the reference's keys (``rnn.rnn.weight_ih_l0`` ... ``rnn.norm.bias``), so ``load_state_dict`` takes a
    reference checkpoint's two files.  Initialisation is the reference's: the GRU's weights orthogonal and its biases zero
    (rnn.py:14-21), the rest as ``MlpBaseActorCritic``."""

    def __init__(self, layer_N=2, obs_dim=_lib.MLPBASE_OBS, num_actions=_lib.MLPBASE_ACTIONS, hidden=_lib.MLPBASE_HIDDEN):
        super().__init__()
        self.obs_dim, self.num_actions, self.hidden, self.layer_N = int(obs_dim), int(num_actions), int(hidden), int(layer_N)
        self.actor = _MlpBaseGruActor(self.obs_dim, self.hidden, self.layer_N, self.num_actions)
        self.critic = _MlpBaseGruCritic(self.obs_dim, self.hidden, self.layer_N)
        for head, head_gain in ((self.actor.act.action_out.linear, 0.01), (self.critic.v_out, 1.0)):
            torch.nn.init.orthogonal_(head.weight, gain=head_gain)
            torch.nn.init.constant_(head.bias, 0.0)
