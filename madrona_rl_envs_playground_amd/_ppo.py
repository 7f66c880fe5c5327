"""PPO for the small MLP actor-critic of Cartpole and Acrobot -- the policy, its rollout on the device, GAE and the update -- and
what the other learners take from it: ``Rollout``, ``gae``, ``_AdamState``, ``_run_update``, ``PpoResult`` and the two helpers that
read an agent made of ``Sequential(Linear, activation, ...)``.  Every name here is also ``simulators``'.

May import: _lib, _device, torch.
"""
import collections
import ctypes

import torch

from . import _lib
from ._device import _require_tensors, _stream_ptr


def _layer_shapes(agent, name, activation, layers):
    """[(in_features, out_features)] of the ``layers`` Linear layers of ``agent.<name>``, which must be ``Sequential(Linear,
    activation, ..., Linear)`` with biases; ValueError otherwise (``MlpPolicy``: Tanh and 3, ``WidePolicy``: ReLU and 4)"""
    nn, net, length = torch.nn, getattr(agent, name, None), 2 * layers - 1
    if (not isinstance(net, nn.Sequential) or len(net) != length or not all(isinstance(net[i], nn.Linear) for i in range(0, length, 2)) or
            not all(isinstance(net[i], activation) for i in range(1, length, 2)) or any(net[i].bias is None for i in range(0, length, 2))):
        form = f", {activation.__name__}, ".join(["Linear"] * layers)
        raise ValueError(f"agent.{name} must be Sequential({form}) with biases")
    return [(net[i].in_features, net[i].out_features) for i in range(0, length, 2)]


def _critic_then_actor(agent):
    """``agent``'s parameters as one flat tensor, the critic's and then the actor's: the order of ``MlpPolicy``'s and
    ``WidePolicy``'s ``params``"""
    return torch.cat([p.detach().reshape(-1) for net in (agent.critic, agent.actor) for p in net.parameters()])


def _aliased(module, params):
    """``module`` with its parameters, in their own order, as VIEWS into the flat tensor ``params`` (``_FlatPolicy``'s actor then
    critic, ``WidePolicy``'s critic then actor: the order of the flat array)"""
    at = 0
    for p in module.parameters():
        p.data = params[at:at + p.numel()].view(p.shape)
        at += p.numel()
    assert at == params.numel()
    return module


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
    (the simulator's STATE row, D = 4), "gym" (Acrobot's six values, D = 6) or "beam" (the balance beam's seat-0 row, D = 7
    with 4 actions and nothing else: the agent of scripts/balance_train_single.py)."""

    _OBS_MODES = {"state": _lib.OBS_RAW, "gym": _lib.OBS_ACROBOT_GYM, "beam": _lib.OBS_BALANCE}

    def __init__(self, obs_dim, num_actions, hidden=64, observation="state", device="cuda:0"):
        if observation not in self._OBS_MODES:
            raise ValueError(f"observation must be 'state', 'gym' or 'beam', got {observation!r}")
        self.obs_dim, self.num_actions, self.hidden, self.observation = int(obs_dim), int(num_actions), int(hidden), observation
        if observation == "beam" and (self.obs_dim, self.num_actions, self.hidden) != (7, 4, 64):
            raise ValueError(f"observation 'beam' takes obs_dim 7, num_actions 4 and hidden 64, got "
                             f"{(self.obs_dim, self.num_actions, self.hidden)}")
        count = int(_lib.lib().mrl_mlp_policy_num_params(self.obs_dim, self.hidden, self.num_actions))
        self.params = torch.zeros(count, dtype=torch.float32, device=torch.device(device))

    @staticmethod
    def _shape_of(agent):
        """(obs_dim, num_actions, hidden) of an agent of the expected form; ValueError otherwise."""
        critic, actor = [_layer_shapes(agent, name, torch.nn.Tanh, 3) for name in ("critic", "actor")]
        d, h = critic[0]
        for shapes, out in ((critic, 1), (actor, actor[2][1])):
            if shapes != [(d, h), (h, h), (h, out)]:
                raise ValueError(f"agent's layers are {shapes}, expected {[(d, h), (h, h), (h, out)]}")
        return d, actor[2][1], h

    _flat = staticmethod(_critic_then_actor)

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


class _PolicyRollout:
    """What ``_Simulator`` inherits of this layer (``self``: a simulator, for ``_L``, ``_handle``, ``gpu_id`` and ``num_worlds``)."""

    def rollout_policy(self, policy, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``num_steps`` steps under ``policy`` (an ``MlpPolicy`` on this GPU) with the host out of the loop: observe, both
        nets, draw, log-prob, value, step and record, two launches per step (``mrl_rollout_policy``; Cartpole, Acrobot and,
        for a policy that observes "beam", the balance beam).  Returns a ``Rollout`` of tensors on this GPU -- new ones, or
        ``out`` (an earlier call's result) filled again.  The draw of (step index ``first_step + k``, world) uses
        ``sample_u``; ``greedy`` takes the first arg-max instead.  On the beam the policy plays seat 0 and seat 1 moves at
        random in the same launch: ``random_balance_action(seed, first_step + k, world, 1)``, whatever ``greedy`` says."""
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
        desc = _lib.MlpPolicyDesc(p.data_ptr(), d, policy.hidden, policy.num_actions, MlpPolicy._OBS_MODES[policy.observation],
                                  _lib.POLICY_GREEDY if greedy else 0)
        buffers = _lib.RolloutBuffers(*[tensor.data_ptr() for tensor in out], t)
        _lib.check(self._L.mrl_rollout_policy(self._handle, ctypes.byref(desc), ctypes.byref(buffers),
                                              int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(self.gpu_id)))
        return out
