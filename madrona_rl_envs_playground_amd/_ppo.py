"""PPO for the small MLP actor-critic of Cartpole and Acrobot -- the policy, its rollout on the device, GAE and the update, for one
policy and for the K members of an ``MlpPolicyBank`` on one batch -- and what the other learners take from it: ``Rollout``,
``gae``, ``_AdamState``, ``_run_update``, ``PpoResult`` and the two helpers that read an agent made of ``Sequential(Linear,
activation, ...)``.  Every name here is also ``simulators``'.

May import: _lib, _device, _bank, torch.
"""
import collections
import ctypes

import torch

from . import _lib
from ._bank import _PolicyBank
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


class MlpPolicyBank(_PolicyBank):
    """K ``MlpPolicy`` of one shape in one dense float32 tensor ``params`` (K, P), P = ``mrl_mlp_policy_num_params``: K seeds of the
    small PPO agent.  ``policy(k)`` is an ``MlpPolicy`` whose ``params`` IS row k, a contiguous view, so ``rollout_policy``,
    ``PpoOptimizer`` and ``ppo_update`` work on a member unchanged and in place.  On a simulator of N = K W worlds member k owns
    worlds ``[k W, (k + 1) W)``: ``rollout_policy_bank`` lets every world act under its member's policy in one launch per step,
    ``ppo_update_bank`` steps every member in one call.  1 <= K <= 256; ``observation`` is ``MlpPolicy``'s."""

    _member_class, _shape = MlpPolicy, ("obs_dim", "num_actions", "hidden", "observation")

    def __init__(self, obs_dim, num_actions, num_policies, hidden=64, observation="state", device="cuda:0"):
        self.obs_dim, self.num_actions, self.hidden, self.observation = int(obs_dim), int(num_actions), int(hidden), observation
        super().__init__(num_policies, device)

    def _count_params(self):
        # (an MlpPolicy on no device refuses, in its own words, an observation it does not know and a beam of another shape)
        return MlpPolicy(self.obs_dim, self.num_actions, self.hidden, self.observation, device="meta").params.numel()

    @classmethod
    def from_modules(cls, agents, observation="state", device=None):
        """A bank holding copies of the parameters of ``agents`` (``MlpPolicy.from_module``'s form, all of one shape), in that
        order (``device``: default the first agent's)."""
        agents = list(agents)
        if not agents:
            raise ValueError("from_modules takes a non-empty list of agents")
        shapes = [MlpPolicy._shape_of(agent) for agent in agents]
        if any(shape != shapes[0] for shape in shapes):
            raise ValueError(f"the agents of a bank must have one shape, got (obs_dim, num_actions, hidden) = {sorted(set(shapes))}")
        d, a, h = shapes[0]
        bank = cls(d, a, len(agents), h, observation, device if device is not None else agents[0].critic[0].weight.device)
        for k, agent in enumerate(agents):
            bank.policy(k).load_(agent)
        return bank


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


class PpoBankOptimizer(_AdamState):
    """``PpoOptimizer`` for every member of an ``MlpPolicyBank`` at once: ``exp_avg`` and ``exp_avg_sq`` (K, P), row k the moments
    of bank row k, ONE ``step`` -- every member has taken the same number of Adam steps -- and one ``lr`` (assignable).
    ``member(k)`` is a ``PpoOptimizer`` for ``bank.policy(k)`` whose moments are VIEWS of row k and whose ``step`` is this one's
    at the time of the call: the plain ``ppo_update`` steps that member alone (the bank's ``step`` does not follow)."""

    def __init__(self, bank, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(bank, MlpPolicyBank):
            raise ValueError("bank must be an MlpPolicyBank")
        super().__init__(bank, betas, eps)  # (the moments take bank.params' shape)
        self.bank = bank
        self.lr = float(lr)

    def member(self, k):
        member = PpoOptimizer(self.bank.policy(k), self.lr, self.betas, self.eps)
        member.exp_avg, member.exp_avg_sq, member.step = self.exp_avg[int(k)], self.exp_avg_sq[int(k)], self.step
        return member

    def workspace_bytes(self, minibatch_size, num_minibatches, num_members=1):
        """``num_members`` times ``mrl_ppo_workspace_bytes`` for the bank's shape: a slice per member trained in one call."""
        b = self.bank
        out = ctypes.c_uint64(0)
        _lib.check(_lib.lib().mrl_ppo_workspace_bytes(b.obs_dim, b.hidden, b.num_actions, int(minibatch_size), int(num_minibatches),
                                                      ctypes.byref(out)))
        return int(out.value) * int(num_members)

    def workspace(self, minibatch_size, num_minibatches, num_members=1):
        return self._cached_workspace(self.workspace_bytes(minibatch_size, num_minibatches, num_members))


def member_minibatch_indices(num_steps, num_worlds, num_members, num_minibatches, epochs, generator=None, device="cpu"):
    """The rows ``ppo_update_bank`` takes for a rollout of ``num_steps`` on ``num_worlds`` = N worlds shared by ``num_members`` = K
    members: int32 (K, epochs * num_minibatches, T W // num_minibatches) on ``device``, W = N // K.  Per member and epoch it is
    one ``torch.randperm(T W)`` -- member 0's epochs first, then member 1's -- cut into ``num_minibatches`` rows; entry q of a
    permutation stands for step ``q // W`` of the member's world ``q % W`` and becomes the flat sample number ``t N + k W + j``.
    Every epoch of member k therefore holds exactly member k's samples, each once.  ``generator``: one generator, or a sequence
    of K, member k's own."""
    t, n, k, mb, epochs = int(num_steps), int(num_worlds), int(num_members), int(num_minibatches), int(epochs)
    if t <= 0 or n <= 0 or k <= 0 or n % k:
        raise ValueError(f"num_worlds ({num_worlds}) must be a positive multiple of num_members ({num_members}), num_steps positive")
    w = n // k
    if mb <= 0 or epochs < 0 or (t * w) % mb:
        raise ValueError(f"a member's {t * w} samples (T W) must be a positive multiple of num_minibatches ({num_minibatches}), "
                         f"epochs not negative")
    if t * n >= 2 ** 31:
        raise ValueError("the sample numbers are int32: T N must stay below 2^31")
    generators = list(generator) if isinstance(generator, (list, tuple)) else [generator] * k
    if len(generators) != k:
        raise ValueError(f"generator must be one generator or one per member ({k})")
    out = torch.empty((k, epochs, t * w), dtype=torch.int32, device=device)
    for member, g in enumerate(generators):
        where = g.device if g is not None else torch.device(device)
        for epoch in range(epochs):
            q = torch.randperm(t * w, generator=g, device=where).to(device)
            out[member, epoch] = (q // w) * n + member * w + q % w
    return out.reshape(k, epochs * mb, (t * w) // mb)


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
    head, cfg = _ppo_structs(policy, "policy.params", p, optimizer.exp_avg, optimizer.exp_avg_sq, optimizer, 0, rollout, advantages,
                             returns, indices, clip_coef, ent_coef, vf_coef, max_grad_norm, norm_adv, clip_vloss)
    return _run_update(_lib.lib().mrl_ppo_update, tuple(ctypes.byref(struct) for struct in head), indices, (ctypes.byref(cfg),),
                       optimizer, len(_lib.PPO_STATS), PpoResult, stats, grads)


def _ppo_structs(shape, name, params, exp_avg, exp_avg_sq, optimizer, members, rollout, advantages, returns, indices, clip_coef, ent_coef,
                 vf_coef, max_grad_norm, norm_adv, clip_vloss):
    """What ``ppo_update`` and ``ppo_update_bank`` check and build alike -> ((shape, optimizer, batch), configuration) structs of
    ``mrl_ppo_update``.  ``params`` (called ``name``), ``exp_avg`` and ``exp_avg_sq``: the policy's arrays, or the trained rows
    of a bank's; ``members``: 0, or how many rows."""
    device, f32 = params.device, torch.float32
    count = rollout.values.numel()
    wanted = ((name, params, f32, params.numel()), ("optimizer.exp_avg", exp_avg, f32, params.numel()),
              ("optimizer.exp_avg_sq", exp_avg_sq, f32, params.numel()), ("rollout.obs", rollout.obs, f32, count * shape.obs_dim),
              ("rollout.actions", rollout.actions, torch.int32, count), ("rollout.logprobs", rollout.logprobs, f32, count),
              ("rollout.values", rollout.values, f32, count), ("advantages", advantages, f32, count), ("returns", returns, f32, count),
              ("indices", indices, torch.int32, None))
    _require_tensors(wanted, device)
    head = (_lib.MlpPolicyDesc(params.data_ptr(), shape.obs_dim, shape.hidden, shape.num_actions, 0, 0),
            _lib.PpoOptimizerDesc(params.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), optimizer.step, members),
            _lib.PpoBatch(rollout.obs.data_ptr(), rollout.actions.data_ptr(), rollout.logprobs.data_ptr(), advantages.data_ptr(),
                          returns.data_ptr(), rollout.values.data_ptr(), count))
    cfg = _lib.PpoConfig(clip_coef, ent_coef, vf_coef, max_grad_norm, optimizer.lr, optimizer.betas[0], optimizer.betas[1],
                         optimizer.eps, (_lib.PPO_NORM_ADV if norm_adv else 0) | (_lib.PPO_CLIP_VLOSS if clip_vloss else 0))
    return head, cfg


def ppo_update_bank(bank, optimizer, rollout, advantages, returns, indices, clip_coef=0.2, ent_coef=0.01, vf_coef=0.5,
                    max_grad_norm=0.5, norm_adv=True, clip_vloss=True, stats=True, grads=False, first_member=0):
    """``ppo_update`` for M members of an ``MlpPolicyBank`` in one call (``mrl_ppo_update`` with ``num_members`` = M): one Adam
    step per row for every member, in the plain update's 1 + 3 R launches whatever M is.  ``indices`` is (M, R, B) int32, row m
    the rows of bank row ``first_member + m`` (``member_minibatch_indices``); ``rollout``, ``advantages`` and ``returns`` are
    everyone's -- the record of a ``rollout_policy_bank`` on N worlds and its ``gae``.  ``optimizer`` is the ``PpoBankOptimizer``
    made for ``bank``; its ``step`` grows by R.  For every trained member the parameter row, both moment rows, the stats and the
    grads are bit for bit what ``ppo_update`` leaves for ``bank.policy(k)`` alone with ``indices[m]``; the other rows keep every
    bit.  Returns ``PpoResult(stats, grads)``: (M, R, 8) and (M, R, P), each None unless asked for."""
    if not isinstance(bank, MlpPolicyBank) or not isinstance(optimizer, PpoBankOptimizer) or optimizer.bank is not bank:
        raise ValueError("bank must be an MlpPolicyBank and optimizer the PpoBankOptimizer made for it")
    p = bank.params
    if not p.is_cuda:
        raise ValueError("bank.params must be a contiguous float32 tensor (num_policies, num_params) on a GPU")
    bank._check_params(p.device.index)
    if not isinstance(indices, torch.Tensor) or indices.dim() != 3:
        raise ValueError("indices must be (members, rows, minibatch_size)")
    members, rows, width = indices.shape
    first = int(first_member)
    if members < 1 or first < 0 or first + members > bank.num_policies:
        raise ValueError(f"indices holds the rows of {members} members from member {first_member}; the bank holds members "
                         f"0..{bank.num_policies - 1}")
    for name, moments in (("exp_avg", optimizer.exp_avg), ("exp_avg_sq", optimizer.exp_avg_sq)):
        if not isinstance(moments, torch.Tensor) or moments.shape != p.shape:
            raise ValueError(f"optimizer.{name} must have bank.params' shape")
    trained = slice(first, first + members)
    head, cfg = _ppo_structs(bank, "bank.params", p[trained], optimizer.exp_avg[trained], optimizer.exp_avg_sq[trained], optimizer,
                             members, rollout, advantages, returns, indices, clip_coef, ent_coef, vf_coef, max_grad_norm, norm_adv,
                             clip_vloss)
    workspace = optimizer.workspace(width, rows, members) if width else None
    out_stats = torch.empty((members, rows, len(_lib.PPO_STATS)), dtype=torch.float32, device=p.device) if stats else None
    out_grads = torch.empty((members, rows, bank.num_params), dtype=torch.float32, device=p.device) if grads else None
    gpu = p.device.index
    _lib.check(_lib.lib().mrl_ppo_update(*[ctypes.byref(struct) for struct in head], indices.data_ptr(), rows, width, ctypes.byref(cfg),
                                         workspace.data_ptr() if workspace is not None else None,
                                         workspace.numel() if workspace is not None else 0, out_stats.data_ptr() if stats else None,
                                         out_grads.data_ptr() if grads else None, gpu, _stream_ptr(gpu)))
    optimizer.step += rows
    return PpoResult(out_stats, out_grads)


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
        return self._rollout_mlp(policy, p, 0, num_steps, seed, first_step, out, greedy)

    def rollout_policy_bank(self, bank, num_steps, seed=0, first_step=0, out=None, greedy=False):
        """``rollout_policy`` for the K members of ``bank`` (an ``MlpPolicyBank`` on this GPU) on one batch
        (``mrl_rollout_policy`` with ``num_members`` = K): this simulator's N = K W worlds are K members of W, member k owns worlds
        ``[k W, (k + 1) W)`` and acts under ``bank.policy(k)``; still two launches per step.  Returns a ``Rollout`` whose columns
        ``[k W, (k + 1) W)`` are member k's.  Every cell is bit for bit what ``rollout_policy(bank.policy(k), ...)`` writes for
        that world on the same simulator state: the draws and the episode numbers are those of world w in the batch of N, not
        those of a simulator holding the member's W worlds alone."""
        if not isinstance(bank, MlpPolicyBank):
            raise ValueError("bank must be an MlpPolicyBank")
        bank._check_params(self.gpu_id)
        if bank.num_params != int(self._L.mrl_mlp_policy_num_params(bank.obs_dim, bank.hidden, bank.num_actions)):
            raise ValueError("bank.params' rows do not have mrl_mlp_policy_num_params elements")
        return self._rollout_mlp(bank, bank.params, bank.num_policies, num_steps, seed, first_step, out, greedy)

    def _rollout_mlp(self, policy, p, members, num_steps, seed, first_step, out, greedy):
        """``mrl_rollout_policy`` under checked parameters ``p`` of ``policy``'s shape (a policy's, or with ``members`` a bank's)"""
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
                                  _lib.POLICY_GREEDY if greedy else 0, members)
        buffers = _lib.RolloutBuffers(*[tensor.data_ptr() for tensor in out], t)
        _lib.check(self._L.mrl_rollout_policy(self._handle, ctypes.byref(desc), ctypes.byref(buffers),
                                              int(seed) & (2 ** 64 - 1), int(first_step) & 0xFFFFFFFF, _stream_ptr(self.gpu_id)))
        return out
