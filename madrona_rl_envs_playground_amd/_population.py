"""The top layer under ``simulators``, what works on a whole bank and so stands above every network: ``cross_play``, which
dispatches on the three bank classes, and MAPPO's learner for all members of a bank at once.  Every name here is also
``simulators``'.

May import: _lib, _device, _bank, _ppo, _wide, _mappo, torch.
"""
import ctypes

import torch

from . import _lib
from ._bank import BEAM_TIME, _cross_play_counted, _cross_play_pairs, _cross_play_result
from ._device import _require_tensors, _stream_ptr
from ._mappo import (CnnPolicyBank, MappoOptimizer, MappoResult, MlpBasePolicyBank, ValueNorm, _MappoRecord, _mappo_config,
                     cnn_act_bank, mlpbase_act_bank)
from ._ppo import _AdamState, gae
from ._wide import WidePolicyBank, _cross_play_wide


def cross_play(env, bank, members_a=None, members_b=None, greedy=True, seed=0, steps=None):
    """The cross-play matrix of ``bank``'s members on one batch of worlds: world n plays pair n mod (Ka Kb), seat 0 under
    ``members_a[pair // Kb]`` and seat 1 under ``members_b[pair % Kb]`` (default every row of the bank).  All worlds are restarted, one
    horizon of (``cnn_act_bank``, step) follows, no host wait inside, and the last-episode return
    of ``enable_episode_stats`` (the team's, as seat 0 received it) is averaged per pair.  ``env``: a two-player kitchen env
    wrapper on the GPU.  Returns ``CrossPlayResult(mean_return, episodes)``, float64 and int64 (Ka, Kb) on the device;
    ``episodes`` is the number of worlds that played the pair.

    With an ``MlpBasePolicyBank`` ``env`` is a ``BalanceMadronaTorch`` on the GPU and ``steps`` (default 12, four times the beam's TIME of
    three: six episodes where nobody leaves the line) times (``mlpbase_act_bank``, step) follow the restart.  The beam's episodes have no fixed length, so every episode a
    world finishes within ``steps`` counts: behind each step the last-episode return of the worlds whose DONE is set is added to
    per-world float64 sums and counts (elementwise, no host wait), which are reduced per pair at the end -- the returns are
    float32, so the sums are exact whatever the order.  ``episodes`` is then the number of finished episodes per pair.

    With a ``WidePolicyBank`` ``env`` is a ``HanabiMadrona`` or a ``BalanceMadronaTorch`` on the GPU and a step is
    ``agent_act_bank`` for seat 0, the same for seat 1, then the simulator's step; the episodes are counted as on the beam.  A game
    of Hanabi has no length to derive a default from: ``steps`` must be given there (on the beam it defaults to 12).  The kitchens
    play one horizon and take no ``steps``."""
    if isinstance(bank, MlpBasePolicyBank):
        return _cross_play_beam(env, bank, members_a, members_b, greedy, seed, steps)
    if isinstance(bank, WidePolicyBank):
        return _cross_play_wide(env, bank, members_a, members_b, greedy, seed, steps)
    if steps is not None:
        raise ValueError("steps is the balance beam's: a kitchen's cross-play lasts one horizon")
    sim = env.sim
    n, p = tuple(sim.observation_world_major_tensor().shape[:2])
    ka, kb, pair, ids = _cross_play_pairs(sim, bank, members_a, members_b, n, p)
    sim.enable_episode_stats()
    sim.reset_worlds(None)
    for t in range(int(env.horizon)):
        cnn_act_bank(sim, bank, ids, seed=seed, step=t, greedy=greedy)
        sim.step()
    last = sim.last_episode_return_tensor().to_torch().reshape(p, n)[0].to(torch.float64)
    return _cross_play_result(ka, kb, pair, last, torch.ones_like(pair))


def _cross_play_beam(env, bank, members_a, members_b, greedy, seed, steps):
    """``cross_play`` for an ``MlpBasePolicyBank`` on the balance beam"""
    sim = env.sim
    if getattr(sim, "_game", None) != "beam":
        raise ValueError("an MlpBasePolicyBank plays on the balance beam: env.sim must be a BalanceBeamSimulator")
    return _cross_play_counted(sim, bank, members_a, members_b, 4 * BEAM_TIME if steps is None else steps,
                               lambda ids, t: mlpbase_act_bank(sim, bank, ids, seed=seed, step=t, greedy=greedy))


class ValueNormBank:
    """One ``ValueNorm`` per member of a policy bank in one tensor: ``state`` (K, 3) float32, row k the three running floats of
    bank row k (``mrl_mappo_bank_update``'s ``value_norm_state``).  ``member(k)`` is a ``ValueNorm`` whose ``state`` IS row k, a
    view: the plain ``mappo_update`` and ``mappo_advantages`` take it, and what either call leaves the other reads."""

    def __init__(self, num_policies, device, beta=0.99999, epsilon=1e-5):
        self.num_policies = int(num_policies)
        if not 1 <= self.num_policies <= _lib.CNN_BANK_MAX_POLICIES:
            raise ValueError(f"a bank holds 1 to {_lib.CNN_BANK_MAX_POLICIES} policies, not {num_policies}")
        self.beta, self.epsilon = float(beta), float(epsilon)
        self.state = torch.zeros((self.num_policies, 3), dtype=torch.float32, device=torch.device(device))

    def __len__(self):
        return self.num_policies

    def member(self, k):
        k = int(k)
        if not 0 <= k < self.num_policies:
            raise IndexError(f"the bank holds policies 0..{self.num_policies - 1}, not {k}")
        member = ValueNorm.__new__(ValueNorm)
        member.beta, member.epsilon, member.state = self.beta, self.epsilon, self.state[k]
        return member


class MappoBankOptimizer(_AdamState):
    """``MappoOptimizer`` for every member of a ``CnnPolicyBank`` or an ``MlpBasePolicyBank`` at once (``mrl_mappo_bank_optimizer``):
    ``exp_avg`` and ``exp_avg_sq`` (K, num_params), row k the moments of bank row k, ONE ``step`` -- every member has taken the same
    number of Adam steps -- and one ``lr`` / ``critic_lr`` (assignable, as ``MappoOptimizer``'s).  ``member(k)`` is a
    ``MappoOptimizer`` for ``bank.policy(k)`` whose moments are VIEWS of row k and whose ``step`` is this one's at the time of the
    call: the plain ``mappo_update`` steps that member alone (the bank's ``step`` does not follow)."""

    def __init__(self, bank, lr=5e-4, critic_lr=5e-4, betas=(0.9, 0.999), eps=1e-5):
        if not isinstance(bank, (CnnPolicyBank, MlpBasePolicyBank)):
            raise ValueError("bank must be a CnnPolicyBank or an MlpBasePolicyBank")
        super().__init__(bank, betas, eps)  # (the moments take bank.params' shape)
        self.bank = bank
        self.lr, self.critic_lr = float(lr), float(critic_lr)

    def member(self, k):
        member = MappoOptimizer(self.bank.policy(k), self.lr, self.critic_lr, self.betas, self.eps)
        member.exp_avg, member.exp_avg_sq, member.step = self.exp_avg[int(k)], self.exp_avg_sq[int(k)], self.step
        return member

    def workspace_bytes(self, minibatch_size, num_minibatches, num_members=1):
        """``mrl_mappo_bank_workspace_bytes`` (``mrl_mappo_mlp_bank_workspace_bytes`` for an ``MlpBasePolicyBank``): ``num_members``
        times the plain call's."""
        out = ctypes.c_uint64(0)
        _lib.check(self.bank.policy(0)._mappo_workspace_bytes(int(minibatch_size), int(num_minibatches), ctypes.byref(out), int(num_members)))
        return int(out.value)

    def workspace(self, minibatch_size, num_minibatches, num_members=1):
        return self._cached_workspace(self.workspace_bytes(minibatch_size, num_minibatches, num_members))


def member_samples(owner, members, num_steps):
    """The sample numbers of each member's cells in a record of ``num_steps`` rows -> int32 (M, S) on ``owner``'s device.
    ``owner``: int32 (N, P), the bank row that owns each (world, seat) cell -- the ``ids`` of a ``rollout_bank`` without a
    resample; ``members``: the bank rows wanted.  Row z holds ``(t N + n) P + p`` for every t < ``num_steps`` and every cell with
    ``owner[n, p] == members[z]``, ascending: member z's own batch, S = ``num_steps`` times its cells.  Raises unless every member
    owns the same number (at least one) of cells: ``mappo_update_bank`` takes one B for all.  Looks at ``owner`` on the host, so it
    is called once, outside the training loop."""
    if not isinstance(owner, torch.Tensor) or owner.dim() != 2 or owner.dtype != torch.int32:
        raise ValueError("owner must be an int32 tensor (num_worlds, num_players)")
    members, t = [int(k) for k in members], int(num_steps)
    cells, flat = owner.numel(), owner.reshape(-1).cpu()
    if not members or t < 1 or t * cells >= 2 ** 31:
        raise ValueError("member_samples needs at least one member, one step and fewer than 2^31 samples")
    own = [torch.nonzero(flat == k).view(-1) for k in members]  # ascending
    counts = [int(c.numel()) for c in own]
    if counts[0] == 0 or any(c != counts[0] for c in counts):
        raise ValueError(f"the members must own the same number of cells, at least one each; members {members} own {counts}")
    rows = torch.arange(t, dtype=torch.int64).view(t, 1) * cells
    return torch.stack([(rows + c.view(1, -1)).view(-1) for c in own]).to(torch.int32).to(owner.device)


def mappo_advantages_bank(record, cells, value_norms=None, gamma=0.99, gae_lambda=0.95, first_member=0):
    """``mappo_advantages`` for the record of a ``rollout_bank`` whose cells are owned by different members -> (advantages,
    returns), each (T, N, P).  ``cells``: ``member_samples``' (M, S) for the record's T, row z the cells of bank row ``first_member``
    + z.  With ``value_norms`` (a ``ValueNormBank``) each member's values, the closing ones included, are denormalised with its own
    row's statistics; then ONE ``mrl_gae`` over the whole record (a column's recurrence reads that column alone); then ``(A -
    mean) / (std + 1e-5)`` per member over that member's cells only -- for each member what ``mappo_advantages`` gives on a record
    of its worlds alone.  Cells of no member keep their values as recorded and their raw advantages.  A loop of torch ops over the
    members on the record's device; it does not wait."""
    if not isinstance(record, _MappoRecord):
        raise ValueError("record must be a CnnRecord or an MlpBaseRecord")
    if value_norms is not None and not isinstance(value_norms, ValueNormBank):
        raise ValueError("value_norms must be a ValueNormBank or None")
    t, cols = record.num_steps, record.num_worlds * record.num_players
    if (not isinstance(cells, torch.Tensor) or cells.dim() != 2 or cells.dtype != torch.int32 or cells.device != record.values.device or
            t < 1 or cells.shape[1] == 0 or cells.shape[1] % t):
        raise ValueError(f"cells must be member_samples' int32 (members, samples) on {record.values.device} for the record's {t} steps")
    at = cells.to(torch.int64)
    each = cells.shape[1] // t  # a member's cells: the head of its row is its samples of row 0
    rollout = record.rollout()
    if value_norms is not None:
        values = record.values.clone()
        flat = values.view(-1)
        for z in range(cells.shape[0]):
            own = torch.cat([at[z], at[z, :each] + t * cols])  # rows 0 .. T - 1, then the closing row T
            flat[own] = value_norms.member(int(first_member) + z).denormalize(flat[own])
        rollout = rollout._replace(values=values[:t].view(t, cols), next_value=values[t].view(cols))
    advantages, returns = gae(rollout, gamma, gae_lambda)
    shape = (record.num_steps, record.num_worlds, record.num_players)
    flat = advantages.view(-1)
    for z in range(cells.shape[0]):
        own = flat[at[z]]
        flat[at[z]] = (own - own.mean()) / (own.std() + 1e-5)
    return advantages.view(shape), returns.view(shape)


def mappo_update_bank(bank, optimizer, record, ring, advantages, returns, indices, value_norms=None, first_member=0, clip_param=0.2,
                      entropy_coef=0.01, value_loss_coef=1.0, max_grad_norm=10.0, huber_delta=10.0, use_huber_loss=True,
                      use_clipped_value_loss=True, use_max_grad_norm=True, stats=True, grads=False):
    """``mappo_update`` for M members of ``bank`` (a ``CnnPolicyBank`` or an ``MlpBasePolicyBank``) in one call
    (``mrl_mappo_bank_update`` / ``mrl_mappo_mlp_bank_update``: 2 + 3 R launches whatever M is), enqueued on torch's current
    stream; it does not wait.  ``indices``: int32 (M, R, B); member z is bank row ``first_member`` + z and takes, for r < R, one
    actor and one critic Adam step on the samples ``indices[z, r]`` -- sample numbers of the shared ``record`` (and ``ring``),
    ``advantages`` and ``returns``, normally a permutation of ``member_samples``' row z cut into rows.  ``optimizer``: the
    ``MappoBankOptimizer`` made for ``bank``; its ``step`` grows by R.  ``value_norms``: a ``ValueNormBank`` of the bank's size
    or None.  The loss options are ``mappo_update``'s.  Bank row ``first_member`` + z, its moments, its ValueNorm row, ``stats[z]``
    and ``grads[z]`` are bit for bit what ``mappo_update`` leaves for ``bank.policy(first_member + z)`` with
    ``optimizer.member(...)``, ``value_norms.member(...)`` and ``indices[z]``; no other row of the bank is read or written.
    Returns ``MappoResult(stats, grads)``: (M, R, 8) and (M, R, P), each None unless asked for."""
    if (not isinstance(bank, (CnnPolicyBank, MlpBasePolicyBank)) or not isinstance(optimizer, MappoBankOptimizer) or
            optimizer.bank is not bank):
        raise ValueError("bank must be a CnnPolicyBank or an MlpBasePolicyBank and optimizer the MappoBankOptimizer made for it")
    policy = bank.policy(0)
    policy._mappo_check(record, ring)
    if value_norms is not None and (not isinstance(value_norms, ValueNormBank) or len(value_norms) != len(bank)):
        raise ValueError("value_norms must be a ValueNormBank of the bank's size or None")
    if not isinstance(indices, torch.Tensor) or indices.dim() != 3:
        raise ValueError("indices must be (members, rows, minibatch_size)")
    members, rows, width = indices.shape
    first = int(first_member)
    if members < 1 or first < 0 or first + members > len(bank):
        raise ValueError(f"members {first}..{first + members - 1} are not rows of a bank of {len(bank)}")
    p = bank.params
    if not p.is_cuda:
        raise ValueError("bank.params must be on a GPU")
    bank._check_params(p.device.index)
    device, f32 = p.device, torch.float32
    count = record.num_steps * record.num_worlds * record.num_players
    wanted = [("optimizer.exp_avg", optimizer.exp_avg, f32, p.numel()), ("optimizer.exp_avg_sq", optimizer.exp_avg_sq, f32, p.numel()),
              ("record.actions", record.actions, torch.int32, count), ("record.logprobs", record.logprobs, f32, count),
              ("record.values", record.values, f32, count + count // max(record.num_steps, 1)), ("advantages", advantages, f32, count),
              ("returns", returns, f32, count), ("indices", indices, torch.int32, None)]
    if value_norms is not None:
        wanted.append(("value_norms.state", value_norms.state, f32, 3 * len(bank)))
    _require_tensors(wanted, device)
    (_, entry), shape, batch_type, obs = policy._mappo_batch(record, ring, count)  # row 0's struct: its params are the bank's base
    opt = _lib.MappoBankOptimizerDesc(p.data_ptr(), optimizer.exp_avg.data_ptr(), optimizer.exp_avg_sq.data_ptr(), 4 * p.stride(0), len(bank),
                                      first, members, optimizer.step)
    batch = batch_type(obs.data_ptr(), record.actions.data_ptr(), record.logprobs.data_ptr(), record.values.data_ptr(), returns.data_ptr(),
                       advantages.data_ptr(), count)
    cfg = _mappo_config(optimizer, value_norms, clip_param, entropy_coef, value_loss_coef, max_grad_norm, huber_delta, use_huber_loss,
                        use_clipped_value_loss, use_max_grad_norm)
    workspace = optimizer.workspace(width, rows, members) if width else None
    out_stats = torch.empty((members, rows, len(_lib.MAPPO_STATS)), dtype=f32, device=device) if stats else None
    out_grads = torch.empty((members, rows, bank.num_params), dtype=f32, device=device) if grads else None
    gpu = device.index
    _lib.check(entry(ctypes.byref(shape), ctypes.byref(opt), ctypes.byref(batch), indices.data_ptr(), rows, width, ctypes.byref(cfg),
                     value_norms.state.data_ptr() if value_norms is not None else None,
                     workspace.data_ptr() if workspace is not None else None, workspace.numel() if workspace is not None else 0,
                     out_stats.data_ptr() if stats else None, out_grads.data_ptr() if grads else None, gpu, _stream_ptr(gpu)))
    optimizer.step += rows
    return MappoResult(out_stats, out_grads)
