"""Python-visible simulator classes: drop-in for the reference's nanobind modules.

    reference module                            class here
    build.madrona_overcooked_example_python  -> OvercookedSimulator   (src/overcooked_env/bindings.cpp:11-84)
    build.madrona_simplecooked_example_python -> SimplecookedSimulator (src/overcooked2_env/bindings.cpp:11-84)
    build.madrona_hanabi_example_python      -> HanabiSimulator       (src/hanabi_env/bindings.cpp:8-48)
    build.madrona_cartpole_example_python    -> CartpoleSimulator     (src/cartpole_env/bindings.cpp:8-31)
    build.madrona_balance_example_python     -> BalanceBeamSimulator  (src/balance_beam_env/bindings.cpp:8-34)
    build.madrona_acrobat_example_python     -> AcrobotSimulator      (src/acrobat_env/bindings.cpp; alias AcrobatSimulator)

Same constructor keywords, same method names; every ``*_tensor()`` returns an
object whose ``to_torch()`` yields a persistent zero-copy ``torch.Tensor`` on the
simulator's GPU (the reference's ``madrona.py.Tensor.to_torch()``).  ``madrona``
below mimics the ``<module>.madrona`` submodule the wrappers reach for
(envs/overcooked_env.py:31).

Everything is computed by libmrl_envs.so (HIP, gfx950).  ``ExecMode.CPU`` raises:
the reference's CPU TaskGraph executor is out of scope, and a
silent CPU path would defeat the parity tests.

This module is what everyone imports and the top of a stack of private modules whose imports go one way, each over those
before it: ``_device`` (stream, exported tensors, checks), ``_draws`` (numpy twins of the device's draws), ``_episode_stats``,
``_bank`` (what the policy banks share), ``_ppo`` (the small MLP's PPO and what every learner shares), ``_wide`` (the wide
agent), ``_mappo_nets`` and ``_mappo`` (MAPPO's two networks), ``_population`` (cross-play and the learner of a whole bank).
It defines the handle and the game classes and re-exports every name of the others, private ones included; none of them
imports it.  ``_Simulator`` inherits the network rollouts (``rollout_policy``, ``rollout_cnn`` ...) from the mixin of the
network's module, and a game class carries ``_game``, the marker by which those modules tell the games apart.
"""
import ctypes
import enum

import torch

from . import _lib
from ._lib import MrlError  # noqa: F401  (re-export, like everything below from the layers)
from ._device import (Tensor, _DeviceBlob, _TORCH_DTYPE, _check_ids, _raw_stream, _require_tensors, _seat_mask,  # noqa: F401
                      _stream_ptr)
from ._draws import (random_acrobot_action, random_action, random_balance_action, random_cartpole_action,  # noqa: F401
                     random_hanabi_action, random_hash, sample_u)
from ._episode_stats import EpisodeStats, RecordsEpisodeStatistics, totals_of  # noqa: F401
from ._bank import (BEAM_TIME, BankResample, CNN_RESAMPLE_MODES, CnnResample, CrossPlayResult, _PolicyBank,  # noqa: F401
                    _bank_resample, _bank_rollout_buffers, _bank_workspace, _check_bank_rollout, _cross_play_counted,
                    _cross_play_pairs, _cross_play_result, resample_twin)
from ._ppo import (MlpAgent, MlpPolicy, MlpPolicyBank, PpoBankOptimizer, PpoOptimizer, PpoResult, Rollout, _AdamState,  # noqa: F401
                   _PolicyRollout, _aliased, _critic_then_actor, _layer_shapes, _mlp, _ppo_structs, _run_update, gae,
                   member_minibatch_indices, minibatch_indices, ppo_update, ppo_update_bank)
from ._wide import (AgentRecord, WideAgent, WideOptimizer, WidePolicy, WidePolicyBank, _WIDE_TYPES, _cross_play_wide,  # noqa: F401
                    _wide_bank_workspace, _wide_mlp, _wide_seats, agent_act, agent_act_bank, agent_bank_workspace_bytes,
                    agent_credit, agent_update, gae_active, wide_resample)
from ._mappo_nets import (CnnActorCritic, MlpBaseActorCritic, MlpBaseGruActorCritic, _ActLayer, _ActorCritic, _CategoricalHead, _CnnActor, _CnnBase,  # noqa: F401
                          _CnnCritic, _CnnLayer, _MlpBase, _MlpBaseActor, _MlpBaseCritic, _MlpBaseGruActor, _MlpBaseGruCritic, _MlpLayer,
                          _RnnLayer)
from ._mappo import (ActsWithCnnPolicy, ActsWithMlpBasePolicy, CnnPolicy, CnnPolicyBank, CnnRecord, MappoOptimizer,  # noqa: F401
                     MappoResult, MlpBaseGruPolicy, MlpBaseGruRecord, MlpBaseGruState, MlpBasePolicy, MlpBasePolicyBank, MlpBaseRecord,
                     ValueNorm, chunk_indices, _ActsWithMappoPolicy, _CNN,
                     _Family, _FlatPolicy, _MLPBASE, _MappoRecord, _MappoRollouts, _act, _act_bank, _bank_call_args,
                     _call_args, _cnn_bank_call_args, _cnn_bank_workspace, _cnn_call_args, _kitchen_cells,
                     _mappo_config, _mlpbase_bank_call_args, _mlpbase_bank_workspace, _mlpbase_call_args, _ring_pointer,
                     _rollout, _rollout_bank, cnn_act, cnn_act_bank, cnn_resample, mappo_advantages, mappo_update, mlpbase_act,
                     mlpbase_act_bank, mlpbase_resample)
from ._population import (MappoBankOptimizer, ValueNormBank, _cross_play_beam, cross_play, mappo_advantages_bank,  # noqa: F401
                          mappo_update_bank, member_samples)


class ExecMode(enum.Enum):
    CPU = 0
    CUDA = 1
    HIP = 1  # alias: on this engine the GPU mode is HIP on MI355X


class madrona:  # noqa: N801  (mirrors `<module>.madrona.ExecMode`)
    ExecMode = ExecMode


class _Simulator(_PolicyRollout, _MappoRollouts):
    """Shared handle management for the six games, and through the two mixins the rollouts under a network: ``rollout_policy``
    and ``rollout_policy_bank`` (``_ppo``), ``rollout_cnn``, ``rollout_cnn_bank``, ``rollout_mlpbase`` and ``rollout_mlpbase_bank`` (``_mappo``)."""

    _SLOTS = {}
    _game = None  # a game class names its game: what the layers below test in place of the class, so a subclass passes

    def __init__(self, exec_mode, gpu_id):
        mode = getattr(exec_mode, "name", str(exec_mode))
        if mode == "CPU" or exec_mode == 0:
            raise NotImplementedError(
                "ExecMode.CPU: this engine has only the HIP (MI355X) step kernels; the reference's CPU "
                "TaskGraph executor is not reproduced (the test-only CPU oracle lives in oracle/).")
        self._L = _lib.lib()
        self._handle = ctypes.c_void_p()
        self.gpu_id = int(gpu_id)
        self._tensors = {}

    # --- reference API -------------------------------------------------
    def step(self):
        """One environment step for all worlds, enqueued on torch's current stream
        (Manager::step; no host synchronisation)."""
        stream = _stream_ptr(self.gpu_id)
        rc = self._L.mrl_step(self._handle, stream)
        if rc:
            _lib.check(rc)

    # --- extensions ----------------------------------------------------
    def _action_pointer(self, actions, steps=None):
        """Every entry point that hands the library a caller-owned action array goes through here: the
        library reads raw int32 words, so dtype, layout, device and size are checked on this side."""
        if not isinstance(actions, torch.Tensor) or not actions.is_cuda or actions.device.index != self.gpu_id:
            raise ValueError(f"actions must be a tensor on cuda:{self.gpu_id} (the simulator's device)")
        if actions.dtype != torch.int32 or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous int32 tensor on the simulator's device")
        expect = self._action_numel if steps is None else steps * self._action_numel
        if actions.numel() != expect:
            raise ValueError(f"actions has {actions.numel()} elements, expected {expect}")
        return actions.data_ptr()

    def step_with_actions(self, actions):
        """Step reading actions from ``actions`` (int32, the ACTION tensor's shape,
        contiguous, on this GPU) instead of the ACTION tensor."""
        ptr = self._action_pointer(actions)
        stream = _stream_ptr(self.gpu_id)
        rc = self._L.mrl_step_with_actions(self._handle, ptr, stream)
        if rc:
            _lib.check(rc)

    def step_with_actions_i64(self, actions):
        """Step reading ``actions`` as int64 (the ACTION tensor's shape, contiguous, on this GPU): the step kernel narrows
        them itself and mirrors them into the ACTION tensor (``mrl_step_with_actions_i64``; Overcooked, Simplecooked)."""
        if (not isinstance(actions, torch.Tensor) or not actions.is_cuda or actions.device.index != self.gpu_id or
                actions.dtype != torch.int64 or not actions.is_contiguous() or actions.numel() != self._action_numel):
            raise ValueError("actions must be a contiguous int64 tensor of the ACTION tensor's size on the simulator's device")
        self._step_i64_checked(actions.data_ptr())

    def _step_i64_checked(self, ptr):
        """``mrl_step_with_actions_i64`` on a pointer the caller has already validated (the env wrappers check the
        harness's tensor once, not twice: every microsecond of host work per call shows at small batches)."""
        rc = self._L.mrl_step_with_actions_i64(self._handle, ptr, _stream_ptr(self.gpu_id))
        if rc:
            _lib.check(rc)

    def step_sequence(self, actions):
        """One step per leading index of ``actions`` (int32, shape (K,) + ACTION tensor's shape, contiguous,
        on this GPU): same results as K ``step_with_actions`` calls (``mrl_step_sequence``)."""
        if not isinstance(actions, torch.Tensor) or actions.dim() < 1:
            raise ValueError("actions must hold K consecutive ACTION tensors")
        ptr = self._action_pointer(actions, steps=int(actions.shape[0]))
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_step_sequence(self._handle, ptr, int(actions.shape[0]), stream))

    def rollout_random(self, num_steps, seed=0, first_step=0):
        """``num_steps`` steps under the uniform random policy, actions drawn on the
        device (``mrl_rollout_random``; see ``random_action`` for the stream)."""
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_rollout_random(self._handle, int(num_steps), int(seed) & (2 ** 64 - 1), int(first_step),
                                              stream))

    def reset_worlds(self, mask=None):
        """Restart the worlds whose ``mask`` entry is nonzero (``None``: every world) as fresh episodes, enqueued on torch's
        current stream (``mrl_reset_worlds``).  ``mask``: (num_worlds,) of bool, uint8 or any integer type, on any device;
        it is copied into a uint8 buffer on the simulator's device that the simulator keeps.  Hanabi, Cartpole and the
        balance beam number the restarted episodes from their episode counter as if those worlds had finished in a step;
        Overcooked and Simplecooked put them back into the start state.  DONE, REWARD and the other per-step outputs keep
        the last step's values."""
        stream = _stream_ptr(self.gpu_id)
        if mask is None:
            _lib.check(self._L.mrl_reset_worlds(self._handle, None, stream))
            return
        if not isinstance(mask, torch.Tensor):
            mask = torch.as_tensor(mask)
        if mask.dim() != 1 or mask.numel() != self.num_worlds:
            raise ValueError(f"mask must have shape ({self.num_worlds},) (one entry per world), got {tuple(mask.shape)}")
        if mask.dtype.is_floating_point or mask.dtype.is_complex:
            raise ValueError(f"mask must be a bool or integer tensor, got {mask.dtype}")
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask != 0
        if getattr(self, "_reset_mask", None) is None:
            self._reset_mask = torch.empty(self.num_worlds, dtype=torch.uint8, device=torch.device("cuda", self.gpu_id))
        with torch.cuda.device(self.gpu_id):
            self._reset_mask.copy_(mask, non_blocking=True)
        self._reset_mask_source = mask  # a pinned host mask is still read by the copy after this returns
        _lib.check(self._L.mrl_reset_worlds(self._handle, self._reset_mask.data_ptr(), stream))

    def step_phase1(self, actions=None):
        ptr = self._action_pointer(actions) if actions is not None else None
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_step_phase1(self._handle, ptr, stream))

    def _word_pointer(self, words, count, what):
        """A caller-owned array of ``count`` 32-bit words the library reads on the device (episode base, gathered
        shard counts): checked here like the action arrays, the C ABI takes a raw pointer."""
        if (not isinstance(words, torch.Tensor) or not words.is_cuda or words.device.index != self.gpu_id or
                words.dtype not in (torch.int32, torch.uint32) or not words.is_contiguous() or words.numel() != count):
            raise ValueError(f"{what} must be a contiguous int32 tensor of {count} element(s) on cuda:{self.gpu_id}")
        return words.data_ptr()

    def step_phase2(self, episode_base=None):
        """``episode_base``: 1-element int32/uint32 CUDA tensor, or None for the
        simulator's own counter."""
        stream = _stream_ptr(self.gpu_id)
        ptr = self._word_pointer(episode_base, 1, "episode_base") if episode_base is not None else None
        _lib.check(self._L.mrl_step_phase2(self._handle, ptr, stream))

    def step_phase2_gathered(self, counts, rank):
        """Phase 2 of rank ``rank`` of a sharded batch: ``counts`` = every rank's SHARD_COUNT of this step (int32 CUDA
        tensor, one element per rank, what an all-gather of ``shard_count_tensor()`` delivers).  The re-seeding launch
        works out its own episode base and advances the simulator's counter (``mrl_step_phase2_gathered``)."""
        if not isinstance(counts, torch.Tensor):
            raise ValueError("counts must be a tensor")
        ptr = self._word_pointer(counts, counts.numel(), "counts")
        _lib.check(self._L.mrl_step_phase2_gathered(self._handle, ptr, int(counts.numel()), int(rank), _stream_ptr(self.gpu_id)))

    def exchange_create(self, num_ranks, rank):
        """This rank's mailbox of the collective-free shard exchange (``mrl_exchange_create``) -> its IPC handle (64 bytes),
        to be handed to every rank."""
        buf = ctypes.create_string_buffer(_lib.IPC_HANDLE_BYTES)
        _lib.check(self._L.mrl_exchange_create(self._handle, int(num_ranks), int(rank), buf))
        return buf.raw

    def exchange_connect(self, handles):
        """``handles``: the IPC handles of all ranks, in rank order (``mrl_exchange_connect``)."""
        blob = b"".join(handles)
        if len(blob) % _lib.IPC_HANDLE_BYTES:
            raise ValueError("handles must be 64 bytes each")
        _lib.check(self._L.mrl_exchange_connect(self._handle, blob))

    def step_exchanged(self, actions=None):
        """One step of a shard whose ranks exchange their finished counts through the mailboxes (``mrl_step_exchanged``):
        phase 1, count + publish, phase 2 polling -- no collective, no host call in between."""
        ptr = None if actions is None else self._action_pointer(actions)
        _lib.check(self._L.mrl_step_exchanged(self._handle, ptr, _stream_ptr(self.gpu_id)))

    def set_observation_output(self, out):
        """Later steps write their observations into ``out`` -- an int8 CUDA tensor of the world-major shape
        (N, P, H, W, F), contiguous, e.g. one slot of a rollout buffer -- instead of the simulator's own tensor; ``None``
        hands the output back (``mrl_set_observation_output``; Overcooked and Simplecooked).  The caller keeps ``out``
        alive while steps that write to it are in flight."""
        if out is None:
            _lib.check(self._L.mrl_set_observation_output(self._handle, None, 0))
            return
        if (not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.gpu_id or
                out.dtype not in (torch.int8, torch.uint8) or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous int8 tensor on cuda:{self.gpu_id}")
        _lib.check(self._L.mrl_set_observation_output(self._handle, out.data_ptr(), out.numel()))

    def prepare_graph_capture(self):
        """Makes this simulator's steps capturable in a HIP graph (``torch.cuda.graph``): Hanabi, Cartpole and the balance beam
        move their launch-to-launch counter state into device memory (``mrl_prepare_graph_capture``; one extra one-thread
        launch per step from then on); nothing to do for Overcooked and Simplecooked.  Call it outside the capture."""
        _lib.check(self._L.mrl_prepare_graph_capture(self._handle, _stream_ptr(self.gpu_id)))

    def set_observation_ring(self, ring):
        """``ring``: an int8 CUDA tensor (T, N, P, H, W, F) whose slots ``ring[s]`` are contiguous -- a rollout buffer.  Step
        number k from this call on writes its observations to ``ring[k % T]``, whether it is a call of its own or step k of
        ``rollout_random`` / ``step_sequence`` (``mrl_set_observation_ring``); ``None`` hands the output back."""
        if ring is None:
            _lib.check(self._L.mrl_set_observation_ring(self._handle, None, 0, 0))
            return
        if (not isinstance(ring, torch.Tensor) or not ring.is_cuda or ring.device.index != self.gpu_id or ring.dim() < 2 or
                ring.dtype not in (torch.int8, torch.uint8) or not ring[0].is_contiguous()):
            raise ValueError(f"ring must be an int8 tensor (T, N, P, H, W, F) on cuda:{self.gpu_id} with contiguous slots")
        _lib.check(self._L.mrl_set_observation_ring(self._handle, ring.data_ptr(), int(ring.stride(0)), int(ring.shape[0])))

    # --- episode returns and lengths on the device (mrl_enable_episode_stats) ---
    def enable_episode_stats(self):
        """From now on every completed step also keeps the worlds' episode returns and lengths, on the device
        (``mrl_enable_episode_stats``: five more tensors, for the rest of the simulator's life; a second call does nothing).
        Call it outside a graph capture."""
        _lib.check(self._L.mrl_enable_episode_stats(self._handle, _stream_ptr(self.gpu_id)))

    def clear_episode_totals(self):
        """Zeroes ``episode_totals_tensor()`` and nothing else (``mrl_clear_episode_totals``); enqueued, no host sync."""
        _lib.check(self._L.mrl_clear_episode_totals(self._handle, _stream_ptr(self.gpu_id)))

    def episode_return_tensor(self): return self._tensor(_lib.STATS_EPISODE_RETURN)  # float32, REWARD's shape
    def episode_steps_tensor(self): return self._tensor(_lib.STATS_EPISODE_STEPS)  # int32, DONE's shape
    def last_episode_return_tensor(self): return self._tensor(_lib.STATS_LAST_RETURN)
    def last_episode_steps_tensor(self): return self._tensor(_lib.STATS_LAST_STEPS)
    def episode_totals_tensor(self): return self._tensor(_lib.STATS_TOTALS)  # float64 (ceil(N / 1024), 2 + players)

    def episode_totals(self):
        """``{"episodes": int, "steps": int, "returns": [float] * players}`` of the episodes finished since the last
        ``clear_episode_totals``: the column sums of ``episode_totals_tensor()``.  The one call here that waits for the GPU."""
        return totals_of(self.episode_totals_tensor().to_torch())

    @property
    def scan_timed_out(self):
        """True once a bounded in-kernel wait has expired (``mrl_scan_timed_out``); every later step raises."""
        return bool(self._L.mrl_scan_timed_out(self._handle))

    def reseed_shard(self, world_offset, num_worlds_total):
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_reseed_shard(self._handle, int(world_offset), int(num_worlds_total), stream))

    def set_episode_counter(self, next_episode):
        stream = _stream_ptr(self.gpu_id)
        _lib.check(self._L.mrl_set_episode_counter(self._handle, int(next_episode), stream))

    @property
    def kernel_name(self):
        return self._L.mrl_kernel_name(self._handle).decode()

    @property
    def rollout_kernel_name(self):
        """The kernel the next ``rollout_random`` runs (a persistent one, or the step kernel once per step)."""
        return self._L.mrl_rollout_kernel_name(self._handle).decode()

    @property
    def bytes_per_world_step(self):
        return int(self._L.mrl_bytes_per_world_step(self._handle))

    @property
    def launch_shape(self):
        """(workgroups, threads per workgroup, LDS bytes per workgroup, worlds per wavefront) of the step kernel."""
        out = (ctypes.c_uint32 * 4)()
        _lib.check(self._L.mrl_launch_shape(self._handle, ctypes.byref(out)))
        return tuple(int(v) for v in out)

    @property
    def num_worlds(self):
        return int(self._L.mrl_num_worlds(self._handle))

    def _tensor(self, slot):
        if slot not in self._tensors:
            self._tensors[slot] = Tensor(self, slot)
        return self._tensors[slot]

    def close(self):
        """Destroys the simulator.  Raises ``MrlError`` if one of its steps ran into SCAN_TIMEOUT (the
        results since then carry unspecified episode numbers) -- after freeing it all the same."""
        if getattr(self, "_handle", None) is not None and self._handle.value:
            bad = bool(self._L.mrl_scan_timed_out(self._handle))
            self._L.mrl_destroy(self._handle)
            self._handle = ctypes.c_void_p()
            if bad:
                raise MrlError("an in-kernel wait expired during this simulator's life (SCAN_TIMEOUT): "
                               "episode numbers since then are unspecified")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OvercookedSimulator(_Simulator):
    """Signature of src/overcooked_env/bindings.cpp:14-71."""

    _create = "mrl_overcooked_create"
    _game = "kitchen"  # (Simplecooked's too: it is an Overcooked simulator wherever the two are told from the other games)

    def __init__(self, exec_mode, gpu_id, num_worlds, terrain, height, width, num_players, start_player_x,
                 start_player_y, placement_in_pot_rew, dish_pickup_rew, soup_pickup_rew, recipe_values, recipe_times,
                 horizon, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        if len(terrain) < height * width:
            raise ValueError("terrain shorter than height*width")
        if len(start_player_x) < num_players or len(start_player_y) < num_players:
            raise ValueError("fewer start positions than players")
        if len(recipe_values) < 16 or len(recipe_times) < 16:
            raise ValueError("recipe tables need 16 entries")
        keep = [_lib.i64_array(terrain), _lib.i64_array(start_player_x), _lib.i64_array(start_player_y),
                _lib.i64_array(recipe_values), _lib.i64_array(recipe_times)]
        cfg = _lib.OvercookedConfig(int(height), int(width), int(num_players), int(placement_in_pot_rew),
                                    int(dish_pickup_rew), int(soup_pickup_rew), int(horizon), *keep)
        _lib.check(getattr(self._L, self._create)(ctypes.byref(cfg), int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self.num_players, self.height, self.width = int(num_players), int(height), int(width)
        self._action_numel = int(num_players) * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def agent_state_tensor(self): return self._tensor(3)  # alias, bindings.cpp:77
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def location_world_id_tensor(self): return self._tensor(8)
    def location_id_tensor(self): return self._tensor(9)
    # world-major views of this engine (no reference counterpart)
    def observation_world_major_tensor(self): return self._tensor(10)
    def state_players_tensor(self): return self._tensor(11)
    def state_objects_tensor(self): return self._tensor(12)
    def state_timestep_tensor(self): return self._tensor(13)


STEP_MANY_MAX = 8  # simulators per launch (the kernel arguments hold that many parameter blocks: mrl_step_many)


def can_step_with_others(sim):
    """May ``sim`` take part in ``step_many``?  Overcooked simulators whose workgroups share one copy of a world's state
    (a large layout that does not fit one tile, with fewer than 8192 worlds: ``mrl_overcooked_step_team``) step alone."""
    return type(sim) is OvercookedSimulator and "step_team" not in sim.kernel_name


def step_many(sims, actions=None):
    """One launch for several ``OvercookedSimulator``s on one GPU -- any mix of layouts and world counts (``mrl_step_many``).
    ``actions``: None (every simulator's ACTION tensor) or one int32 tensor per simulator (an entry may be None)."""
    if not sims:
        return
    if any(type(s) is not OvercookedSimulator for s in sims):
        raise ValueError("step_many takes OvercookedSimulator instances")
    handles = (ctypes.c_void_p * len(sims))(*[s._handle for s in sims])
    ptrs = None
    if actions is not None:
        if len(actions) != len(sims):
            raise ValueError("one action tensor (or None) per simulator")
        ptrs = (ctypes.c_void_p * len(sims))(*[None if a is None else s._action_pointer(a) for s, a in zip(sims, actions)])
    _lib.check(sims[0]._L.mrl_step_many(handles, len(sims), ptrs, _stream_ptr(sims[0].gpu_id)))


class SimplecookedSimulator(OvercookedSimulator):
    """Signature of src/overcooked2_env/bindings.cpp:14-71 ("Simplecooked": the world the reference's trainer
    uses, train/env_utils.py:3).  Same keyword arguments and tensor getters as ``OvercookedSimulator``; terrain
    values follow overcooked2's enum (tomato source last), rows are 5P + 10 bytes, at most 2 players, 100 cells."""

    _create = "mrl_simplecooked_create"

    def dishes_out_tensor(self): return self._tensor(14)  # WorldState.num_dishes_out, int32 (N)


class HanabiSimulator(_Simulator):
    """Signature of src/hanabi_env/bindings.cpp:10-36."""

    _game = "hanabi"

    def __init__(self, exec_mode, gpu_id, num_worlds, colors, ranks, players, max_information_tokens,
                 max_life_tokens, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        cfg = _lib.HanabiConfig(int(colors), int(ranks), int(players), int(max_information_tokens),
                                int(max_life_tokens))
        _lib.check(self._L.mrl_hanabi_create(ctypes.byref(cfg), int(gpu_id), int(num_worlds),
                                             ctypes.byref(self._handle)))
        self._action_numel = 2 * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def agent_state_tensor(self): return self._tensor(8)
    def game_tensor(self): return self._tensor(9)
    def reset_count_tensor(self): return self._tensor(10)
    def scan_timeout_tensor(self): return self._tensor(11)
    def shard_count_tensor(self): return self._tensor(12)


class CartpoleSimulator(_Simulator):
    """Signature of src/cartpole_env/bindings.cpp:11-24."""

    _game = "cartpole"

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_cartpole_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = int(num_worlds)

    def reset_tensor(self): return self._tensor(0)
    def action_tensor(self): return self._tensor(1)
    def observation_tensor(self): return self._tensor(2)
    def reward_tensor(self): return self._tensor(3)
    def world_id_tensor(self): return self._tensor(4)
    def reset_count_tensor(self): return self._tensor(5)
    def scan_timeout_tensor(self): return self._tensor(6)
    def shard_count_tensor(self): return self._tensor(7)


class AcrobotSimulator(_Simulator):
    """Signature of src/acrobat_env/bindings.cpp (``AcrobatSimulator`` there).  ``observation_tensor`` is the raw state
    (theta1, theta2, omega1, omega2); ``episode_length_tensor`` is this engine's per-world episode length (the reference
    keeps one length for all worlds: include/mrl_envs.h)."""

    _game = "acrobot"

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_acrobot_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = int(num_worlds)

    def reset_tensor(self): return self._tensor(0)
    def action_tensor(self): return self._tensor(1)
    def observation_tensor(self): return self._tensor(2)
    def reward_tensor(self): return self._tensor(3)
    def world_id_tensor(self): return self._tensor(4)
    def reset_count_tensor(self): return self._tensor(5)
    def scan_timeout_tensor(self): return self._tensor(6)
    def shard_count_tensor(self): return self._tensor(7)
    def episode_length_tensor(self): return self._tensor(8)


AcrobatSimulator = AcrobotSimulator  # the reference's binding name


class BalanceBeamSimulator(_Simulator):
    """Signature of src/balance_beam_env/bindings.cpp:10-24."""

    _game = "beam"

    def __init__(self, exec_mode, gpu_id, num_worlds, debug_compile=True):
        super().__init__(exec_mode, gpu_id)
        _lib.check(self._L.mrl_balance_create(int(gpu_id), int(num_worlds), ctypes.byref(self._handle)))
        self._action_numel = 2 * int(num_worlds)

    def done_tensor(self): return self._tensor(0)
    def active_agent_tensor(self): return self._tensor(1)
    def action_tensor(self): return self._tensor(2)
    def observation_tensor(self): return self._tensor(3)
    def agent_state_tensor(self): return self._tensor(3)  # alias, bindings.cpp:29
    def action_mask_tensor(self): return self._tensor(4)
    def reward_tensor(self): return self._tensor(5)
    def world_id_tensor(self): return self._tensor(6)
    def agent_id_tensor(self): return self._tensor(7)
    def reset_count_tensor(self): return self._tensor(8)
    def shard_count_tensor(self): return self._tensor(9)
