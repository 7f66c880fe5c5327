"""ctypes binding of libmrl_envs.so -- the C ABI declared in include/mrl_envs.h.

There is no fallback: if the library is missing or cannot be loaded the import
of any simulator raises.  ``build()`` compiles it with hipcc for gfx950
(cross-compiles without a GPU).
"""
import ctypes
import os
import subprocess

# torch first: its wheel bundles its own HIP runtime (torch/lib/libamdhip64.so).
# If libmrl_envs.so pulled in /opt/rocm's copy before torch is imported, the
# process would hold two runtimes and torch's would find no GPU.
import torch  # noqa: F401

_PKG = os.path.dirname(os.path.abspath(__file__))
# MRL_ENVS_LIB: load another build of the same ABI (the diagnostic build of `make diag`, diag/libmrl_envs_diag.so)
LIB_PATH = os.environ.get("MRL_ENVS_LIB") or os.path.join(_PKG, "libmrl_envs.so")
CSRC = os.path.join(_PKG, "csrc")
HEADER = os.path.join(os.path.dirname(_PKG), "include", "mrl_envs.h")

MRL_OK, MRL_ERR_INVALID, MRL_ERR_DEVICE, MRL_ERR_SLOT = 0, 1, 2, 3
MRL_INT8, MRL_UINT8, MRL_INT32, MRL_FLOAT32, MRL_UINT32 = 0, 1, 2, 3, 4
MRL_FLOAT64 = 5
# tensor slots of mrl_enable_episode_stats, the same for every game
STATS_EPISODE_RETURN, STATS_EPISODE_STEPS, STATS_LAST_RETURN, STATS_LAST_STEPS, STATS_TOTALS = 64, 65, 66, 67, 68
MAX_DIMS = 6
MAX_RANKS, IPC_HANDLE_BYTES = 16, 64  # MRL_MAX_RANKS, MRL_IPC_HANDLE_BYTES
OBS_RAW, OBS_ACROBOT_GYM = 0, 1  # MRL_OBS_*: the observation mrl_rollout_policy forms from STATE
OBS_BALANCE = 2  # MRL_OBS_BALANCE: the balance beam's seat-0 OBSERVATION row
POLICY_GREEDY = 1  # MRL_POLICY_GREEDY
AGENT_ALL_ROWS, AGENT_VALUE_ONLY = 2, 4  # MRL_AGENT_*: flags of mrl_agent_act beside POLICY_GREEDY
WIDE_HIDDEN, WIDE_MAX_ACTIONS = 512, 64  # MRL_WIDE_*
PPO_NORM_ADV, PPO_CLIP_VLOSS = 1, 2  # MRL_PPO_*
CNN_VALUE_ONLY = 4  # MRL_CNN_VALUE_ONLY: flag of mrl_cnn_act beside POLICY_GREEDY
CNN_HIDDEN, CNN_ACTIONS = 64, 6  # the one shape mrl_cnn_act runs
CNN_BANK_MAX_POLICIES = 256  # the rows an mrl_cnn_bank may hold
CNN_RESAMPLE_ROBIN, CNN_RESAMPLE_RANDOM = 1, 2  # MRL_CNN_RESAMPLE_*
MLPBASE_VALUE_ONLY = 4  # MRL_MLPBASE_VALUE_ONLY: flag of mrl_mlpbase_act beside POLICY_GREEDY
MLPBASE_HIDDEN, MLPBASE_OBS, MLPBASE_ACTIONS = 64, 7, 4  # the one shape mrl_mlpbase_act runs (layer_N 1 or 2)
MLPBASE_RECURRENT = 16  # MRL_MLPBASE_RECURRENT: bit of mrl_mlpbase_policy.flags; the policy is then an mrl_mlpbase_gru_policy
MLPBASE_GRU_LAYERS = 0x100  # MRL_MLPBASE_GRU_LAYERS: added to layer_N in the size queries for the recurrent shape
MLPBASE_GRU_MAX_CHUNK = 16  # MRL_MLPBASE_GRU_MAX_CHUNK: the longest chunk mrl_mappo_mlp_update back-propagates through
MAPPO_VALUENORM, MAPPO_HUBER_LOSS, MAPPO_CLIPPED_VALUE_LOSS, MAPPO_MAX_GRAD_NORM = 1, 2, 4, 8  # MRL_MAPPO_*
MAPPO_STATS = ("value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm", "ratio", "clipfrac", "reserved")
PPO_STATS = ("pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "total_norm", "loss")  # a stats row
AGENT_UPDATE_STATS = PPO_STATS + ("samples", "status")  # a stats row of mrl_agent_update; status 0 done, 1 B < 2, 2 B > capacity

# every symbol include/mrl_envs.h declares
SYMBOLS = [
    "mrl_overcooked_create", "mrl_hanabi_create", "mrl_cartpole_create", "mrl_step", "mrl_step_with_actions",
    "mrl_step_phase1", "mrl_step_phase2", "mrl_set_episode_counter", "mrl_reseed_shard", "mrl_tensor", "mrl_game",
    "mrl_num_worlds", "mrl_kernel_name", "mrl_rollout_kernel_name", "mrl_bytes_per_world_step", "mrl_destroy", "mrl_last_error",
    "mrl_abi_version", "mrl_rollout_random", "mrl_step_sequence", "mrl_debug_set", "mrl_probe_stream",
    "mrl_scan_timed_out", "mrl_simplecooked_create", "mrl_launch_shape", "mrl_balance_create", "mrl_step_with_actions_i64",
    "mrl_step_phase2_gathered", "mrl_set_observation_output", "mrl_set_observation_ring", "mrl_prepare_graph_capture", "mrl_step_many",
    "mrl_build_hash", "mrl_exchange_create", "mrl_exchange_connect", "mrl_step_exchanged", "mrl_reset_worlds",
    "mrl_acrobot_create", "mrl_enable_episode_stats", "mrl_clear_episode_totals", "mrl_mlp_policy_num_params",
    "mrl_rollout_policy", "mrl_gae", "mrl_ppo_workspace_bytes", "mrl_ppo_update", "mrl_wide_policy_num_params",
    "mrl_agent_workspace_bytes", "mrl_agent_act", "mrl_agent_credit", "mrl_gae_active", "mrl_cnn_policy_num_params",
    "mrl_cnn_workspace_bytes", "mrl_cnn_act", "mrl_rollout_cnn", "mrl_mappo_workspace_bytes", "mrl_mappo_update",
    "mrl_agent_update_workspace_bytes", "mrl_agent_update", "mrl_mlpbase_policy_num_params", "mrl_mlpbase_act",
    "mrl_rollout_mlpbase", "mrl_mappo_mlp_workspace_bytes", "mrl_mappo_mlp_update", "mrl_cnn_bank_workspace_bytes",
    "mrl_cnn_act_bank", "mrl_cnn_bank_resample", "mrl_rollout_cnn_bank", "mrl_mlpbase_bank_workspace_bytes", "mrl_mlpbase_act_bank",
    "mrl_mlpbase_bank_resample", "mrl_rollout_mlpbase_bank", "mrl_agent_bank_workspace_bytes", "mrl_agent_act_bank",
    "mrl_agent_bank_resample", "mrl_mappo_bank_workspace_bytes", "mrl_mappo_bank_update", "mrl_mappo_mlp_bank_workspace_bytes",
    "mrl_mappo_mlp_bank_update",
]
ABI_VERSION = 4  # MRL_ABI_VERSION of include/mrl_envs.h this binding was written against


class TensorDesc(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("ndim", ctypes.c_int32),
                ("shape", ctypes.c_int64 * MAX_DIMS), ("strides", ctypes.c_int64 * MAX_DIMS),
                ("device", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class OvercookedConfig(ctypes.Structure):
    _fields_ = [("height", ctypes.c_int64), ("width", ctypes.c_int64), ("num_players", ctypes.c_int64),
                ("placement_in_pot_rew", ctypes.c_int64), ("dish_pickup_rew", ctypes.c_int64),
                ("soup_pickup_rew", ctypes.c_int64), ("horizon", ctypes.c_int64),
                ("terrain", ctypes.POINTER(ctypes.c_int64)), ("start_player_x", ctypes.POINTER(ctypes.c_int64)),
                ("start_player_y", ctypes.POINTER(ctypes.c_int64)), ("recipe_values", ctypes.POINTER(ctypes.c_int64)),
                ("recipe_times", ctypes.POINTER(ctypes.c_int64))]


class HanabiConfig(ctypes.Structure):
    _fields_ = [("colors", ctypes.c_uint32), ("ranks", ctypes.c_uint32), ("players", ctypes.c_uint32),
                ("max_information_tokens", ctypes.c_uint32), ("max_life_tokens", ctypes.c_uint32)]


class MlpPolicyDesc(ctypes.Structure):  # mrl_mlp_policy
    _fields_ = [("params_dev", ctypes.c_void_p), ("obs_dim", ctypes.c_uint32), ("hidden", ctypes.c_uint32),
                ("num_actions", ctypes.c_uint32), ("obs_mode", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("num_members", ctypes.c_uint32)]  # in what was tail padding; 0, which ctypes fills in, is one policy


class RolloutBuffers(ctypes.Structure):  # mrl_rollout_buffers
    _fields_ = [(name, ctypes.c_void_p) for name in ("obs", "actions", "logprobs", "values", "rewards", "dones", "next_obs",
                                                     "next_value", "next_done")] + [("num_steps", ctypes.c_uint32)]


class PpoConfig(ctypes.Structure):  # mrl_ppo_config
    _fields_ = [(name, ctypes.c_float) for name in ("clip_coef", "ent_coef", "vf_coef", "max_grad_norm", "lr", "beta1", "beta2",
                                                    "eps")] + [("flags", ctypes.c_uint32)]


class PpoBatch(ctypes.Structure):  # mrl_ppo_batch
    _fields_ = [(name, ctypes.c_void_p) for name in ("obs", "actions", "logprobs", "advantages", "returns", "values")] + \
               [("size", ctypes.c_uint32)]


class PpoOptimizerDesc(ctypes.Structure):  # mrl_ppo_optimizer
    _fields_ = [("params_dev", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step", ctypes.c_uint32), ("num_members", ctypes.c_uint32)]  # the same: 0 is one policy


class WidePolicyDesc(ctypes.Structure):  # mrl_wide_policy
    _fields_ = [("params_dev", ctypes.c_void_p), ("obs_dim", ctypes.c_uint32), ("state_dim", ctypes.c_uint32),
                ("num_actions", ctypes.c_uint32)]


AGENT_RECORD_BUFFERS = ("obs", "states", "action_masks", "active", "actions", "logprobs", "values", "dones", "rewards", "last_active",
                        "new_game", "next_done", "running_rewards", "totals", "next_value", "next_active", "first_step", "logits")


class AgentRecord(ctypes.Structure):  # mrl_agent_record
    _fields_ = [(name, ctypes.c_void_p) for name in AGENT_RECORD_BUFFERS] + [("num_steps", ctypes.c_uint32),
                                                                             ("num_worlds", ctypes.c_uint32)]


class CnnPolicyDesc(ctypes.Structure):  # mrl_cnn_policy
    _fields_ = [("params_dev", ctypes.c_void_p), ("hidden", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


CNN_RECORD_BUFFERS = ("actions", "logprobs", "values", "rewards", "dones", "next_done", "logits")


class CnnRecordDesc(ctypes.Structure):  # mrl_cnn_record
    _fields_ = [(name, ctypes.c_void_p) for name in CNN_RECORD_BUFFERS] + [("num_steps", ctypes.c_uint32)]


class CnnBankDesc(ctypes.Structure):  # mrl_cnn_bank
    _fields_ = [("params_dev", ctypes.c_void_p), ("num_policies", ctypes.c_uint32), ("stride", ctypes.c_uint64), ("hidden", ctypes.c_uint32),
                ("flags", ctypes.c_uint32)]


class CnnResampleDesc(ctypes.Structure):  # mrl_cnn_resample
    _fields_ = [("mode", ctypes.c_uint32), ("first_id", ctypes.POINTER(ctypes.c_uint32)), ("num_ids", ctypes.POINTER(ctypes.c_uint32)),
                ("seed", ctypes.c_uint64)]


class MappoPolicyDesc(ctypes.Structure):  # mrl_mappo_policy
    _fields_ = [("params_dev", ctypes.c_void_p), ("hidden", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("channels", ctypes.c_uint32)]


class MappoConfig(ctypes.Structure):  # mrl_mappo_config
    _fields_ = [(name, ctypes.c_float) for name in ("clip_param", "entropy_coef", "value_loss_coef", "max_grad_norm", "huber_delta", "lr",
                                                    "critic_lr", "beta1", "beta2", "opti_eps", "valuenorm_beta",
                                                    "valuenorm_one_minus_beta", "valuenorm_epsilon")] + [("flags", ctypes.c_uint32)]


class MappoBatch(ctypes.Structure):  # mrl_mappo_batch
    _fields_ = [(name, ctypes.c_void_p) for name in ("obs", "actions", "logprobs", "value_preds", "returns", "advantages")] + \
               [("size", ctypes.c_uint32)]


class MappoOptimizerDesc(ctypes.Structure):  # mrl_mappo_optimizer
    _fields_ = [("params_dev", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("step", ctypes.c_uint32)]


class MappoBankOptimizerDesc(ctypes.Structure):  # mrl_mappo_bank_optimizer
    _fields_ = [("params_dev", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("row_bytes", ctypes.c_uint64), ("num_policies", ctypes.c_uint32), ("first_member", ctypes.c_uint32),
                ("num_members", ctypes.c_uint32), ("step", ctypes.c_uint32)]


class MlpBasePolicyDesc(ctypes.Structure):  # mrl_mlpbase_policy
    _fields_ = [("params_dev", ctypes.c_void_p), ("hidden", ctypes.c_uint32), ("layer_N", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


MLPBASE_RECORD_BUFFERS = CNN_RECORD_BUFFERS + ("obs",)


class MlpBaseRecordDesc(ctypes.Structure):  # mrl_mlpbase_record
    _fields_ = [(name, ctypes.c_void_p) for name in MLPBASE_RECORD_BUFFERS] + [("num_steps", ctypes.c_uint32)]


class MlpBaseBankDesc(ctypes.Structure):  # mrl_mlpbase_bank
    _fields_ = [("params_dev", ctypes.c_void_p), ("num_policies", ctypes.c_uint32), ("stride", ctypes.c_uint64), ("hidden", ctypes.c_uint32),
                ("layer_N", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class WideBankDesc(ctypes.Structure):  # mrl_wide_bank
    _fields_ = [("params_dev", ctypes.c_void_p), ("num_policies", ctypes.c_uint32), ("stride", ctypes.c_uint64), ("obs_dim", ctypes.c_uint32),
                ("state_dim", ctypes.c_uint32), ("num_actions", ctypes.c_uint32)]


class MappoMlpBatch(ctypes.Structure):  # mrl_mappo_mlp_batch
    _fields_ = MappoBatch._fields_


# The recurrent MLPBase's structs BEGIN WITH the plain ones and travel through the same entry points (``base_ref``).
class MlpBaseGruPolicyDesc(ctypes.Structure):  # mrl_mlpbase_gru_policy
    _extends_ = MlpBasePolicyDesc
    _fields_ = [("base", MlpBasePolicyDesc), ("h_actor", ctypes.c_void_p), ("h_critic", ctypes.c_void_p)]


class MlpBaseGruRecordDesc(ctypes.Structure):  # mrl_mlpbase_gru_record
    _extends_ = MlpBaseRecordDesc
    _fields_ = [("base", MlpBaseRecordDesc), ("h0_actor", ctypes.c_void_p), ("h0_critic", ctypes.c_void_p), ("chunk_length", ctypes.c_uint32)]


class MappoMlpGruBatch(ctypes.Structure):  # mrl_mappo_mlp_gru_batch
    _extends_ = MappoMlpBatch
    _fields_ = [("base", MappoMlpBatch), ("h0_actor", ctypes.c_void_p), ("h0_critic", ctypes.c_void_p), ("dones", ctypes.c_void_p),
                ("chunk_length", ctypes.c_uint32), ("num_worlds", ctypes.c_uint32), ("num_seats", ctypes.c_uint32)]


def base_ref(struct):
    """``ctypes.byref(struct)`` as the entry points' argument types take it: an extended struct (``_extends_``) goes as a pointer
    to the plain struct it begins with, which is how the library reads it until it has seen the flag"""
    base = getattr(type(struct), "_extends_", None)
    return ctypes.byref(struct) if base is None else ctypes.cast(ctypes.pointer(struct), ctypes.POINTER(base))


class MrlError(RuntimeError):
    pass


def build(force=False, verbose=False):
    """Compile csrc/*.hip into libmrl_envs.so for gfx950 (needs hipcc, no GPU).  Up to date means: the hash compiled into
    the library (``mrl_build_hash``) is the hash of the sources lying beside it -- not file times."""
    if not force and embedded_hash(LIB_PATH) == source_hash():
        return LIB_PATH
    jobs = str(min(6, os.cpu_count() or 1))  # one object per kernel file (csrc/Makefile)
    proc = subprocess.run(["make", "-C", CSRC, "-j", jobs] + (["-B"] if force else []), capture_output=True, text=True)
    if proc.returncode == 0 and embedded_hash(LIB_PATH) != source_hash():
        # file times said "up to date" but the binary is of other sources (a stale copy with a newer time): everything again
        proc = subprocess.run(["make", "-C", CSRC, "-j", jobs, "-B"], capture_output=True, text=True)
    if verbose or proc.returncode != 0:
        print(proc.stdout + proc.stderr)
    if proc.returncode != 0:
        raise MrlError("building libmrl_envs.so failed:\n" + proc.stdout + proc.stderr)
    if embedded_hash(LIB_PATH) != source_hash():
        raise MrlError(f"{LIB_PATH} was rebuilt but carries hash {embedded_hash(LIB_PATH)}, the sources hash to {source_hash()}")
    return LIB_PATH


def source_hash():
    """sha256 (first 16 hex digits) over the sources libmrl_envs.so is built from: name NUL contents of csrc/*.hip, *.hpp and
    the Makefile in sorted order, then include/mrl_envs.h -- the value csrc/Makefile compiles into the library
    (``mrl_build_hash()``).  Measurements that cannot be taken inside a benchmark run (PMC counters:
    profiles/step_traffic.json) carry the LIBRARY's hash, and are only quoted for the build they were taken on."""
    import hashlib
    h = hashlib.sha256()
    files = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp")) or f == "Makefile")
    for path in [os.path.join(CSRC, f) for f in files] + [HEADER]:
        h.update(os.path.basename(path).encode() + b"\0")
        h.update(open(path, "rb").read())
    return h.hexdigest()[:16]


_HASH_TAG = b"MRL_SOURCE_HASH="


def embedded_hash(path):
    """The source hash compiled into a library file, read from its bytes without loading it (None: no such file or no tag)."""
    try:
        blob = open(path, "rb").read()
    except OSError:
        return None
    at = blob.find(_HASH_TAG)
    if at < 0:
        return None
    value = blob[at + len(_HASH_TAG):at + len(_HASH_TAG) + 16]
    return value.decode() if len(value) == 16 and all(c in b"0123456789abcdef" for c in value) else None


def build_hash():
    """``mrl_build_hash()`` of the loaded library."""
    return lib().mrl_build_hash().decode()


_lib = None


def lib():
    """The loaded library.  Raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MrlError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950). There is no CPU fallback for the step kernels.")
    if os.path.isdir(CSRC) and embedded_hash(LIB_PATH) != source_hash():
        # the binary must prove which sources it was built from: rebuild (hipcc cross-compiles anywhere) or refuse
        stale = embedded_hash(LIB_PATH)
        try:
            build()
        except (MrlError, OSError) as exc:
            raise MrlError(f"{LIB_PATH} was built from other sources than those beside it (library {stale}, sources "
                           f"{source_hash()}) and could not be rebuilt: {exc}") from None
    L = ctypes.CDLL(LIB_PATH)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    L.mrl_overcooked_create.argtypes = [ctypes.POINTER(OvercookedConfig), i32, u32, ctypes.POINTER(vp)]
    L.mrl_simplecooked_create.argtypes = [ctypes.POINTER(OvercookedConfig), i32, u32, ctypes.POINTER(vp)]
    L.mrl_launch_shape.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32 * 4)]
    L.mrl_hanabi_create.argtypes = [ctypes.POINTER(HanabiConfig), i32, u32, ctypes.POINTER(vp)]
    L.mrl_cartpole_create.argtypes = [i32, u32, ctypes.POINTER(vp)]
    L.mrl_balance_create.argtypes = [i32, u32, ctypes.POINTER(vp)]
    L.mrl_acrobot_create.argtypes = [i32, u32, ctypes.POINTER(vp)]
    L.mrl_step.argtypes = [vp, vp]
    L.mrl_step_with_actions.argtypes = [vp, vp, vp]
    L.mrl_step_with_actions_i64.argtypes = [vp, vp, vp]
    L.mrl_step_many.argtypes = [ctypes.POINTER(vp), u32, ctypes.POINTER(vp), vp]
    L.mrl_step_phase1.argtypes = [vp, vp, vp]
    L.mrl_step_phase2.argtypes = [vp, vp, vp]
    L.mrl_step_phase2_gathered.argtypes = [vp, vp, u32, u32, vp]
    L.mrl_exchange_create.argtypes = [vp, u32, u32, ctypes.c_char_p]
    L.mrl_exchange_connect.argtypes = [vp, ctypes.c_char_p]
    L.mrl_step_exchanged.argtypes = [vp, vp, vp]
    L.mrl_set_observation_output.argtypes = [vp, vp, ctypes.c_uint64]
    L.mrl_set_observation_ring.argtypes = [vp, vp, ctypes.c_uint64, u32]
    L.mrl_prepare_graph_capture.argtypes = [vp, vp]
    L.mrl_set_episode_counter.argtypes = [vp, u32, vp]
    L.mrl_reseed_shard.argtypes = [vp, u32, u32, vp]
    L.mrl_rollout_random.argtypes = [vp, u32, ctypes.c_uint64, u32, vp]
    L.mrl_step_sequence.argtypes = [vp, vp, u32, vp]
    L.mrl_reset_worlds.argtypes = [vp, vp, vp]
    L.mrl_enable_episode_stats.argtypes = [vp, vp]
    L.mrl_clear_episode_totals.argtypes = [vp, vp]
    L.mrl_mlp_policy_num_params.argtypes = [u32, u32, u32]
    L.mrl_mlp_policy_num_params.restype = ctypes.c_uint64
    L.mrl_rollout_policy.argtypes = [vp, ctypes.POINTER(MlpPolicyDesc), ctypes.POINTER(RolloutBuffers), ctypes.c_uint64, u32, vp]
    L.mrl_gae.argtypes = [vp, vp, vp, vp, vp, u32, u32, ctypes.c_float, ctypes.c_float, vp, vp, i32, vp]
    L.mrl_ppo_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_ppo_update.argtypes = [ctypes.POINTER(MlpPolicyDesc), ctypes.POINTER(PpoOptimizerDesc), ctypes.POINTER(PpoBatch), vp, u32,
                                 u32, ctypes.POINTER(PpoConfig), vp, ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_wide_policy_num_params.argtypes = [u32, u32, u32]
    L.mrl_wide_policy_num_params.restype = ctypes.c_uint64
    L.mrl_agent_workspace_bytes.argtypes = [u32]
    L.mrl_agent_workspace_bytes.restype = ctypes.c_uint64
    L.mrl_agent_act.argtypes = [vp, u32, ctypes.POINTER(WidePolicyDesc), ctypes.POINTER(AgentRecord), u32, ctypes.c_uint64, u32, u32, vp,
                                vp]
    L.mrl_agent_credit.argtypes = [ctypes.POINTER(AgentRecord), vp, vp, u32, i32, vp]
    L.mrl_gae_active.argtypes = [ctypes.POINTER(AgentRecord), vp, vp, ctypes.c_float, ctypes.c_float, vp, vp, i32, vp]
    L.mrl_agent_update_workspace_bytes.argtypes = [u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_agent_update.argtypes = [ctypes.POINTER(WidePolicyDesc), ctypes.POINTER(PpoOptimizerDesc), ctypes.POINTER(AgentRecord), u32, u32,
                                   vp, vp, u32, ctypes.POINTER(PpoConfig), u32, vp, ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_cnn_policy_num_params.argtypes = [u32, u32, u32, u32, u32]
    L.mrl_cnn_policy_num_params.restype = ctypes.c_uint64
    L.mrl_cnn_workspace_bytes.argtypes = [u32, u32]
    L.mrl_cnn_workspace_bytes.restype = ctypes.c_uint64
    L.mrl_cnn_act.argtypes = [vp, u32, ctypes.POINTER(CnnPolicyDesc), ctypes.POINTER(CnnRecordDesc), u32, ctypes.c_uint64, u32, u32, vp,
                              ctypes.c_uint64, vp]
    L.mrl_mappo_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_mappo_update.argtypes = [ctypes.POINTER(MappoPolicyDesc), ctypes.POINTER(MappoOptimizerDesc), ctypes.POINTER(MappoBatch), vp,
                                   u32, u32, ctypes.POINTER(MappoConfig), vp, vp, ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_rollout_cnn.argtypes = [vp, u32, ctypes.POINTER(CnnPolicyDesc), ctypes.POINTER(CnnRecordDesc), vp, ctypes.c_uint64, u32, vp]
    L.mrl_cnn_bank_workspace_bytes.argtypes = [u32, u32, u32]
    L.mrl_cnn_bank_workspace_bytes.restype = ctypes.c_uint64
    L.mrl_cnn_act_bank.argtypes = [vp, u32, ctypes.POINTER(CnnBankDesc), vp, ctypes.POINTER(CnnRecordDesc), vp, u32, ctypes.c_uint64, u32, u32,
                                   vp, ctypes.c_uint64, vp]
    L.mrl_cnn_bank_resample.argtypes = [vp, u32, ctypes.POINTER(CnnResampleDesc), vp, vp, vp]
    L.mrl_rollout_cnn_bank.argtypes = [vp, u32, ctypes.POINTER(CnnBankDesc), vp, vp, ctypes.POINTER(CnnResampleDesc),
                                       ctypes.POINTER(CnnRecordDesc), vp, vp, ctypes.c_uint64, u32, vp, ctypes.c_uint64, vp]
    L.mrl_mlpbase_policy_num_params.argtypes = [u32, u32, u32, u32]
    L.mrl_mlpbase_policy_num_params.restype = ctypes.c_uint64
    L.mrl_mlpbase_act.argtypes = [vp, u32, ctypes.POINTER(MlpBasePolicyDesc), ctypes.POINTER(MlpBaseRecordDesc), u32, ctypes.c_uint64, u32,
                                  u32, vp]
    L.mrl_rollout_mlpbase.argtypes = [vp, u32, ctypes.POINTER(MlpBasePolicyDesc), ctypes.POINTER(MlpBaseRecordDesc), ctypes.c_uint64, u32, vp]
    L.mrl_mlpbase_bank_workspace_bytes.argtypes = [u32, u32]
    L.mrl_mlpbase_bank_workspace_bytes.restype = ctypes.c_uint64
    L.mrl_mlpbase_act_bank.argtypes = [vp, u32, ctypes.POINTER(MlpBaseBankDesc), vp, ctypes.POINTER(MlpBaseRecordDesc), vp, u32, ctypes.c_uint64,
                                       u32, u32, vp, ctypes.c_uint64, vp]
    L.mrl_mlpbase_bank_resample.argtypes = [vp, u32, ctypes.POINTER(CnnResampleDesc), vp, vp, vp]
    L.mrl_rollout_mlpbase_bank.argtypes = [vp, u32, ctypes.POINTER(MlpBaseBankDesc), vp, vp, ctypes.POINTER(CnnResampleDesc),
                                           ctypes.POINTER(MlpBaseRecordDesc), vp, ctypes.c_uint64, u32, vp, ctypes.c_uint64, vp]
    L.mrl_agent_bank_workspace_bytes.argtypes = [u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_agent_act_bank.argtypes = [vp, u32, ctypes.POINTER(WideBankDesc), vp, vp, ctypes.c_uint64, u32, u32, vp, ctypes.c_uint64, vp]
    L.mrl_agent_bank_resample.argtypes = [vp, u32, ctypes.POINTER(CnnResampleDesc), vp, vp, vp]
    L.mrl_mappo_mlp_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_mappo_bank_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_mappo_mlp_bank_workspace_bytes.argtypes = [u32, u32, u32, u32, u32, u32, u32, ctypes.POINTER(ctypes.c_uint64)]
    L.mrl_mappo_bank_update.argtypes = [ctypes.POINTER(MappoPolicyDesc), ctypes.POINTER(MappoBankOptimizerDesc), ctypes.POINTER(MappoBatch),
                                        vp, u32, u32, ctypes.POINTER(MappoConfig), vp, vp, ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_mappo_mlp_bank_update.argtypes = [ctypes.POINTER(MlpBasePolicyDesc), ctypes.POINTER(MappoBankOptimizerDesc),
                                            ctypes.POINTER(MappoMlpBatch), vp, u32, u32, ctypes.POINTER(MappoConfig), vp, vp,
                                            ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_mappo_mlp_update.argtypes = [ctypes.POINTER(MlpBasePolicyDesc), ctypes.POINTER(MappoOptimizerDesc), ctypes.POINTER(MappoMlpBatch),
                                       vp, u32, u32, ctypes.POINTER(MappoConfig), vp, vp, ctypes.c_uint64, vp, vp, i32, vp]
    L.mrl_tensor.argtypes = [vp, i32, ctypes.POINTER(TensorDesc)]
    L.mrl_game.argtypes = [vp]
    L.mrl_num_worlds.argtypes = [vp]
    L.mrl_num_worlds.restype = u32
    L.mrl_kernel_name.argtypes = [vp]
    L.mrl_kernel_name.restype = ctypes.c_char_p
    L.mrl_rollout_kernel_name.argtypes = [vp]
    L.mrl_rollout_kernel_name.restype = ctypes.c_char_p
    L.mrl_bytes_per_world_step.argtypes = [vp]
    L.mrl_bytes_per_world_step.restype = ctypes.c_uint64
    L.mrl_destroy.argtypes = [vp]
    L.mrl_destroy.restype = None
    L.mrl_last_error.restype = ctypes.c_char_p
    L.mrl_abi_version.restype = i32
    L.mrl_build_hash.restype = ctypes.c_char_p
    L.mrl_debug_set.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    L.mrl_probe_stream.argtypes = [vp, vp, ctypes.c_uint64, i32, i32, vp]
    L.mrl_scan_timed_out.argtypes = [vp]
    if L.mrl_abi_version() != ABI_VERSION:
        raise MrlError(f"{LIB_PATH} implements ABI version {L.mrl_abi_version()}, this binding expects {ABI_VERSION}: "
                       "rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
    if os.path.isdir(CSRC) and L.mrl_build_hash().decode() != source_hash():
        raise MrlError(f"{LIB_PATH} reports build hash {L.mrl_build_hash().decode()}, the sources beside it hash to {source_hash()}")
    _lib = L
    return L


def debug_set(key, value):
    """Test / measurement knob for the NEXT simulator created (``mrl_debug_set``); ``debug_set(None, 0)`` clears all."""
    check(lib().mrl_debug_set(key.encode() if key is not None else None, int(value)))


class debug_knobs:
    """``with debug_knobs({"fused_step": 1}): sim = ...`` -- knobs apply to simulators created inside."""

    def __init__(self, knobs):
        self.knobs = dict(knobs)

    def __enter__(self):
        for k, v in self.knobs.items():
            debug_set(k, v)
        return self

    def __exit__(self, *exc):
        debug_set(None, 0)
        return False


def check(rc):
    if rc != MRL_OK:
        msg = lib().mrl_last_error().decode() or f"error code {rc}"
        raise MrlError(msg)


def i64_array(values):
    arr = (ctypes.c_int64 * len(values))(*[int(v) for v in values])
    return arr
