"""The broken calls behind tests/golden/capi_refusals.json: for the C API's learners' entry points, every refusal that can be raised
without dereferencing an argument, alone and together with the refusal that follows it in the entry point's order of checks (the
earlier one must speak).  tests/test_capi_layers_api.py runs the cases that need no simulator, tests/test_gpu_capi_refusals.py the
ones that need a live one; both compare (return code, whole message) with the file.

A ``Form`` is a well-formed argument list of one entry point; its ``stages`` are the entry point's checks in the order the C code
makes them, each a list of alternative ways (label, overrides) to fail it.  An override names an argument (``None``: a null
pointer) or ``argument.field`` of a descriptor.  ``cases()`` turns the stages into the alone and the paired calls.

The file is recorded by running this module (``python tests/capi_refusal_cases.py cpu|gpu``) with ``MRL_ENVS_LIB`` pointing at a
build of the commit the messages are to be held to, never from the library under test.  Messages carry no addresses.  The file
holds every distinct (return code, message) once and, per form, the messages of its cases in the order of ``Form.cases()``:
``expected()`` gives them back per case id."""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from madrona_rl_envs_playground_amd import _lib  # noqa: E402

GOLDEN = os.path.join(REPO, "tests", "golden", "capi_refusals.json")
NO_MESSAGE = b"capi_refusal_cases: no such key"  # mrl_debug_set refuses it: the message a case shows when it sets none of its own
A = 1 << 20  # a dummy device address, 4 KiB aligned, of the cases that need no simulator


class Form:
    def __init__(self, name, entry_point, args, stages, extras=()):
        self.name, self.entry_point, self.args, self.stages, self.extras = name, entry_point, args, stages, list(extras)

    def call(self, L, overrides):
        unknown = [k for k in overrides if k.split(".")[0] not in dict(self.args)]
        assert not unknown, (self.name, unknown)
        keep, values = [], []
        for arg, default in self.args:
            value = overrides.get(arg, default)
            if isinstance(value, ctypes.Structure):
                value = type(value).from_buffer_copy(value)
                for key, field_value in overrides.items():
                    if key.startswith(arg + "."):
                        setattr(value, key[len(arg) + 1:], field_value)
                keep.append(value)
                value = ctypes.byref(value)
            values.append(value)
        L.mrl_debug_set(NO_MESSAGE, 0)
        rc = getattr(L, self.entry_point)(*values)
        return [int(rc), L.mrl_last_error().decode()]

    def cases(self):
        """(id, overrides): every alternative of every stage alone; every stage's first alternative with the nearest later stage
        that can be broken at the same time (no override in common)"""
        out = []
        for i, stage in enumerate(self.stages):
            for label, overrides in stage:
                out.append((f"{self.name}: {label}", overrides))
            pair = None
            for later in self.stages[i + 1:]:
                pair = next(((a, b) for a in stage for b in later if not clash(a[1], b[1])), None)
                if pair:
                    break
            if pair:
                (la, oa), (lb, ob) = pair
                out.append((f"{self.name}: {la} + {lb}", {**oa, **ob}))
        out += [(f"{self.name}: {label}", overrides) for label, overrides in self.extras]
        assert len({case_id for case_id, _ in out}) == len(out), self.name
        return out


def clash(a, b):
    """two sets of overrides cannot be applied together: one key twice, or a whole argument and one of its fields"""
    whole = lambda o: {k for k in o if "." not in k}  # noqa: E731
    roots = lambda o: {k.split(".")[0] for k in o}  # noqa: E731
    return bool(set(a) & set(b)) or bool(whole(a) & roots(b)) or bool(whole(b) & roots(a))


def run(L, forms):
    return {case_id: form.call(L, overrides) for form in forms for case_id, overrides in form.cases()}


# ---------------------------------------------------------------- the cases that need no simulator

def mappo_update_forms():
    cfg = _lib.MappoConfig(0.2, 0.01, 1.0, 10.0, 10.0, 5e-4, 5e-4, 0.9, 0.999, 1e-5, 0.99999, 1e-5, 1e-5, 15)
    nets = {
        "mrl_mappo": (_lib.MappoPolicyDesc(A, 64, 0, 5, 4, 26), _lib.MappoBatch(A, A, A, A, A, A, 128),
                      [("hidden 32", {"policy.hidden": 32}), ("width 2", {"policy.width": 2}),
                       ("more than 65535 cells", {"policy.width": 300, "policy.height": 300}), ("12 x 5 LDS image", {"policy.width": 12, "policy.height": 5}),
                       ("minibatch_size 0", {"minibatch_size": 0}), ("empty batch", {"batch.size": 0})]),
        "mrl_mappo_mlp": (_lib.MlpBasePolicyDesc(A, 64, 2, 0), _lib.MappoMlpBatch(A, A, A, A, A, A, 128),
                          [("hidden 32", {"policy.hidden": 32}), ("layer_N 0", {"policy.layer_N": 0}), ("layer_N 3", {"policy.layer_N": 3}),
                           ("minibatch_size 0", {"minibatch_size": 0}), ("empty batch", {"batch.size": 0})]),
    }
    forms = []
    for prefix, (policy, batch, shape_stage) in nets.items():
        for bank in (False, True):
            opt = _lib.MappoBankOptimizerDesc(A, 2 * A, 2 * A, 1 << 24, 3, 0, 2, 0) if bank else _lib.MappoOptimizerDesc(A, 2 * A, 2 * A, 0)
            args = [("policy", policy), ("opt", opt), ("batch", batch), ("indices", A), ("num_minibatches", 1), ("minibatch_size", 64),
                    ("cfg", cfg), ("state", A), ("workspace", A), ("workspace_bytes", 1 << 40), ("stats", None), ("grads", None), ("gpu_id", 0),
                    ("stream", None)]
            nulls = [(f"null {name}", {name: None}) for name in ("policy", "batch", "indices", "cfg", "workspace")]
            stages = [
                nulls if bank else nulls + [("null opt", {"opt": None})],
                [(f"null {key}", {key: None}) for key in ("batch.obs", "opt.exp_avg", "opt.exp_avg_sq", "opt.params_dev", "policy.params_dev",
                                                           "batch.actions", "batch.logprobs", "batch.value_preds", "batch.returns",
                                                           "batch.advantages")],
                [("another params_dev", {"policy.params_dev": 3 * A})],
                [("unknown flag", {"cfg.flags": 17})],
                [("VALUENORM without state", {"state": None})],
                shape_stage,
                [("small workspace", {"workspace_bytes": 0})],
                [("workspace off 16 bytes", {"workspace": A + 8}), ("returns off 4 bytes", {"batch.returns": A + 2}), ("stats off 4 bytes", {"stats": A + 2})],
            ]
            extras = []
            if prefix == "mrl_mappo_mlp":
                stages[-1].append(("obs off 4 bytes", {"batch.obs": A + 1}))
            else:  # an int8 observation block may start anywhere: the call gets as far as the next check that fails
                extras.append(("obs off 4 bytes is fine + small workspace", {"batch.obs": A + 1, "workspace_bytes": 0}))
            if bank:
                stages = [
                    [("null optimizer", {"opt": None})],
                    [("no members", {"opt.num_members": 0}), ("no policies", {"opt.num_policies": 0}), ("257 policies", {"opt.num_policies": 257}),
                     ("members past the end", {"opt.first_member": 2})],
                    [("row_bytes off 4 bytes", {"opt.row_bytes": (1 << 24) + 2}), ("row_bytes below the policy", {"opt.row_bytes": 64})],
                ] + stages
                # the workspace must hold one plain workspace per trained member
                extras.append(("workspace of one member for two", {"workspace_bytes": one_member_bytes(prefix)}))
            name = prefix + ("_bank_update" if bank else "_update")
            forms.append(Form(name, name, args, stages, extras))
    return forms


def one_member_bytes(prefix):
    out = ctypes.c_uint64(0)
    shape = (5, 4, 26, 64) if prefix == "mrl_mappo" else (7, 64, 2, 4)
    assert getattr(_lib.lib(), prefix + "_workspace_bytes")(*shape, 64, 1, ctypes.byref(out)) == 0
    return out.value


def ppo_update_form():
    cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, _lib.PPO_NORM_ADV | _lib.PPO_CLIP_VLOSS)
    args = [("shape", _lib.MlpPolicyDesc(0, 4, 64, 2, 0, 0)), ("opt", _lib.PpoOptimizerDesc(A, A, A, 0)), ("batch", _lib.PpoBatch(A, A, A, A, A, A, 128)),
            ("indices", A), ("num_minibatches", 1), ("minibatch_size", 64), ("cfg", cfg), ("workspace", A), ("workspace_bytes", 1 << 40),
            ("stats", None), ("grads", None), ("gpu_id", 0), ("stream", None)]
    stages = [
        [(f"null {name}", {name: None}) for name in ("shape", "opt", "batch", "indices", "cfg", "workspace")],
        [(f"null {key}", {key: None}) for key in ("batch.obs", "opt.params_dev", "opt.exp_avg", "opt.exp_avg_sq", "batch.actions", "batch.logprobs",
                                                   "batch.advantages", "batch.returns", "batch.values")],
        [("hidden 32", {"shape.hidden": 32}), ("obs_dim 5", {"shape.obs_dim": 5}), ("6 observations, 2 actions", {"shape.obs_dim": 6})],
        [("minibatch_size 0", {"minibatch_size": 0}), ("empty batch", {"batch.size": 0}), ("NORM_ADV over one sample", {"minibatch_size": 1})],
        [("small workspace", {"workspace_bytes": 0})],
        [("workspace off 16 bytes", {"workspace": A + 8}), ("obs off 16 bytes", {"batch.obs": A + 8})],
    ]
    extras = [("6 observations: obs off 8 bytes", {"shape.obs_dim": 6, "shape.num_actions": 3, "batch.obs": A + 4}),
              ("6 observations: obs on 8 bytes is fine + small workspace", {"shape.obs_dim": 6, "shape.num_actions": 3, "batch.obs": A + 8, "workspace_bytes": 0})]
    return Form("mrl_ppo_update", "mrl_ppo_update", args, stages, extras)


def agent_update_form():
    cfg = _lib.PpoConfig(0.2, 0.01, 0.5, 0.5, 2.5e-4, 0.9, 0.999, 1e-5, _lib.PPO_NORM_ADV | _lib.PPO_CLIP_VLOSS)
    args = [("policy", _lib.WidePolicyDesc(A, 187, 212, 16)), ("opt", _lib.PpoOptimizerDesc(A, A, A, 0)), ("record", _lib.AgentRecord(*([A] * 18), 8, 33)),
            ("obs_type", _lib.MRL_INT8), ("state_type", _lib.MRL_INT8), ("advantages", A), ("returns", A), ("epochs", 1), ("cfg", cfg),
            ("capacity", 8 * 33), ("workspace", A), ("workspace_bytes", 1 << 40), ("stats", A), ("grads", A), ("gpu_id", 0), ("stream", None)]
    stages = [
        [(f"null {name}", {name: None}) for name in ("policy", "opt", "record", "cfg", "advantages", "returns", "workspace")],
        [(f"null {key}", {key: None}) for key in ("record.obs", "opt.params_dev", "opt.exp_avg", "opt.exp_avg_sq", "record.states", "record.action_masks",
                                                   "record.active", "record.actions", "record.logprobs", "record.values")],
        [("2^24 cells", {"record.num_steps": 1 << 12, "record.num_worlds": 1 << 12})],
        [("no actions", {"policy.num_actions": 0}), ("65 actions", {"policy.num_actions": 65}), ("obs_dim 0", {"policy.obs_dim": 0}),
         ("capacity 0", {"capacity": 0}), ("capacity above T N", {"capacity": 8 * 33 + 1})],
        [("unknown flag", {"cfg.flags": 4})],
        [("obs_type 5", {"obs_type": 5}), ("state_type 5", {"state_type": 5})],
        [("small workspace", {"workspace_bytes": 0})],
        [("workspace off 16 bytes", {"workspace": A + 8}), ("returns off 4 bytes", {"returns": A + 2}), ("int32 obs off 4 bytes", {"obs_type": _lib.MRL_INT32, "record.obs": A + 1})],
    ]
    extras = [("int8 obs off 4 bytes is fine + small workspace", {"record.obs": A + 1, "workspace_bytes": 0})]
    return Form("mrl_agent_update", "mrl_agent_update", args, stages, extras)


def sizer_forms():
    out = ctypes.c_uint64(0)
    keep.append(out)
    ref = ctypes.pointer(out)
    forms = [
        Form("mrl_ppo_workspace_bytes", "mrl_ppo_workspace_bytes",
             [("obs_dim", 4), ("hidden", 64), ("num_actions", 2), ("minibatch_size", 64), ("num_minibatches", 1), ("out", ref)],
             [[("null out", {"out": None}), ("hidden 32", {"hidden": 32}), ("obs_dim 5", {"obs_dim": 5}), ("minibatch_size 0", {"minibatch_size": 0})]]),
        Form("mrl_agent_update_workspace_bytes", "mrl_agent_update_workspace_bytes",
             [("obs_dim", 187), ("state_dim", 212), ("num_actions", 16), ("capacity", 64), ("out", ref)],
             [[("null out", {"out": None})], [("65 actions", {"num_actions": 65}), ("state_dim 0", {"state_dim": 0})],
              [("capacity 0", {"capacity": 0}), ("capacity 2^24", {"capacity": 1 << 24})]]),
        Form("mrl_agent_bank_workspace_bytes", "mrl_agent_bank_workspace_bytes", [("num_worlds", 33), ("num_policies", 3), ("out", ref)],
             [[("null out", {"out": None}), ("no policies", {"num_policies": 0}), ("257 policies", {"num_policies": 257})]]),
    ]
    cnn = [("width", 5), ("height", 4), ("channels", 26), ("hidden", 64), ("minibatch_size", 64), ("num_minibatches", 1)]
    cnn_shape = [[("hidden 32", {"hidden": 32})], [("width 2", {"width": 2}), ("no channels", {"channels": 0})],
                 [("more than 65535 cells", {"width": 300, "height": 300})], [("12 x 5 LDS image", {"width": 12, "height": 5})],
                 [("minibatch_size 0", {"minibatch_size": 0})]]
    mlp = [("obs_dim", 7), ("hidden", 64), ("layer_N", 2), ("num_actions", 4), ("minibatch_size", 64), ("num_minibatches", 1)]
    mlp_shape = [[("hidden 32", {"hidden": 32})], [("layer_N 0", {"layer_N": 0}), ("layer_N 3", {"layer_N": 3})],
                 [("obs_dim 8", {"obs_dim": 8}), ("5 actions", {"num_actions": 5})], [("minibatch_size 0", {"minibatch_size": 0})]]
    members = [("no members", {"num_members": 0}), ("257 members", {"num_members": 257})]
    for prefix, args, shape in (("mrl_mappo", cnn, cnn_shape), ("mrl_mappo_mlp", mlp, mlp_shape)):
        forms.append(Form(prefix + "_workspace_bytes", prefix + "_workspace_bytes", args + [("out", ref)], [[("null out", {"out": None})]] + shape))
        forms.append(Form(prefix + "_bank_workspace_bytes", prefix + "_bank_workspace_bytes", args + [("num_members", 2), ("out", ref)],
                          [members, [("null out", {"out": None})]] + shape))
    return forms


keep = []


def null_handle_forms():
    """a NULL simulator into every entry point that takes one (an argument list otherwise well-formed over dummy addresses)"""
    u32x2 = ctypes.c_uint32 * 2
    first, num = u32x2(0, 0), u32x2(3, 3)
    keep.extend([first, num])
    resample = _lib.CnnResampleDesc(1, first, num, 0)
    cnn_record, mlp_record = _lib.CnnRecordDesc(*([A] * 7), 2), _lib.MlpBaseRecordDesc(*([A] * 8), 2)
    cnn_bank, mlp_bank, wide_bank = _lib.CnnBankDesc(A, 3, 1 << 20, 64, 0), _lib.MlpBaseBankDesc(A, 3, 1 << 20, 64, 2, 0), _lib.WideBankDesc(A, 3, 1 << 20, 7, 7, 4)
    null_list = (ctypes.c_void_p * 1)(None)
    keep.append(null_list)
    s = ("sim", None)
    simple = {
        "mrl_step": [s, ("stream", None)], "mrl_step_with_actions": [s, ("actions", A), ("stream", None)],
        "mrl_step_with_actions_i64": [s, ("actions", A), ("stream", None)],
        "mrl_step_many": [("sims", null_list), ("count", 1), ("actions", None), ("stream", None)],
        "mrl_step_phase1": [s, ("actions", None), ("stream", None)], "mrl_step_phase2": [s, ("base", A), ("stream", None)],
        "mrl_step_phase2_gathered": [s, ("counts", A), ("num_ranks", 1), ("rank", 0), ("stream", None)],
        "mrl_exchange_create": [s, ("num_ranks", 1), ("rank", 0), ("handle", ctypes.create_string_buffer(64))],
        "mrl_exchange_connect": [s, ("handles", ctypes.create_string_buffer(64))], "mrl_step_exchanged": [s, ("actions", None), ("stream", None)],
        "mrl_set_observation_output": [s, ("obs", A), ("bytes", 64)], "mrl_set_observation_ring": [s, ("base", A), ("stride", 64), ("slots", 1)],
        "mrl_prepare_graph_capture": [s, ("stream", None)], "mrl_enable_episode_stats": [s, ("stream", None)],
        "mrl_clear_episode_totals": [s, ("stream", None)], "mrl_set_episode_counter": [s, ("next", 0), ("stream", None)],
        "mrl_reseed_shard": [s, ("offset", 0), ("total", 1), ("stream", None)], "mrl_reset_worlds": [s, ("mask", None), ("stream", None)],
        "mrl_step_sequence": [s, ("actions", A), ("steps", 1), ("stream", None)],
        "mrl_rollout_random": [s, ("steps", 1), ("seed", 0), ("first_step", 0), ("stream", None)],
        "mrl_rollout_policy": [s, ("policy", _lib.MlpPolicyDesc(A, 4, 64, 2, 0, 0)), ("buffers", _lib.RolloutBuffers(*([A] * 9), 2)), ("seed", 0),
                               ("first_step", 0), ("stream", None)],
        "mrl_agent_act": [s, ("player", 0), ("policy", _lib.WidePolicyDesc(A, 7, 7, 4)), ("record", None), ("row", 0), ("seed", 0), ("step", 0), ("flags", 0),
                          ("workspace", A), ("stream", None)],
        "mrl_agent_act_bank": [s, ("player", 0), ("bank", wide_bank), ("ids", A), ("ids_row", None), ("seed", 0), ("step", 0), ("flags", 0), ("workspace", A),
                               ("workspace_bytes", 1 << 30), ("stream", None)],
        "mrl_cnn_act": [s, ("players", 3), ("policy", _lib.CnnPolicyDesc(A, 64, 0)), ("record", cnn_record), ("row", 0), ("seed", 0), ("step", 0), ("flags", 0),
                        ("workspace", A), ("workspace_bytes", 256), ("stream", None)],
        "mrl_mlpbase_act": [s, ("players", 3), ("policy", _lib.MlpBasePolicyDesc(A, 64, 2, 0)), ("record", mlp_record), ("row", 0), ("seed", 0), ("step", 0),
                            ("flags", 0), ("stream", None)],
        "mrl_cnn_act_bank": [s, ("players", 3), ("bank", cnn_bank), ("ids", A), ("record", cnn_record), ("ids_row", None), ("row", 0), ("seed", 0), ("step", 0),
                             ("flags", 0), ("workspace", A), ("workspace_bytes", 1 << 30), ("stream", None)],
        "mrl_mlpbase_act_bank": [s, ("players", 3), ("bank", mlp_bank), ("ids", A), ("record", mlp_record), ("ids_row", None), ("row", 0), ("seed", 0), ("step", 0),
                                 ("flags", 0), ("workspace", A), ("workspace_bytes", 1 << 30), ("stream", None)],
        "mrl_rollout_cnn": [s, ("players", 3), ("policy", _lib.CnnPolicyDesc(A, 64, 0)), ("record", cnn_record), ("ring", A), ("seed", 0), ("first_step", 0),
                            ("stream", None)],
        "mrl_rollout_mlpbase": [s, ("players", 3), ("policy", _lib.MlpBasePolicyDesc(A, 64, 2, 0)), ("record", mlp_record), ("seed", 0), ("first_step", 0),
                                ("stream", None)],
        "mrl_rollout_cnn_bank": [s, ("players", 3), ("bank", cnn_bank), ("ids", A), ("episodes", A), ("resample", resample), ("record", cnn_record),
                                 ("ids_record", A), ("ring", A), ("seed", 0), ("first_step", 0), ("workspace", A), ("workspace_bytes", 1 << 30), ("stream", None)],
        "mrl_rollout_mlpbase_bank": [s, ("players", 3), ("bank", mlp_bank), ("ids", A), ("episodes", A), ("resample", resample), ("record", mlp_record),
                                     ("ids_record", A), ("seed", 0), ("first_step", 0), ("workspace", A), ("workspace_bytes", 1 << 30), ("stream", None)],
        "mrl_tensor": [s, ("slot", 0), ("out", _lib.TensorDesc())],
    }
    for name in ("mrl_cnn_bank_resample", "mrl_mlpbase_bank_resample", "mrl_agent_bank_resample"):
        simple[name] = [s, ("players", 3), ("resample", resample), ("ids", A), ("episodes", A), ("stream", None)]
    forms = []
    for name, args in simple.items():
        stages = [[("null simulator", {})]]
        # what is checked next to the handle: the earlier one of the two must speak
        second = next((arg for arg in ("bank", "policy", "resample") if arg in dict(args)), None)
        extras = [(f"null simulator + null {second}", {second: None})] if second else []
        forms.append(Form(name + " (no simulator)", name, args, stages, extras))
    return forms


def cpu_forms():
    return mappo_update_forms() + [ppo_update_form(), agent_update_form()] + sizer_forms() + null_handle_forms()


# ---------------------------------------------------------------- the cases that need a live simulator

class Live:
    """The smallest simulators there are and real device buffers for every argument, so that a call that is not refused (none
    must be) would show: ``unchanged()`` compares every buffer a launch could write with its marks."""

    def __init__(self):
        import torch
        from madrona_rl_envs_playground_amd import layouts
        from madrona_rl_envs_playground_amd.simulators import (BalanceBeamSimulator, CartpoleSimulator, ExecMode, OvercookedSimulator,
                                                                 SimplecookedSimulator)
        self.torch, self.dev = torch, torch.device("cuda", 0)
        make = lambda cls, n, **params: cls(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **params)  # noqa: E731
        cramped = layouts.get_base_layout_params("cramped_room", 25)
        smallest = min(layouts.SIMPLECOOKED_LAYOUTS, key=lambda name: (lambda p: int(p["width"]) * int(p["height"]))(
            layouts.get_simplecooked_layout_params(name, 25)))
        self.sims = {
            "overcooked": make(OvercookedSimulator, 2, **cramped), "simplecooked": make(SimplecookedSimulator, 2, **layouts.get_simplecooked_layout_params(smallest, 25)),
            "balance": make(BalanceBeamSimulator, 2), "cartpole": make(CartpoleSimulator, 1),
            "sharded overcooked": make(OvercookedSimulator, 2, **cramped), "sharded balance": make(BalanceBeamSimulator, 2),
            "prepared balance": make(BalanceBeamSimulator, 2),
        }
        self.sims["sharded overcooked"].exchange_create(1, 0)
        self.sims["sharded balance"].exchange_create(1, 0)
        self.sims["prepared balance"].prepare_graph_capture()
        self.marked = []
        self.T, self.K = 2, 3
        torch.cuda.synchronize()

    def handle(self, name):
        return self.sims[name]._handle

    def buffer(self, count, dtype, value):
        t = self.torch.full((count,), value, dtype=dtype, device=self.dev)
        self.marked.append((t, t.clone()))
        return t.data_ptr()

    def watch(self, tensor):
        self.marked.append((tensor, tensor.clone()))

    def unchanged(self):
        self.torch.cuda.synchronize()
        return all(self.torch.equal(now, then) for now, then in self.marked)

    def close(self):
        for sim in self.sims.values():
            sim.close()


def resample_stages(P):
    u32 = ctypes.c_uint32 * 32
    ranges = lambda f, m: (u32(*([f] * P)), u32(*([m] * P)))  # noqa: E731
    empty, late, long = ranges(0, 0), ranges(255, 2), ranges(0, 257)
    keep.extend([empty, late, long])
    as_pointer = lambda arr: ctypes.cast(arr, ctypes.POINTER(ctypes.c_uint32))  # noqa: E731
    desc = [("mode 0", {"resample.mode": 0}), ("mode 3", {"resample.mode": 3}), ("null first_id", {"resample.first_id": None}),
            ("null num_ids", {"resample.num_ids": None})]
    seat_ranges = [("an empty range", {"resample.num_ids": as_pointer(empty[1])}),
                   ("a range past 256", {"resample.first_id": as_pointer(late[0]), "resample.num_ids": as_pointer(late[1])}),
                   ("a range of 257", {"resample.num_ids": as_pointer(long[1])})]
    return desc, seat_ranges


def gpu_forms(live):
    """every form that needs a live simulator: the CNN's five entry points on Overcooked and on Simplecooked, MLPBase's five and
    the wide agent's resample on the balance beam"""
    torch = live.torch
    L = _lib.lib()
    T, K = live.T, live.K
    forms = []
    wrong = live.handle("cartpole")
    u32 = ctypes.c_uint32 * 32

    def common(sim_name, P):
        cells = 2 * P
        first, num = u32(*([0] * P)), u32(*([K] * P))
        keep.extend([first, num])
        resample = _lib.CnnResampleDesc(1, ctypes.cast(first, ctypes.POINTER(ctypes.c_uint32)), ctypes.cast(num, ctypes.POINTER(ctypes.c_uint32)), 0)
        ids = live.buffer(cells, torch.int32, 1)
        episodes = live.buffer(2, torch.int32, 5)
        ids_record = live.buffer((T + 1) * cells, torch.int32, 9)
        bank_bytes = int(L.mrl_cnn_bank_workspace_bytes(2, P, K))
        workspace = live.buffer(bank_bytes + 256, torch.uint8, 0xA5)
        live.sims[sim_name].done_tensor().to_torch().fill_(1)  # a resample that ran would move every id
        for tensor in (live.sims[sim_name].action_tensor().to_torch(),):
            tensor.fill_(-7)
            live.watch(tensor)
        return cells, resample, ids, episodes, ids_record, bank_bytes, workspace

    def bank_stages(num_params, bank_bytes, workspace, ids):
        return [
            [("no policies", {"bank.num_policies": 0}), ("257 policies", {"bank.num_policies": 257})],
            [("stride below the policy", {"bank.stride": num_params - 1})],
            [("null ids", {"ids": None}), ("ids off 4 bytes", {"ids": ids + 2})],
            [("null workspace", {"workspace": None}), ("workspace off 16 bytes", {"workspace": workspace + 8}), ("small workspace", {"workspace_bytes": bank_bytes - 1})],
        ]

    row_stages = lambda only: [  # noqa: E731
        [("unknown flag", {"flags": 8})],
        [("row == num_steps", {"row": T}), (only + " before the last row", {"flags": 4, "row": T - 1}), (only + " without a record", {"flags": 4, "row": T, "record": None})],
    ]

    # ---- the CNN on the two kitchens
    for sim_name in ("overcooked", "simplecooked"):
        sim = live.sims[sim_name]
        obs = sim.observation_world_major_tensor().to_torch()
        _, P, H, W, F = obs.shape
        num_params = int(L.mrl_cnn_policy_num_params(W, H, F, 64, 6))
        assert num_params > 0
        cells, resample, ids, episodes, ids_record, bank_bytes, workspace = common(sim_name, P)
        params = live.buffer(K * num_params, torch.float32, 0.0)
        record = _lib.CnnRecordDesc(*[live.buffer((T + 1) * cells * (6 if name == "logits" else 1), torch.int32 if name == "actions" else torch.float32, -77)
                                      for name in _lib.CNN_RECORD_BUFFERS], T)
        ring = live.buffer((T + 1) * obs.numel(), torch.int8, 3)
        policy, bank = _lib.CnnPolicyDesc(params, 64, 0), _lib.CnnBankDesc(params, K, num_params, 64, 0)
        h, everyone = live.handle(sim_name), (1 << P) - 1
        scope = [[("a sharded simulator", {"sim": live.handle("sharded overcooked")})]] if sim_name == "overcooked" else []
        front = lambda who: [[("null simulator", {"sim": None})], [("another game", {"sim": wrong})]] + scope + [  # noqa: E731
            ([] if who == "bank" else [("null policy", {who: None})]) +
            [("null params_dev", {who + ".params_dev": None}), ("hidden 32", {who + ".hidden": 32}), ("policy flag 2", {who + ".flags": 2})],
            [("a record without values", {"record.values": None}), ("a record without next_done", {"record.next_done": None})],
            [("no seat", {"players": 0}), ("a seat beyond the last", {"players": 1 << P})],
        ]
        null_bank = [[("null bank", {"bank": None})]]
        desc, seat_ranges = resample_stages(P)
        act_ws = [[("null workspace", {"workspace": None}), ("workspace off 16 bytes", {"workspace": workspace + 8}), ("small workspace", {"workspace_bytes": 255})]]
        tag = f" on {sim_name}"
        forms.append(Form("mrl_cnn_act" + tag, "mrl_cnn_act",
                          [("sim", h), ("players", everyone), ("policy", policy), ("record", record), ("row", 0), ("seed", 1), ("step", 0), ("flags", 0),
                           ("workspace", workspace), ("workspace_bytes", 256), ("stream", None)],
                          front("policy") + row_stages("MRL_CNN_VALUE_ONLY") + act_ws))
        forms.append(Form("mrl_cnn_act_bank" + tag, "mrl_cnn_act_bank",
                          [("sim", h), ("players", everyone), ("bank", bank), ("ids", ids), ("record", record), ("ids_row", None), ("row", 0), ("seed", 1),
                           ("step", 0), ("flags", 0), ("workspace", workspace), ("workspace_bytes", bank_bytes), ("stream", None)],
                          null_bank + front("bank") + bank_stages(num_params, bank_bytes, workspace, ids) + row_stages("MRL_CNN_VALUE_ONLY")))
        forms.append(Form("mrl_rollout_cnn" + tag, "mrl_rollout_cnn",
                          [("sim", h), ("players", everyone), ("policy", policy), ("record", record), ("ring", ring), ("seed", 1), ("first_step", 0), ("stream", None)],
                          front("policy") + [[("null record", {"record": None}), ("null ring", {"ring": None})]]))
        forms.append(Form("mrl_rollout_cnn_bank" + tag, "mrl_rollout_cnn_bank",
                          [("sim", h), ("players", everyone), ("bank", bank), ("ids", ids), ("episodes", episodes), ("resample", resample), ("record", record),
                           ("ids_record", ids_record), ("ring", ring), ("seed", 1), ("first_step", 0), ("workspace", workspace), ("workspace_bytes", bank_bytes),
                           ("stream", None)],
                          null_bank + front("bank") + bank_stages(num_params, bank_bytes, workspace, ids) + [[("null record", {"record": None}), ("null ring", {"ring": None})]] +
                          [desc, seat_ranges, [("null episodes", {"episodes": None}), ("episodes off 4 bytes", {"episodes": episodes + 2})]],
                          # the CNN takes ids_record wherever it lies: the call gets as far as the next check that fails
                          [("ids_record off 4 bytes is fine + mode 0", {"ids_record": ids_record + 2, "resample.mode": 0})]))
        forms.append(Form("mrl_cnn_bank_resample" + tag, "mrl_cnn_bank_resample",
                          [("sim", h), ("players", everyone), ("resample", resample), ("ids", ids), ("episodes", episodes), ("stream", None)],
                          [[("null simulator", {"sim": None})], [("another game", {"sim": wrong})], [("null resample", {"resample": None})] + desc,
                           [("no seat", {"players": 0}), ("a seat beyond the last", {"players": 1 << P})], seat_ranges,
                           [("null ids", {"ids": None}), ("null episodes", {"episodes": None}), ("ids off 4 bytes", {"ids": ids + 2}),
                            ("episodes off 4 bytes", {"episodes": episodes + 2})]]))

    # ---- MLPBase and the wide agent's resample on the balance beam
    P = 2
    num_params = int(L.mrl_mlpbase_policy_num_params(7, 64, 2, 4))
    cells, resample, ids, episodes, ids_record, bank_bytes, workspace = common("balance", P)
    params = live.buffer(K * num_params, torch.float32, 0.0)
    width = {"logits": 4, "obs": 7}
    record = _lib.MlpBaseRecordDesc(*[live.buffer((T + 1) * cells * width.get(name, 1), torch.int32 if name in ("actions", "obs") else torch.float32, -77)
                                      for name in _lib.MLPBASE_RECORD_BUFFERS], T)
    policy, bank = _lib.MlpBasePolicyDesc(params, 64, 2, 0), _lib.MlpBaseBankDesc(params, K, num_params, 64, 2, 0)
    h = live.handle("balance")

    def front(who):
        return [[("null simulator", {"sim": None})], [("another game", {"sim": wrong})],
                [("a sharded simulator", {"sim": live.handle("sharded balance")}), ("a simulator prepared for capture", {"sim": live.handle("prepared balance")})],
                ([] if who == "bank" else [("null policy", {who: None})]) +
                [("null params_dev", {who + ".params_dev": None}), ("hidden 128", {who + ".hidden": 128}), ("layer_N 0", {who + ".layer_N": 0}),
                 ("layer_N 3", {who + ".layer_N": 3}), ("policy flag 2", {who + ".flags": 2})],
                [("a record without values", {"record.values": None}), ("a record without obs", {"record.obs": None})],
                [("logits off 4 bytes", {"record.logits": record.logits + 2}), ("params_dev off 4 bytes", {who + ".params_dev": params + 2})],
                [("no seat", {"players": 0}), ("a seat beyond the last", {"players": 4})]]

    null_bank = [[("null bank", {"bank": None})]]
    desc, seat_ranges = resample_stages(P)
    only = "MRL_MLPBASE_VALUE_ONLY"
    forms.append(Form("mrl_mlpbase_act", "mrl_mlpbase_act",
                      [("sim", h), ("players", 3), ("policy", policy), ("record", record), ("row", 0), ("seed", 1), ("step", 0), ("flags", 0), ("stream", None)],
                      front("policy") + row_stages(only)))
    forms.append(Form("mrl_mlpbase_act_bank", "mrl_mlpbase_act_bank",
                      [("sim", h), ("players", 3), ("bank", bank), ("ids", ids), ("record", record), ("ids_row", None), ("row", 0), ("seed", 1), ("step", 0),
                       ("flags", 0), ("workspace", workspace), ("workspace_bytes", bank_bytes), ("stream", None)],
                      null_bank + front("bank") + bank_stages(num_params, bank_bytes, workspace, ids) + row_stages(only) +
                      [[("ids_row off 4 bytes", {"ids_row": ids_record + 2})]]))
    forms.append(Form("mrl_rollout_mlpbase", "mrl_rollout_mlpbase",
                      [("sim", h), ("players", 3), ("policy", policy), ("record", record), ("seed", 1), ("first_step", 0), ("stream", None)],
                      front("policy") + [[("null record", {"record": None})]]))
    forms.append(Form("mrl_rollout_mlpbase_bank", "mrl_rollout_mlpbase_bank",
                      [("sim", h), ("players", 3), ("bank", bank), ("ids", ids), ("episodes", episodes), ("resample", resample), ("record", record),
                       ("ids_record", ids_record), ("seed", 1), ("first_step", 0), ("workspace", workspace), ("workspace_bytes", bank_bytes), ("stream", None)],
                      null_bank + front("bank") + bank_stages(num_params, bank_bytes, workspace, ids) + [[("null record", {"record": None})]] +
                      [[("ids_record off 4 bytes", {"ids_record": ids_record + 2})]] +
                      [desc, seat_ranges, [("null episodes", {"episodes": None}), ("episodes off 4 bytes", {"episodes": episodes + 2})]]))
    for name in ("mrl_mlpbase_bank_resample", "mrl_agent_bank_resample"):
        forms.append(Form(name, name, [("sim", h), ("players", 3), ("resample", resample), ("ids", ids), ("episodes", episodes), ("stream", None)],
                          [[("null simulator", {"sim": None})], [("another game", {"sim": wrong})], [("null resample", {"resample": None})] + desc,
                           [("no seat", {"players": 0}), ("a seat beyond the last", {"players": 4})], seat_ranges,
                           [("null ids", {"ids": None}), ("null episodes", {"episodes": None}), ("ids off 4 bytes", {"ids": ids + 2}),
                            ("episodes off 4 bytes", {"episodes": episodes + 2})]]))
    return forms


# The golden file holds every distinct (return code, message) once, the entry point's own name at a message's head written
# "{what}", and per form the messages of its cases in the order of ``Form.cases()``.

def expected(section, forms):
    """{case id: [return code, whole message]} of `forms` as the golden file has them"""
    golden = json.load(open(GOLDEN))
    out = {}
    for form in forms:
        cases, indices = form.cases(), golden[section][form.name]
        assert len(cases) == len(indices), (form.name, len(cases), len(indices))
        for (case_id, _), index in zip(cases, indices):
            rc, text = golden["messages"][index]
            out[case_id] = [rc, form.entry_point + text[len("{what}"):] if text.startswith("{what}: ") else text]
    return out


def templated(forms, got):
    """{form: [[rc, message with "{what}" at its head], ...]} of the results `got` of `forms`, in the order of the cases"""
    out = {}
    for form in forms:
        rows = [got[case_id] for case_id, _ in form.cases()]
        out[form.name] = [[rc, "{what}" + text[len(form.entry_point):] if text.startswith(form.entry_point + ": ") else text] for rc, text in rows]
    return out


def store(sections):
    """writes {section: templated(...)} as the golden file"""
    messages = []
    for row in (row for section in sections.values() for rows in section.values() for row in rows):
        if row not in messages:
            messages.append(row)
    lines = [",\n".join(f"  {json.dumps(name)}: {json.dumps([messages.index(row) for row in rows])}" for name, rows in section.items())
             for section in sections.values()]
    with open(GOLDEN, "w") as f:
        f.write('{"messages": [\n' + ",\n".join(" " + json.dumps(m) for m in messages) + "],\n")
        f.write(",\n".join(f' "{name}": {{\n{body}}}' for name, body in zip(sections, lines)) + "}\n")


def record(section):
    """runs the cases of `section` on the loaded library (MRL_ENVS_LIB) and writes them into the golden file; the other
    section stays as it is"""
    L = _lib.lib()
    live = Live() if section == "gpu" else None
    forms = gpu_forms(live) if live else cpu_forms()
    got = run(L, forms)
    if live:
        assert live.unchanged(), "a refused call wrote something"
    sections = {section: templated(forms, got)}
    if os.path.exists(GOLDEN):
        golden = json.load(open(GOLDEN))
        sections.update({name: {form: [golden["messages"][i] for i in rows] for form, rows in golden[name].items()}
                         for name in ("cpu", "gpu") if name != section and name in golden})
    store(dict(sorted(sections.items())))
    print(f"{len(got)} {section} cases recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    record(sys.argv[1])
