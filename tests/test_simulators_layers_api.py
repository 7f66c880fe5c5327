"""``simulators`` is a façade over the package's private layers: its surface is pinned, every layer's names are the façade's
own objects, the layers import one way, and MAPPO's two networks refuse in the order they always did.  No GPU."""
import ast
import importlib
import inspect
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from madrona_rl_envs_playground_amd import simulators

PACKAGE = "madrona_rl_envs_playground_amd"
PARTS = ("_device", "_draws", "_episode_stats", "_bank", "_ppo", "_wide", "_mappo_nets", "_mappo", "_population")  # bottom up
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "simulators_surface.json")


def _signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return "callable"


def _member(cls, name):
    member = inspect.getattr_static(cls, name)
    if isinstance(member, property):
        return "property"
    member = getattr(member, "__func__", member)  # what a staticmethod or a classmethod wraps
    return _signature(member) if callable(member) else "attribute"


def _hidden(name):
    return name.startswith("_") and name.endswith("_")  # dunders, and the sunder names an Enum keeps for itself


def _defines(cls, name):
    """does ``cls`` define ``name`` itself or through a base class of this package (not through ``object``, torch or a builtin)"""
    return any(name in vars(base) for base in cls.__mro__ if base.__module__.startswith(PACKAGE))


def surface(module, recorded=None):
    """name -> entry for every name of ``module`` (of ``recorded``, an earlier result, when given) that is neither hidden nor a
    module.  A class's members are those it defines itself, and with ``recorded`` the recorded ones where the class or a base
    class of this package defines them today: a method may move to a mixin, it may not change or go."""
    out = {}
    for name in (recorded if recorded is not None else vars(module)):
        obj = getattr(module, name, None)
        if _hidden(name) or inspect.ismodule(obj):
            continue
        if inspect.isclass(obj):
            members = recorded[name].get("members", ()) if recorded is not None else [m for m in vars(obj) if not _hidden(m)]
            out[name] = {"kind": "class", "signature": _signature(obj),
                         "members": {m: _member(obj, m) if _defines(obj, m) else "missing" for m in sorted(members)}}
        elif inspect.isfunction(obj):
            out[name] = {"kind": "function", "signature": _signature(obj)}
        else:
            out[name] = {"kind": "missing" if not hasattr(module, name) else "other"}
    return out


def test_surface_is_a_superset_of_the_recorded_one():
    """tests/golden/simulators_surface.json is the surface of the commit before the split, written by

        import json
        from madrona_rl_envs_playground_amd import simulators
        from tests.test_simulators_layers_api import surface
        json.dump(surface(simulators), open("tests/golden/simulators_surface.json", "w"), indent=0, sort_keys=True)

    It holds 121 names: 58 functions, 6 others and 57 classes -- the 56 that module defined or aliased and the re-exported
    ``MrlError``.  A later change may add names and members; to change or drop a recorded one it has to regenerate the file."""
    with open(GOLDEN) as f:
        recorded = json.load(f)
    kinds = [entry["kind"] for entry in recorded.values()]
    assert (len(recorded), kinds.count("class"), kinds.count("function"), kinds.count("other")) == (121, 57, 58, 6)
    assert sum(name.startswith("_") for name in recorded) == 44
    today = surface(simulators, recorded)
    changed = {name: (recorded[name], today.get(name)) for name in recorded if today.get(name) != recorded[name]}
    assert not changed


def _defined_in(module):
    """the names a module's own top-level statements define: classes, functions and assignments, not imports"""
    names = []
    for node in ast.parse(inspect.getsource(module)).body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)):
            names.append(node.name)
        elif isinstance(node, ast.Assign):
            names += [target.id for target in node.targets if isinstance(target, ast.Name)]
    return names


@pytest.mark.parametrize("part", PARTS)
def test_facade_holds_every_layers_own_objects(part):
    module = importlib.import_module(f"{PACKAGE}.{part}")
    names = _defined_in(module)
    assert names
    for name in names:
        assert getattr(simulators, name, None) is getattr(module, name), f"{part}.{name} is not simulators.{name}"


@pytest.mark.parametrize("part", PARTS)
def test_layers_import_one_way(part):
    """A layer imports alone, in a fresh interpreter, without the façade; what it imports of the package, inside functions
    included, is on the ``May import:`` line of its header, and only layers below it are."""
    code = (f"import sys, {PACKAGE}.{part}\n"
            f"assert '{PACKAGE}.simulators' not in sys.modules, 'the layer imported the facade'\n"
            f"assert 'torch.cuda' not in sys.modules or not sys.modules['torch'].cuda.is_initialized()\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    done = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    module = importlib.import_module(f"{PACKAGE}.{part}")
    allowed = re.search(r"^May import: (.*)$", module.__doc__, re.MULTILINE)
    assert allowed, "the header docstring has no 'May import:' line"
    allowed = set(re.findall(r"\b_\w+", allowed.group(1)))
    assert allowed <= set(PARTS[:PARTS.index(part)]) | {"_lib"}
    imported = set()
    for node in ast.walk(ast.parse(inspect.getsource(module))):
        if isinstance(node, ast.ImportFrom) and node.level:
            assert node.level == 1
            imported |= {node.module} if node.module else {alias.name for alias in node.names}
        elif isinstance(node, ast.Import):
            assert not any(alias.name.startswith(PACKAGE) for alias in node.names)
    assert imported <= allowed, f"{part} imports {sorted(imported - allowed)}, which its header does not list"


class _NoSimulator:
    """touching anything of it is an AttributeError: a refusal that comes first never looks at the simulator"""


def _beam(cls=simulators.BalanceBeamSimulator):
    sim = cls.__new__(cls)  # no handle: the checks below stop before any call into the library
    sim.gpu_id = 0
    return sim


class _BeamSubclass(simulators.BalanceBeamSimulator):
    pass


def _callers(network):
    """(caller name, call(sim, policy or bank)) for the four public callers of a network; ``ring`` where the network has one"""
    ring = (None,) if network == "cnn" else ()
    ids = torch.zeros((3, 2), dtype=torch.int32)
    return {
        "act": lambda sim, policy: getattr(simulators, f"{network}_act")(sim, policy),
        "act_bank": lambda sim, bank: getattr(simulators, f"{network}_act_bank")(sim, bank, ids),
        "rollout": lambda sim, policy: getattr(simulators._Simulator, f"rollout_{network}")(sim, policy, None, *ring),
        "rollout_bank": lambda sim, bank: getattr(simulators._Simulator, f"rollout_{network}_bank")(sim, bank, ids, None, *ring),
    }


NETWORKS = {
    "cnn": ("policy must be a CnnPolicy", "bank must be a CnnPolicyBank",
            lambda: simulators.CnnPolicy(5, 4, 26, device="cpu"), lambda: simulators.CnnPolicyBank(5, 4, 26, 2, device="cpu")),
    "mlpbase": ("policy must be an MlpBasePolicy", "bank must be an MlpBasePolicyBank",
                lambda: simulators.MlpBasePolicy(device="cpu"), lambda: simulators.MlpBasePolicyBank(2, device="cpu")),
}


@pytest.mark.parametrize("caller", ["act", "act_bank", "rollout", "rollout_bank"])
@pytest.mark.parametrize("network", sorted(NETWORKS))
def test_refusal_precedence(hip_lib, network, caller):
    """The policy's or bank's type is refused first, with the network's own words, before anything of the simulator is looked at:
    the other network's object, the single policy where a bank is due and the reverse.  Then the simulator's game (the beam's
    network only; a subclass of the beam's simulator passes), and only then ``params``."""
    policy_message, bank_message, policy, bank = NETWORKS[network]
    other = "mlpbase" if network == "cnn" else "cnn"
    call = _callers(network)[caller]
    banked = caller.endswith("bank")
    message = bank_message if banked else policy_message
    wrong = [NETWORKS[other][3 if banked else 2](), (policy if banked else bank)(), None]
    for sim in (_NoSimulator(), _beam()):
        for thing in wrong:
            with pytest.raises(ValueError, match=f"^{message}$"):
                call(sim, thing)
    right = (bank if banked else policy)()
    if network == "cnn":
        with pytest.raises(ValueError, match=r"^(policy|bank)\.params must be a contiguous float32 tensor .* on cuda:0$"):
            call(_beam(), right)  # no check of the game: the kitchen's shape would be next, behind params
        return
    entry = "mrl_mlpbase_act_bank" if banked else "mrl_mlpbase_act"  # the rollouts refuse in their act's name
    for sim in (_NoSimulator(), _beam(simulators.HanabiSimulator), _beam(simulators.OvercookedSimulator)):
        with pytest.raises(ValueError, match=f"^{entry} runs on a BalanceBeamSimulator$"):
            call(sim, right)
    for sim in (_beam(), _beam(_BeamSubclass)):
        with pytest.raises(ValueError, match=r"^(policy|bank)\.params must be a contiguous float32 tensor .* on cuda:0$"):
            call(sim, right)
