"""CPU: the C-ABI and Python ends of mrl_reset_worlds that need no GPU -- the null handle, the binding's symbol list, and the
env wrappers that refuse to restart chosen worlds or only pass the request on."""
import pytest
import torch

from madrona_rl_envs_playground_amd.pantheonrl_extension.vectorenv import SyncVectorEnv, VectorMultiAgentEnv


def test_null_handle_is_an_error_naming_the_simulator(hip_lib):
    assert hip_lib.mrl_reset_worlds(None, None, None) != 0
    assert b"null simulator" in hip_lib.mrl_last_error()


def test_symbol_is_bound():
    from madrona_rl_envs_playground_amd import _lib
    assert "mrl_reset_worlds" in _lib.SYMBOLS and _lib.ABI_VERSION == 4


class _Recording(VectorMultiAgentEnv):
    """A two-player vector env that records what n_reset was given."""

    def __init__(self):
        super().__init__(3, device=torch.device("cpu"), n_players=2)
        self.calls = []

    def n_step(self, actions):
        raise AssertionError("not stepped")

    def n_reset(self, worlds=None):
        self.calls.append(worlds)
        return ["ego", "partner"]


def test_vector_env_reset_passes_worlds_only_when_given():
    env = _Recording()
    resampled = []
    env.resample_partner = lambda: resampled.append(True)
    assert env.reset() == "ego"
    mask = torch.tensor([True, False, True])
    assert env.reset(worlds=mask) == "ego"
    assert len(resampled) == 2 and env.calls[0] is None and env.calls[1] is mask


class _OneWorld:
    n_players = 2
    observation_space = action_space = share_observation_space = None

    def n_reset(self):
        return (0, 1), [((0.0,), (0.0,), (1,)), ((0.0,), (0.0,), (1,))]


def test_sync_vector_env_refuses_chosen_worlds():
    env = SyncVectorEnv([_OneWorld, _OneWorld], device=torch.device("cpu"))
    env.n_reset()
    with pytest.raises(NotImplementedError, match="cannot restart chosen worlds"):
        env.n_reset(worlds=torch.tensor([True, False]))


def test_multi_layout_refuses_chosen_worlds():
    from madrona_rl_envs_playground_amd.envs.multi_layout import OvercookedMultiLayout
    multi = OvercookedMultiLayout.__new__(OvercookedMultiLayout)  # (no simulators: the refusal comes first)
    multi.envs = []
    assert multi.n_reset() == []
    with pytest.raises(NotImplementedError, match="cannot restart chosen worlds"):
        multi.n_reset(worlds=torch.ones(4, dtype=torch.bool))
