"""CPU: the ends of mrl_enable_episode_stats / mrl_clear_episode_totals that need no GPU -- the null handle, the binding's
symbol list, the totals' arithmetic, and the env wrappers' ``record_episode_statistics`` keyword against a recording
stand-in simulator."""
import pytest
import torch

from madrona_rl_envs_playground_amd import simulators
from madrona_rl_envs_playground_amd.pantheonrl_extension.vectorenv import MadronaEnv


def test_null_handle_is_an_error_naming_the_simulator(hip_lib):
    for call in (hip_lib.mrl_enable_episode_stats, hip_lib.mrl_clear_episode_totals):
        hip_lib.mrl_step(None, None)  # (leaves another message behind)
        assert call(None, None) != 0
        assert b"null simulator" in hip_lib.mrl_last_error()


def test_symbols_are_bound():
    from madrona_rl_envs_playground_amd import _lib
    assert "mrl_enable_episode_stats" in _lib.SYMBOLS and "mrl_clear_episode_totals" in _lib.SYMBOLS
    assert _lib.ABI_VERSION == 4 and _lib.MRL_FLOAT64 == 5
    assert simulators._TORCH_DTYPE[_lib.MRL_FLOAT64][0] is torch.float64
    assert (_lib.STATS_EPISODE_RETURN, _lib.STATS_EPISODE_STEPS, _lib.STATS_LAST_RETURN, _lib.STATS_LAST_STEPS,
            _lib.STATS_TOTALS) == (64, 65, 66, 67, 68)


def test_totals_are_the_column_sums():
    totals = torch.tensor([[2.0, 31.0, 4.5, -1.0], [0.0, 0.0, 0.0, 0.0], [1.0, 9.0, 0.25, -2.0]], dtype=torch.float64)
    assert simulators.totals_of(totals) == {"episodes": 3, "steps": 40, "returns": [4.75, -3.0]}
    # float64 holds every count a run can reach exactly: far beyond float32's 2^24
    big = torch.tensor([[2.0 ** 40, 2.0 ** 45 + 1.0, 1.0]], dtype=torch.float64)
    assert simulators.totals_of(big) == {"episodes": 2 ** 40, "steps": 2 ** 45 + 1, "returns": [1.0]}

    class Sim(simulators._Simulator):
        def __init__(self):
            pass

        def episode_totals_tensor(self):
            class T:
                def to_torch(self):
                    return totals
            return T()

        def close(self):
            pass

    assert Sim().episode_totals() == {"episodes": 3, "steps": 40, "returns": [4.75, -3.0]}


class _Exported:
    def __init__(self, tensor):
        self.tensor = tensor

    def to_torch(self):
        return self.tensor


class _RecordingSim:
    """Stands in for a two-player simulator of three worlds and records what the wrapper asks of it."""

    def __init__(self):
        self.calls = []
        z = torch.zeros
        self._t = {"done": z(3, dtype=torch.int32), "active_agent": z(2, 3, dtype=torch.int32), "action": z(2, 3, 1, dtype=torch.int32),
                   "observation": z(2, 3, 4, dtype=torch.int8), "agent_state": z(2, 3, 5, dtype=torch.int8),
                   "action_mask": z(2, 3, 6, dtype=torch.int32), "reward": z(2, 3), "world_id": z(2, 3, dtype=torch.int32),
                   "agent_id": z(2, 3, dtype=torch.int32),
                   "episode_return": z(2, 3), "episode_steps": z(3, dtype=torch.int32), "last_episode_return": z(2, 3),
                   "last_episode_steps": z(3, dtype=torch.int32), "episode_totals": z(1, 4, dtype=torch.float64)}

    def __getattr__(self, name):
        if name.endswith("_tensor") and name[:-7] in self._t:
            if name[:-7].startswith(("episode_", "last_episode_")) and "enable_episode_stats" not in self.calls:
                raise AssertionError("statistics tensor asked for before enable_episode_stats")
            return lambda: _Exported(self._t[name[:-7]])
        raise AttributeError(name)

    def enable_episode_stats(self):
        self.calls.append("enable_episode_stats")

    def clear_episode_totals(self):
        self.calls.append("clear_episode_totals")

    def episode_totals(self):
        self.calls.append("episode_totals")
        return {"episodes": 7, "steps": 70, "returns": [1.0, 2.0]}

    def step(self):
        self.calls.append("step")


def test_madrona_env_passes_the_keyword_on_and_leaves_infos_alone():
    sim = _RecordingSim()
    env = MadronaEnv(3, 0, sim, record_episode_statistics=True)
    assert sim.calls == ["enable_episode_stats"]
    stats = env.episode_stats
    assert stats.episode_return is sim._t["episode_return"] and stats.episode_steps is sim._t["episode_steps"]
    assert stats.last_return is sim._t["last_episode_return"] and stats.last_steps is sim._t["last_episode_steps"]
    assert stats.totals is sim._t["episode_totals"]
    _, _, _, infos = env.n_step(torch.zeros(2, 3, 1, dtype=torch.int32))
    assert infos == [{}] * 3 and infos is env.infos
    assert env.episode_totals() == {"episodes": 7, "steps": 70, "returns": [1.0, 2.0]}
    env.clear_episode_totals()
    assert sim.calls == ["enable_episode_stats", "step", "episode_totals", "clear_episode_totals"]


def test_without_the_keyword_nothing_is_enabled():
    sim = _RecordingSim()
    env = MadronaEnv(3, 0, sim)
    assert sim.calls == [] and env.episode_stats is None
    with pytest.raises(simulators.MrlError, match="record_episode_statistics"):
        env.episode_totals()
    with pytest.raises(simulators.MrlError, match="record_episode_statistics"):
        env.clear_episode_totals()
    assert env.n_step(torch.zeros(2, 3, 1, dtype=torch.int32))[3] == [{}] * 3


def test_every_wrapper_takes_the_keyword_last():
    import inspect
    from madrona_rl_envs_playground_amd.envs import (acrobot_env, balance_beam_env, cartpole_env, hanabi_env, overcooked2_env,
                                                      overcooked_env)
    for cls in (cartpole_env.CartpoleMadronaTorch, cartpole_env.CartpoleMadronaNumpy, acrobot_env.AcrobotMadronaTorch,
                acrobot_env.AcrobotMadronaNumpy, hanabi_env.HanabiMadrona, balance_beam_env.BalanceMadronaTorch,
                overcooked_env.OvercookedMadrona, overcooked2_env.OvercookedMadrona, MadronaEnv):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == "record_episode_statistics" and params[-1].default is False, cls
        assert issubclass(cls, simulators.RecordsEpisodeStatistics)


def test_cartpole_wrapper_enables_on_its_simulator(monkeypatch):
    """``_CartpoleBase`` and the Acrobot base build their simulator themselves: with a stand-in class in its place, the
    keyword reaches ``enable_episode_stats`` and ``infos`` keeps its shape."""
    from madrona_rl_envs_playground_amd.envs import acrobot_env, cartpole_env

    class OneLane(_RecordingSim):
        def __init__(self, **kwargs):
            super().__init__()
            z = torch.zeros
            self._t.update({"reset": z(3, 1, dtype=torch.int32), "action": z(3, 1, dtype=torch.int32), "observation": z(3, 4),
                            "reward": z(3, 1)})

    for module, name, cls in ((cartpole_env, "CartpoleSimulator", cartpole_env.CartpoleMadronaTorch),
                              (acrobot_env, "AcrobotSimulator", acrobot_env.AcrobotMadronaTorch)):
        monkeypatch.setattr(module, name, OneLane)
        env = cls(3, 0, record_episode_statistics=True)
        assert env.sim.calls == ["enable_episode_stats"] and env.episode_stats.totals is env.sim._t["episode_totals"]
        assert env.step(torch.zeros(3, dtype=torch.int32))[3] == [{}] * 3
        assert env.episode_totals()["episodes"] == 7
        plain = cls(3, 0)
        assert plain.sim.calls == [] and plain.episode_stats is None
