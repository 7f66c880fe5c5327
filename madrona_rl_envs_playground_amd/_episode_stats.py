"""Episode returns and lengths kept on the device, as the env wrappers offer them.  Every name here is also ``simulators``'.

May import: _lib.
"""
from ._lib import MrlError


def totals_of(totals):
    """The column sums of a TOTALS tensor (float64, (blocks, 2 + players)) as ``episode_totals`` returns them."""
    sums = totals.sum(dim=0).tolist()  # (the host waits here)
    return {"episodes": int(round(sums[0])), "steps": int(round(sums[1])), "returns": [float(v) for v in sums[2:]]}


class EpisodeStats:
    """What ``env.episode_stats`` is for an env wrapper built with ``record_episode_statistics=True``: the five tensors of
    ``mrl_enable_episode_stats`` as persistent torch views on the simulator's GPU."""

    def __init__(self, sim):
        sim.enable_episode_stats()
        self.episode_return = sim.episode_return_tensor().to_torch()
        self.episode_steps = sim.episode_steps_tensor().to_torch()
        self.last_return = sim.last_episode_return_tensor().to_torch()
        self.last_steps = sim.last_episode_steps_tensor().to_torch()
        self.totals = sim.episode_totals_tensor().to_torch()


class RecordsEpisodeStatistics:
    """Mixin of the env wrappers (``self.sim`` is the simulator): the ``record_episode_statistics`` keyword.  ``infos`` stays
    as it is -- per-world dicts would mean a host synchronisation per step; the numbers are tensors and one call."""

    episode_stats = None

    def _record_episode_statistics(self, record):
        if record:
            self.episode_stats = EpisodeStats(self.sim)

    def _recording(self):
        if self.episode_stats is None:
            raise MrlError("this environment was built without record_episode_statistics=True")

    def episode_totals(self):
        """``sim.episode_totals()``: episodes finished since the last clear, their steps and returns (waits for the GPU)."""
        self._recording()
        return self.sim.episode_totals()

    def clear_episode_totals(self):
        self._recording()
        self.sim.clear_episode_totals()
