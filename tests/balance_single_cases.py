"""What tests/test_balance_single_api.py and tests/test_gpu_balance_single.py share: the sizes, seeds and agents of the single-agent
PPO path on the balance beam (``MlpPolicy(7, 4, observation="beam")``), observations drawn from the beam's space, and the update's
batches -- ``ppo_twin.make_batch`` on integer-valued beam rows.  Nothing here touches a GPU."""
import functools

import numpy as np
import torch

import policy_twin
import ppo_twin

D, A = 7, 4
SIZES = [1, 63, 257, 1025]       # one lane, the tails of a wavefront, of a 256-thread workgroup and of the step kernel's grid
SCALES = [1.0, 100.0]            # the trainer's initialisation, and the actor's last layer times 100
ROWS = 8                         # episodes last at most three steps: every world restarts at least twice in the window
SEED = 31337                     # of the rollouts' draws; tests/test_balance_single_api.py counts the draws near a boundary
NVEC = np.array([9] * 6 + [3])   # MultiDiscrete([9] * 6 + [3]): six positions shifted by BUFFER, and the steps left
RAGGED = "three tiles and a tail"
CAP = "the workgroup cap and five"
UPDATE_SIZES = [2, 63, 65, 257, RAGGED, CAP]
STAT_DRAWS = 9  # batches a scalar stat's d is the largest over: as many draws as ppo_twin.stat_margins pools (3 shapes x 3)
# (scale, B) -> seed of its batch and index row, where the derived one puts a sample within 1e-5 of a kink of the loss
SEEDS = {(1.0, 16389): 186124}  # (the size beyond the cap uses all 4 099 samples four times over)


def observations(count, rng):
    """``count`` rows drawn uniformly from the space's ranges, float32 (integer-valued, as the kernel's conversion makes them)"""
    return rng.integers(0, NVEC, size=(count, D)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def agent(scale):
    return policy_twin.make_agent(D, A, policy_twin.AGENT_SEED, actor_scale=scale)


@functools.lru_cache(maxsize=None)
def params(scale):
    return ppo_twin.flat(agent(scale)).numpy().astype(np.float32)


def make_batch(weights, size, seed):
    """``ppo_twin.make_batch`` with the observations replaced by beam rows: uniform actions, old_logprob = current + U(-0.4, 0.4),
    old_value = current + U(-0.5, 0.5), returns = old_value + N(0, 1), advantages = N(0, 3)."""
    rng = np.random.default_rng(seed)
    obs = observations(size, rng)
    actions = rng.integers(0, A, size=size).astype(np.int32)
    now = policy_twin.act(weights, obs, np.zeros(size), A)
    logprobs = (now["logp"][np.arange(size), actions] + rng.uniform(-0.4, 0.4, size=size)).astype(np.float32)
    values = (now["values"] + rng.uniform(-0.5, 0.5, size=size)).astype(np.float32)
    returns = (values + rng.normal(size=size)).astype(np.float32)
    advantages = rng.normal(scale=3.0, size=size).astype(np.float32)
    return ppo_twin.Batch(obs, actions, logprobs, advantages, returns, values)


def seed_of(scale, width):
    return SEEDS.get((scale, width), 70400 + int(scale) + 7 * width)


@functools.lru_cache(maxsize=None)
def fixed_case(scale, width, rows=1, draw=0):
    """Parameters, batch and index rows of one update case, and for row 0 the float64 twin and torch's float32 computation.
    ``draw`` > 0 gives further batches of the same case (``stat_margins``)."""
    weights = params(scale)
    seed = seed_of(scale, width) + 1000003 * draw
    batch = make_batch(weights, ppo_twin.BATCH, seed)
    indices = ppo_twin.make_indices(rows, width, ppo_twin.BATCH, seed)
    cfg = ppo_twin.Config()
    return {"params": weights, "batch": batch, "indices": indices, "cfg": cfg, "twin": ppo_twin.row(weights, batch, indices[0], cfg),
            "f32": ppo_twin.row(weights, batch, indices[0], cfg, torch.float32)}


@functools.lru_cache(maxsize=None)
def stat_margins(scale, width):
    """d of every scalar stat of a case: the largest distance of torch's float32 computation from the twin over ``STAT_DRAWS``
    batches of the same weight set and minibatch size.  One row's own distance is a single draw of a float32 rounding error and
    bounds no other float32 computation (``ppo_twin.stat_margins``, which pools three shapes; this path has one).  A batch with
    a sample within 1e-5 of a kink is passed over: there the two computations may take different branches."""
    d = {name: 0.0 for name in ppo_twin.STATS}
    used, draw = 0, 0
    while used < STAT_DRAWS:
        fixed = fixed_case(scale, width, 1, draw)
        draw += 1
        assert draw < 64
        if fixed["twin"]["kink"] <= ppo_twin.KINK:
            continue
        used += 1
        own = ppo_twin.row_margins(fixed["twin"], fixed["f32"])
        for name in ppo_twin.STATS:
            d[name] = max(d[name], own[name])
    return d


def resolve(width, tile, saturation):
    """a name of ``UPDATE_SIZES`` -> B, given the gradient kernel's tile and the largest B of one tile per workgroup"""
    return 3 * tile + 5 if width == RAGGED else saturation + 5 if width == CAP else width
