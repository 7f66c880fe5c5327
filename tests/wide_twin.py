"""Float64 numpy twin of the device-side wide-policy act (``mrl_agent_act``: forward pass, head, sampling), the same function in
torch float32 -- whose distance from the twin sets the tests' margins --, the synthetic inputs the GPU tests write into a
simulator's tensors, the closed loops the CPU oracle walks under the twin (``twin_step``, which also judges the device's own walk
step by step), and float32 numpy restatements of ``mrl_agent_credit`` and ``mrl_gae_active`` that follow include/mrl_envs.h
operation for operation.  Nothing here touches a GPU."""
import functools

import numpy as np
import torch

import hanabi_configs
from madrona_rl_envs_playground_amd import hanabi_spec
from madrona_rl_envs_playground_amd.envs.hanabi_env import config_choice
from madrona_rl_envs_playground_amd.simulators import WideAgent, random_hash

H = 512
SIZES = (1, 31, 33, 65, 257)
AGENT_SEED = 11
WEIGHTS = {"orthogonal": 1.0, "peaked": 300.0}  # the factor on the actor's output layer: 300 moves the probabilities far from uniform


def config_of(game):
    """the configuration of "hanabi_<name>": one of the three named games, or an id of ``hanabi_configs.BY_ID``"""
    name = game[len("hanabi_"):]
    return config_choice[name] if name in config_choice else hanabi_configs.BY_ID[name]


def dims(game):
    """(D, S, A) of ``game``: "balance" or "hanabi_<config>" """
    if game == "balance":
        return 7, 7, 4
    config = config_of(game)
    return hanabi_spec.observation_size(config), hanabi_spec.state_size(config), hanabi_spec.num_moves(config)


# every forward case of tests/test_gpu_wide_agent.py: (game, worlds); each runs with both weight sets
CASES = [(game, n) for game in ("balance", "hanabi_very_small") for n in SIZES] + [("hanabi_full", 65)]


# forward cases past one pass of the world list (1024 worlds): (game, worlds, player, step), each with both weight sets.  They
# are not part of CASES: the margins of the cases above are a maximum over CASES and stay what they were.
#   hanabi_very_small 2081 = 1024 + 1024 + 33: three passes, two carries, a ragged last pass
#   hanabi_full 1025 = 1024 + 1: a last pass of one world; 1025 x 783 elements are past the bookkeeping kernel's 2048 workgroups
#   balance 2081: the int32 inputs
LARGE_CASES = [("hanabi_very_small", 2081, 1, 3), ("hanabi_full", 1025, 0, 3), ("balance", 2081, 1, 3)]

# the forward cases of tests/test_gpu_wide_agent_configs.py: every configuration of tests/hanabi_configs.py at 65 worlds -- three
# 32-row tiles with a last tile of one row, and a head workgroup of one lane --, each with both weight sets.  Not part of
# CASES either; their margins are ``config_margins``, one configuration each.
CONFIG_CASES = [("hanabi_" + cid, 65) for cid in hanabi_configs.IDS]

# (seed, player, world) of hanabi_very_small, 65 worlds, step 0, whose draw sits at an end of the 2^-24 grid (found by search,
# checked by tests/test_wide_agent_api.py through ``draws``)
EDGE_GAME, EDGE_N, EDGE_VARIANTS = "hanabi_very_small", 65, 8
EDGE_DRAWS = {
    "top": [(17086, 1, 13), (98468, 1, 18), (176164, 0, 7), (296419, 0, 11), (680799, 1, 47), (830688, 0, 6)],  # u = 1 - 2^-24
    "zero": [(8124, 1, 45), (455495, 1, 39), (543352, 0, 36), (570769, 1, 25), (659495, 1, 27), (1183274, 0, 17)],  # u = 0
}
EDGE_U = {"top": 1.0 - 2.0 ** -24, "zero": 0.0}


def case_seed(game, n, weights):
    """seed of the inputs and of the draws of one case"""
    named = {"balance": 1, "hanabi_very_small": 2, "hanabi_full": 3}
    last = named[game] if game in named else 10 + hanabi_configs.IDS.index(game[len("hanabi_"):])
    return 7919 * n + 104729 * sorted(WEIGHTS).index(weights) + last


def make_agent(game, weights, seed=AGENT_SEED):
    """A ``WideAgent`` of the game's shape, initialised as the reference's ``layer_init`` does under ``torch.manual_seed``;
    the actor's output layer is multiplied by ``WEIGHTS[weights]``."""
    d, s, a = dims(game)
    torch.manual_seed(seed)
    agent = WideAgent(d, s, a, orthogonal=True)
    with torch.no_grad():
        agent.actor[6].weight.mul_(WEIGHTS[weights])
        for net in (agent.critic, agent.actor):  # (the reference's biases start at zero: move them, or a bias mix-up goes unseen)
            for i in (0, 2, 4, 6):
                net[i].bias.uniform_(-0.1, 0.1)
    return agent


def flat(agent):
    return torch.nn.utils.parameters_to_vector(agent.parameters()).detach().numpy()


def case_inputs(game, n, seed, player=0):
    """What a forward test writes into the simulator's tensors for ``player``: ``state`` (n, S) and ``obs`` = its first D entries
    (Hanabi's OBSERVATION is the head of the STATE row; the balance beam's state is its observation), ``mask`` (n, A) with at
    least one legal action per world, ``active`` (n).  Hanabi values are 0 / 1, the balance beam's 0..8."""
    d, s, a = dims(game)
    rng = np.random.default_rng(seed)
    if game == "balance":
        state = rng.integers(0, 9, size=(n, s)).astype(np.int32)
    else:
        state = (rng.uniform(size=(n, s)) < 0.3).astype(np.int8)
    mask = (rng.uniform(size=(n, a)) < 0.6).astype(np.int32)
    mask[np.arange(n), rng.integers(0, a, size=n)] = 1
    active = (rng.uniform(size=n) < 0.55).astype(np.int32)
    active[0] = 1  # (N = 1 computes something)
    return {"obs": state[:, :d], "state": state, "mask": mask, "active": active}


def narrow_inputs(inputs, d, s, a):
    """what a policy of (d, s, a) reads of a case's inputs: the first d / s / a entries of the rows"""
    return {"obs": inputs["obs"][:, :d], "state": inputs["state"][:, :s], "mask": inputs["mask"][:, :a], "active": inputs["active"]}


def edge_inputs(kind, seed, world, variant=0):
    """The inputs of one edge-draw row: ``case_inputs(EDGE_GAME, EDGE_N, 1000 * variant + seed)`` with ``world`` active and its
    mask set so that the end of the grid decides.  "top": action 0 illegal, 1 .. A - 5 legal, the last four illegal -- the
    exact cumulative sum reaches 1 at action A - 5 and u = 1 - 2^-24 asks for the last legal action, or, where float32
    rounding leaves the sum below u, counts on into the illegal tail.  "zero": the first three actions illegal, action 3
    legal -- u = 0 passes the three empty boundaries and stops at the first legal action."""
    inputs = case_inputs(EDGE_GAME, EDGE_N, 1000 * variant + seed)
    a = inputs["mask"].shape[1]
    inputs["active"][world] = 1
    if kind == "top":
        inputs["mask"][world] = 0
        inputs["mask"][world, 1:a - 4] = 1
    else:
        inputs["mask"][world, :3] = 0
        inputs["mask"][world, 3] = 1
    return inputs


def edge_rows():
    """every edge-draw row of the GPU test: (kind, seed, player, world, variant, the action the header asks for)"""
    a = dims(EDGE_GAME)[2]
    return [("top", seed, player, world, variant, a - 5) for seed, player, world in EDGE_DRAWS["top"] for variant in range(EDGE_VARIANTS)] + \
        [("zero", seed, player, world, 0, 3) for seed, player, world in EDGE_DRAWS["zero"]]


def head32(logits, mask, u):
    """The head's cumulative sum restated in float32, WITHOUT its fallback: the raw count of boundaries at or below u.
    e = the float64 exponential of the float32 difference, rounded once to float32 (a correctly rounded expf, independent of
    any library's vectorised one); the sum, the divides and the running sum are float32, ascending."""
    f = np.float32
    legal = np.asarray(mask) != 0
    logits = np.asarray(logits, f)[:, :legal.shape[1]]  # (a recorded row is MRL_WIDE_MAX_ACTIONS wide)
    u = np.asarray(u, np.float64).astype(f)
    n, a = legal.shape
    count = np.zeros(n, np.int32)
    for w in range(n):
        if not legal[w].any():
            continue
        top = logits[w][legal[w]].max()
        e = np.where(legal[w], np.exp((logits[w] - top).astype(np.float64)), 0.0).astype(f)
        total, cdf = f(0.0), f(0.0)
        for i in range(a):
            total = f(total + e[i])
        for i in range(a - 1):
            cdf = f(cdf + f(e[i] / total))
            count[w] += int(u[w] >= cdf)
    return count


# policies narrower than the simulator's rows: (game, D, S, A).  K = 1 is a single padded product, 2 one unpadded step, 65 a
# chunk of 64 and an odd tail of one; A = 1, 15 and 3 read a mask row whose stride is not A.
NARROW_CASES = [("hanabi_very_small", 1, 65, 1), ("hanabi_very_small", 2, 64, 15), ("hanabi_very_small", 65, 1, 16), ("balance", 5, 5, 3)]
NARROW_N, TIE = 33, (4, 9)  # the two actor outputs of the A = 15 case that share weights and bias


INTEGER_SEED = 4242  # of the ``case_inputs`` the integer-weight GPU cases run on


def integer_layers(d, s, a, seed=99, tie=None):
    """Integer weights and biases of a (d, s, a) policy, the construction of ``test_operand_maps_with_exact_integers``: the first
    layer dense in -2..2, the others one entry in 32, plus a pattern that is asymmetric in row and column.  With ``tie`` =
    (lo, hi) the actor's output row hi is a copy of row lo.  {"critic" / "actor": [(w, b)] * 4} in int64."""
    rng = np.random.default_rng(seed)
    layers = {}
    for name, first, out in (("critic", s, 1), ("actor", d, a)):
        layers[name] = []
        for k, (rows, cols) in enumerate(((H, first), (H, H), (H, H), (out, H))):
            density = 1.0 if k == 0 else 1.0 / 32
            w = (rng.integers(-2, 3, size=(rows, cols)) * (rng.uniform(size=(rows, cols)) < density)).astype(np.int64)
            w += (np.arange(rows)[:, None] % 3 == 0) & (np.arange(cols)[None, :] % 7 == 0)
            b = rng.integers(-3, 4, size=rows).astype(np.int64)
            layers[name].append((w, b))
    if tie:
        w, b = layers["actor"][3]
        w[tie[1]], b[tie[1]] = w[tie[0]], b[tie[0]]
    return layers


def integer_params(layers):
    return np.concatenate([x.reshape(-1) for name in ("critic", "actor") for w, b in layers[name] for x in (w, b)]).astype(np.float32)


def integer_forward(layers, obs, state):
    """(values (n,), logits (n, A)) in int64, and the largest sum of absolute terms over every output of every layer: below
    2^24 every partial sum is an integer float32 holds exactly, in whatever order it is taken"""
    out, bound = {}, 0
    for name, x in (("critic", np.asarray(state, np.int64)), ("actor", np.asarray(obs, np.int64))):
        for k, (w, b) in enumerate(layers[name]):
            bound = max(bound, int((np.abs(x) @ np.abs(w).T + np.abs(b)).max()))
            x = x @ w.T + b
            if k < 3:
                x = np.maximum(x, 0)
        out[name] = x
    return out["critic"][:, 0], out["actor"], bound


def draws(seed, step, n, player):
    """u of every world: ``(hash >> 8) * 2^-24`` of (seed, step, world, player), float64 (exact)"""
    h = random_hash(seed, step, np.arange(n), np.full(n, player))
    return (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def split(params, d, s, a):
    p = np.asarray(params, np.float64)
    at, nets = 0, {}
    for name, first, out in (("critic", s, 1), ("actor", d, a)):
        layers = []
        for rows, cols in ((H, first), (H, H), (H, H), (out, H)):
            w = p[at:at + rows * cols].reshape(rows, cols)
            at += rows * cols
            layers.append((w, p[at:at + rows]))
            at += rows
        nets[name] = layers
    assert at == p.size
    return nets


def forward(params, obs, state, num_actions):
    """values (n,), logits (n, A) in float64"""
    obs, state = np.asarray(obs, np.float64), np.asarray(state, np.float64)
    nets = split(params, obs.shape[1], state.shape[1], num_actions)
    out = []
    for name, x in (("critic", state), ("actor", obs)):
        for k, (w, b) in enumerate(nets[name]):
            x = x @ w.T + b
            if k < 3:
                x = np.maximum(x, 0.0)
        out.append(x)
    return out[0][:, 0], out[1]


def act(params, obs, state, mask, u):
    """The head of include/mrl_envs.h in float64.  ``values``; ``logits``; ``logp`` (n, A), -inf where illegal; ``cdf`` (n, A - 1) the
    boundaries p_0 + ... + p_a; ``actions``; ``greedy`` the first legal arg-max."""
    legal = np.asarray(mask) != 0
    values, logits = forward(params, obs, state, legal.shape[1])
    masked = np.where(legal, logits, -np.inf)
    top = masked.max(axis=1, keepdims=True)
    e = np.where(legal, np.exp(masked - top), 0.0)
    total = e.sum(axis=1, keepdims=True)
    cdf = np.cumsum(e / total, axis=1)[:, :-1]
    actions = (np.asarray(u, np.float64)[:, None] >= cdf).sum(axis=1)
    last_legal = legal.shape[1] - 1 - legal[:, ::-1].argmax(axis=1)
    actions = np.where(legal[np.arange(len(legal)), actions], actions, last_legal).astype(np.int32)
    return {"values": values, "logits": logits, "logp": (masked - top) - np.log(total), "cdf": cdf, "actions": actions,
            "greedy": masked.argmax(axis=1).astype(np.int32)}


def near_boundary(cdf, u, tol=1e-5):
    """rows whose draw lies within ``tol`` of a boundary: the only ones whose action a float32 evaluation may decide otherwise"""
    return (np.abs(np.asarray(u, np.float64)[:, None] - cdf) <= tol).any(axis=1)


def torch_forward32(agent, obs, state, mask):
    """torch's float32 CPU evaluation of ``agent``, as the reference calls it: values (n,), log-probabilities (n, A), float64 arrays"""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(obs)).float()
        s = torch.from_numpy(np.ascontiguousarray(state)).float()
        legal = torch.from_numpy(np.asarray(mask) != 0)
        logits = agent.actor(x).masked_fill(torch.logical_not(legal), -float("inf"))
        return agent.critic(s)[:, 0].double().numpy(), torch.distributions.Categorical(logits=logits).logits.double().numpy()


def margins(agent, inputs, actions=None, twin=None):
    """d per kind on one case's inputs: the largest distance between torch float32 and the twin over the rows, for the values
    and for the log-probability of ``actions`` (default: every legal action).  ``twin``: what ``act`` gave on these inputs with
    the agent's parameters, where the caller has it already (its values and log-probabilities do not depend on the draws)."""
    v32, lp32 = torch_forward32(agent, inputs["obs"], inputs["state"], inputs["mask"])
    if twin is None:
        twin = act(flat(agent), inputs["obs"], inputs["state"], inputs["mask"], np.zeros(len(v32)))
    legal = inputs["mask"] != 0
    if actions is None:
        d_logp = np.abs(np.where(legal, lp32 - np.where(legal, twin["logp"], 0.0), 0.0)).max()
    else:
        rows = np.arange(len(v32))
        d_logp = np.abs(lp32[rows, actions] - twin["logp"][rows, actions]).max()
    return float(np.abs(v32 - twin["values"]).max()), float(d_logp)


@functools.lru_cache(maxsize=None)
def config_margins(game, weights):
    """d of one configuration (a ``CONFIG_CASES`` game) at one weight set: the largest ``margins`` over three input sets of 65 rows,
    ``case_inputs`` at the case's seed, at seed + 1000003 and at seed + 2000006.  One set's value distance is a single draw of
    about one ulp of a value, hence the pool; the three agree within about 30 %."""
    n = dict(CONFIG_CASES)[game]
    agent, seed = make_agent(game, weights), case_seed(game, n, weights)
    per_set = [margins(agent, case_inputs(game, n, seed + 1000003 * k)) for k in range(3)]
    return max(m[0] for m in per_set), max(m[1] for m in per_set)


# ---------------------------------------------------------------- a closed loop on the CPU: the oracle under the twin's actions
#
# What tests/test_gpu_wide_agent_configs.py collects on the device, walked here by the oracle and the twin alone.  WALK_SEEDS:
# the walked configurations and the seed of their draws, chosen so that no active row of the walk lies within 1e-5 of a
# boundary (tests/test_wide_agent_api.py asserts it: a row the device decided otherwise would send the trajectories apart).
# Without a deck or with a deck of 2 most worlds end an episode every few moves; k5r4i8l3 is code variant 0 with A = 19,
# k4r5i5l2 variant 1 with A = 19, k5r5i1l3 A = 20 on a game that is not the full one.
WALK_N, WALK_STEPS = 65, 24
WALK_SEEDS = {"k1r5i1l1": 79, "k3r2i1l1": 77, "k2r4i1l1": 77, "k5r4i8l3": 77, "k4r5i5l2": 79, "k5r5i1l3": 79}


def walk_agents(game):
    """the two seats' policies of a closed loop, the device's collection included: ``make_agent(game, sorted(WEIGHTS)[p], seed=21 + p)``"""
    return [make_agent(game, w, seed=21 + p) for p, w in enumerate(sorted(WEIGHTS))]


def oracle_tensors(game, orc):
    """Copies of what both seats read of an oracle and of what its last step left: "obs", "state", "mask", "active", "reward",
    "done".  The balance beam's state is its observation, its four actions are always legal and both seats act in every world."""
    if game == "balance":
        n = orc.N
        return {"obs": orc.obs.copy(), "state": orc.obs.copy(), "mask": np.ones((2, n, 4), np.int32), "active": np.ones((2, n), np.int32),
                "reward": orc.reward.copy(), "done": orc.done.copy()}
    return {name: getattr(orc, name).copy() for name in ("obs", "state", "mask", "active", "reward", "done")}


def twin_step(game, agents, tensors, seed, t, actions=None):
    """One step's decisions of both seats, by the twin: seat p follows ``act`` with the parameters of ``agents[p]`` on the first D,
    S and A entries of the active rows of ``tensors`` ("obs", "state", "mask", "active" of both seats, (2, n, ...)), with the
    draws ``draws(seed, t, n, p)``.  Per seat {"active", "twin": ``act`` over the active rows, "u": their draws, "d": ``margins`` of
    torch float32 on those rows at ``actions[p]`` (2, n) -- default: at the actions the twin chose --, None where no row is
    active}."""
    d, s, a = dims(game)
    n = tensors["active"].shape[1]
    seats = []
    for p in range(2):
        active = tensors["active"][p] != 0
        inputs = {"obs": tensors["obs"][p][active, :d], "state": tensors["state"][p][active, :s], "mask": tensors["mask"][p][active, :a]}
        u = draws(seed, t, n, p)[active]
        out = act(flat(agents[p]), inputs["obs"], inputs["state"], inputs["mask"], u)
        at = out["actions"] if actions is None else np.asarray(actions)[p][active]
        seats.append({"active": active, "twin": out, "u": u, "d": margins(agents[p], inputs, at, twin=out) if active.any() else None})
    return seats


def twin_walk(game, n, steps, seed):
    """Steps the oracle of ``game`` ("balance" or "hanabi_<configuration id>") under the twin: ``twin_step`` with ``walk_agents`` on the
    oracle's own tensors.  Yields per step {"before" / "after": ``oracle_tensors`` around the step, "actions" (2, n) int32, 0 where
    a seat is not the one to act, "seats": what ``twin_step`` gave}."""
    from oracle import oracle
    oracle.build()
    agents = walk_agents(game)
    orc = oracle.BalanceOracle(n) if game == "balance" else oracle.HanabiOracle(config_of(game), n)
    for t in range(steps):
        before = oracle_tensors(game, orc)
        seats = twin_step(game, agents, before, seed, t)
        actions = np.zeros((2, n), np.int32)
        for p, seat in enumerate(seats):
            actions[p, seat["active"]] = seat["twin"]["actions"]
        orc.step(actions)
        yield {"before": before, "after": oracle_tensors(game, orc), "actions": actions, "seats": seats}
    orc.close()


def config_walk(cid, n, steps, seed):
    """``twin_walk`` of the Hanabi configuration ``cid``: the policies of the device's collection on the oracle's own
    ``obs[:, :D]``, ``state[:, :S]``, ``mask[:, :A]`` and ``active``"""
    return twin_walk("hanabi_" + cid, n, steps, seed)


@functools.lru_cache(maxsize=None)
def walked(cid):
    """the committed walk of ``cid``, walked once and shared: a list, one entry per step"""
    return list(config_walk(cid, WALK_N, WALK_STEPS, WALK_SEEDS[cid]))


# ---------------------------------------------------------------- the closed loop past 1024 worlds, judged step by step
#
# (game, worlds, seed of the draws) of tests/test_gpu_wide_agent_live.py.  2081 = 1024 + 1024 + 33: three passes of the world
# list, three blocks of episode totals with a short last one, nine 256-world workgroups of the Hanabi step and of the
# advantage pass with a last one of 33 worlds.  Among 2081 x 12 rows some lie within 1e-5 of a boundary whatever the seed, so
# the loop is teacher-forced: the oracle is fed the device's actions and ``twin_step`` judges every step on the oracle's
# tensors; a near-boundary row decided otherwise then changes the trajectory that is judged, not the verdict.
# tests/test_wide_agent_api.py asserts on the CPU what the cases are here for:
#   hanabi_k1r5i1l1   episodes of two moves: every block ends hundreds of episodes in every step
#   hanabi_k5r4i8l3   code variant 0, 19 actions; steps without an ended episode, then steps in which blocks 0 and 1 end some and
#                     block 2 none; list lengths between a few dozen and some two thousand
#   hanabi_k2r4i1l1   list lengths around 1024, on either side of it
#   balance           every world in step, both seats active in every row, K = 7
LIVE_STEPS = 12
LIVE_CASES = [("hanabi_k1r5i1l1", 2081, 79), ("hanabi_k5r4i8l3", 2081, 77), ("hanabi_k2r4i1l1", 2081, 77), ("balance", 2081, 77)]
NEAR_CAP = 0.001  # the share of a walk's active rows that may lie within 1e-5 of a boundary


def coupled_across_workgroups(active, next_active, group=256):
    """Whether the advantage pass over a record's ``active`` (T, n) and ``next_active`` (n) is coupled across workgroups of ``group``
    worlds: t* -- the least, over the worlds, of T where a world is bootstrapped and of its last active row where not -- lies
    below T - 1, and some bootstrapped world is active at a row t >= t* that the least of its own workgroup alone lies above.
    A t* taken per workgroup computes that row; the batch's t* leaves it at 0."""
    active, boot = np.asarray(active) != 0, np.asarray(next_active) != 0
    num_steps, n = active.shape
    first = np.where(boot, num_steps, np.where(active.any(axis=0), num_steps - 1 - active[::-1].argmax(axis=0), -1))
    t_star = int(first.min())
    if not 0 <= t_star < num_steps - 1:
        return False
    for start in range(0, n, group):
        own = int(first[start:start + group].min())
        if own > t_star and (active[t_star:own, start:start + group] & boot[start:start + group]).any():
            return True
    return False


# ---------------------------------------------------------------- the record's bookkeeping, float32, operation for operation

def new_record(num_steps, n):
    f, z = np.float32, np.zeros
    return {"active": z((num_steps, n), np.uint8), "dones": z((num_steps, n), f), "rewards": z((num_steps, n), f),
            "last_active": z(n, np.int32), "new_game": z(n, np.uint8), "next_done": z(n, np.uint8), "running_rewards": z(n, f),
            "totals": np.tile(np.array([0.0, 0.0, np.inf, -np.inf]), ((n + 1023) // 1024, 1))}


def book(rec, row, active):
    """the per-world part of a recorded ``mrl_agent_act``"""
    active = np.asarray(active) != 0
    rec["active"][row] = active
    rec["dones"][row] = rec["next_done"].astype(np.float32)
    rec["next_done"][:] = 0
    rec["rewards"][row] = 0.0
    rec["last_active"][active] = row
    rec["new_game"][active] = 0


def credit(rec, rewards, dones):
    """``mrl_agent_credit``; returns the float32 returns of the episodes that finished"""
    r, done = np.asarray(rewards, np.float32), np.asarray(dones) != 0
    n = len(r)
    running = rec["running_rewards"] + r
    w = np.arange(n)
    rec["rewards"][rec["last_active"], w] += np.where(rec["new_game"] != 0, np.float32(0.0), r)
    rec["next_done"][done] = 1
    rec["new_game"][done] = 1
    for b in range((n + 1023) // 1024):
        mine = done[1024 * b:1024 * b + 1024]
        if mine.any():
            finished = running[1024 * b:1024 * b + 1024][mine].astype(np.float64)
            t = rec["totals"][b]
            t[0] += len(finished)
            t[1] += finished.sum()
            t[2], t[3] = min(t[2], finished.min()), max(t[3], finished.max())
    rec["running_rewards"] = np.where(done, np.float32(0.0), running).astype(np.float32)
    return running[done]  # the returns of the episodes that finished, in world order


def gae_active(rewards, values, dones, active, next_done, next_value, next_active, gamma, gae_lambda):
    """``mrl_gae_active`` in float32: (advantages, returns, active afterwards)"""
    f = np.float32
    rewards, values, dones = (np.asarray(a, f) for a in (rewards, values, dones))
    active = (np.asarray(active) != 0).copy()
    num_steps, n = rewards.shape
    gamma32, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    boot = np.asarray(next_active) != 0
    first = np.where(boot, num_steps, np.where(active.any(axis=0), num_steps - 1 - active[::-1].argmax(axis=0), -1))
    t_star = first.min()
    adv = np.zeros((num_steps, n), f)
    for w in range(n):
        b = bool(boot[w])
        nnt = f(1.0) - f(np.asarray(next_done)[w] != 0) if b else f(0.0)
        nv = f(next_value[w]) if b else f(0.0)
        last = f(0.0)
        for t in reversed(range(num_steps)):
            if not active[t, w]:
                continue
            if not b or t < t_star:
                delta = rewards[t, w] + gamma32 * nv * nnt - values[t, w]
                adv[t, w] = last = delta + gl * nnt * last
            if not b:  # the row only carries the bootstrap; the reference's cleared flag also hides it from the two lines below
                active[t, w] = False
                b = True
                continue
            nnt = f(1.0) - dones[t, w]
            nv = values[t, w]
    return adv, adv + values, active


def sum_margin(finished):
    """d of a float64 total of float32 returns: a float32 running sum's distance from it (0 where float32 is exact)"""
    finished = np.asarray(finished, np.float32)
    if finished.size == 0:
        return 0.0
    return abs(float(np.cumsum(finished, dtype=np.float32)[-1]) - float(finished.astype(np.float64).sum()))
