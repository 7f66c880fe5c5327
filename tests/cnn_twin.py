"""Float64 numpy twin of the device-side CNN actor-critic act (``mrl_cnn_act``: both nets and the head), the same function in
torch float32 on the CPU -- whose distance from the twin sets the tests' margins --, the inputs of the GPU cases (observations
of worlds the CPU oracle stepped, and synthetic int8 blocks), the replay of the draws through ``random_hash``, and an
exact-integer construction that pins the operand and index maps.  Nothing here touches a GPU."""
import functools

import numpy as np
import torch

from madrona_rl_envs_playground_amd import layouts
from madrona_rl_envs_playground_amd.simulators import CnnActorCritic, random_hash

A, HIDDEN, CHANNELS = 6, 64, 32
# every forward case of tests/test_gpu_cnn_policy.py: (layout, worlds); N * P is never a multiple of the 32-sample tile
CASES = [("cramped_room", 1), ("cramped_room", 33), ("cramped_room", 257), ("asymmetric_advantages", 33), ("coordination_ring", 65)]
WEIGHTS = ("reference", "trained")
INPUTS = ("stepped", "synthetic")
HORIZON, STEPPED = 400, 7
MODULE_SEED = 23
INTEGER_LAYOUTS = ("cramped_room", "asymmetric_advantages")  # 5 x 4 and 9 x 5
INTEGER_N, TIE = 33, (1, 3)  # the two head rows of the integer actor that share weights and bias

# (seed, seat, world) of 33 worlds, step 0, whose draw sits at an end of the 2^-24 grid (found by search; checked by
# tests/test_cnn_policy_api.py through ``draws``)
EDGE_LAYOUT, EDGE_N = "cramped_room", 33
EDGE_DRAWS = {
    "top": [(17086, 1, 13), (98468, 1, 18), (176164, 0, 7), (296419, 0, 11), (830688, 0, 6), (849194, 1, 24)],  # u = 1 - 2^-24
    "zero": [(570769, 1, 25), (659495, 1, 27), (1183274, 0, 17), (1257010, 0, 3), (1282874, 0, 16), (1327352, 1, 26)],  # u = 0
}
EDGE_U = {"top": 1.0 - 2.0 ** -24, "zero": 0.0}


def shape(layout):
    """(W, H, P, F) of a layout"""
    p = layouts.get_base_layout_params(layout, HORIZON)
    return int(p["width"]), int(p["height"]), int(p["num_players"]), 5 * int(p["num_players"]) + 16


def case_seed(layout, n, weights, inputs):
    """seed of the inputs and of the draws of one case"""
    return 7919 * n + 104729 * WEIGHTS.index(weights) + 1299709 * INPUTS.index(inputs) + sorted(l for l, _ in CASES).index(layout) + 5


@functools.lru_cache(maxsize=None)
def make_module(layout, weights, seed=MODULE_SEED):
    """``reference``: the reference's initialisation under ``torch.manual_seed``.  ``trained``: normal weights of a trained net's
    scale -- He-scaled matrices, a head that spreads the six probabilities, biases of a tenth."""
    w, h, _, f = shape(layout)
    torch.manual_seed(seed)
    module = CnnActorCritic(w, h, f)
    if weights == "trained":
        with torch.no_grad():
            for name, p in module.named_parameters():
                if name.endswith("bias"):
                    p.normal_(0.0, 0.1)
                elif "action_out" in name or "v_out" in name:
                    p.normal_(0.0, 0.3)
                else:
                    p.normal_(0.0, (2.0 / p[0].numel()) ** 0.5)
    return module


def flat(module):
    return torch.nn.utils.parameters_to_vector(module.parameters()).detach().numpy()


def stepped_observations(layout, n, seed, steps=STEPPED, horizon=HORIZON):
    """(N, P, H, W, F) int8 of ``n`` worlds the CPU oracle stepped ``steps`` times with random actions, and those actions
    (steps, P, N) int32: the GPU equals the oracle bit for bit, so a GPU test that replays the actions holds these bytes"""
    from oracle import oracle
    oracle.build()
    w, h, p, f = shape(layout)
    orc = oracle.OvercookedOracle(layouts.get_base_layout_params(layout, horizon), n)
    rng = np.random.default_rng(seed)
    actions = rng.integers(0, 6, size=(steps, p, n)).astype(np.int32)
    for t in range(steps):
        orc.step(actions[t])
    obs = orc.obs.reshape(n, p, h, w, f).astype(np.int8).copy()
    orc.close()
    return obs, actions


def synthetic_observations(layout, n, seed):
    """(N, P, H, W, F) int8: a quarter ones, one entry in 16 a count up to 20, one in 64 negative (-3..-1)"""
    w, h, p, f = shape(layout)
    rng = np.random.default_rng(seed)
    size = (n, p, h, w, f)
    obs = (rng.uniform(size=size) < 0.25).astype(np.int8)
    counts = rng.integers(0, 21, size=size).astype(np.int8)
    obs = np.where(rng.uniform(size=size) < 1.0 / 16, counts, obs)
    obs = np.where(rng.uniform(size=size) < 1.0 / 64, rng.integers(-3, 0, size=size).astype(np.int8), obs)
    return obs.astype(np.int8)


@functools.lru_cache(maxsize=None)
def case_inputs(layout, n, weights, inputs):
    """{"obs": (N, P, H, W, F) int8, "actions": the oracle's action stream or None} -- shared, never modified"""
    seed = case_seed(layout, n, weights, inputs)
    if inputs == "stepped":
        obs, actions = stepped_observations(layout, n, seed)
    else:
        obs, actions = synthetic_observations(layout, n, seed), None
    obs.setflags(write=False)
    return {"obs": obs, "actions": actions}


def rows_of(obs):
    """the samples of a block in the kernel's order (n, p): (N * P, H, W, F)"""
    return obs.reshape((-1,) + obs.shape[2:])


def draws(seed, step, n, num_players, players=None):
    """u of every sample (N * P,): ``(hash >> 8) * 2^-24`` of (seed, step, world, seat), float64 (exact)"""
    world = np.repeat(np.arange(n), num_players)
    seat = np.tile(np.arange(num_players), n)
    h = random_hash(seed, step, world, seat)
    return (h >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def split(params, w, h, f):
    """{"actor" / "critic": [(weight, bias)] * 4} in float64, in parameters_to_vector order"""
    p = np.asarray(params, np.float64)
    npos = (w - 2) * (h - 2)
    at, nets = 0, {}
    for name, out in (("actor", A), ("critic", 1)):
        layers = []
        for wshape in ((CHANNELS, f, 3, 3), (HIDDEN, CHANNELS * npos), (HIDDEN, HIDDEN), (out, HIDDEN)):
            count = int(np.prod(wshape))
            weight = p[at:at + count].reshape(wshape)
            at += count
            layers.append((weight, p[at:at + wshape[0]]))
            at += wshape[0]
        nets[name] = layers
    assert at == p.size
    return nets


def net_forward(layers, rows, relu_bound=None):
    """One net on rows (n, H, W, F): torch sees x[n, f, w, h] = rows[n, h, w, f]; conv[n, c, ow, oh] = bc[c] + sum over (f, i, j) of
    Wc[c, f, i, j] * rows[n, oh + j, ow + i, f]; the flattened index is c * npos + ow * (H - 2) + oh.  Works in the dtype of the
    layers (float64, or int64 for the integer construction).  ``relu_bound``: a one-element list that takes the largest sum of
    absolute terms over every output of every layer."""
    dtype = layers[0][0].dtype
    x = np.asarray(rows).astype(dtype).transpose(0, 3, 2, 1)  # (n, f, w, h)
    patches = np.lib.stride_tricks.sliding_window_view(x, (3, 3), axis=(2, 3))  # (n, f, ow, oh, i, j)
    (wc, bc), rest = layers[0], layers[1:]
    if relu_bound is not None:
        relu_bound[0] = max(relu_bound[0], int((np.einsum("nfxyij,cfij->ncxy", np.abs(patches), np.abs(wc)) + np.abs(bc)[None, :, None, None]).max()))
    y = np.einsum("nfxyij,cfij->ncxy", patches, wc) + bc[None, :, None, None]
    y = np.maximum(y, 0).reshape(len(rows), -1)
    for k, (weight, bias) in enumerate(rest):
        if relu_bound is not None:
            relu_bound[0] = max(relu_bound[0], int((np.abs(y) @ np.abs(weight).T + np.abs(bias)).max()))
        y = y @ weight.T + bias
        if k < 2:
            y = np.maximum(y, 0)
    return y


def forward(params, rows):
    """values (n,), logits (n, 6) in float64 of rows (n, H, W, F)"""
    _, h, w, f = rows.shape
    nets = split(params, w, h, f)
    return net_forward(nets["critic"], rows)[:, 0], net_forward(nets["actor"], rows)


def act(params, rows, u):
    """The head of include/mrl_envs.h in float64: ``values``; ``logits``; ``logp`` (n, 6); ``cdf`` (n, 5) the boundaries p_0 + ... +
    p_a; ``actions``; ``greedy`` the first arg-max."""
    values, logits = forward(params, rows)
    top = logits.max(axis=1, keepdims=True)
    e = np.exp(logits - top)
    total = e.sum(axis=1, keepdims=True)
    cdf = np.cumsum(e / total, axis=1)[:, :-1]
    actions = (np.asarray(u, np.float64)[:, None] >= cdf).sum(axis=1).astype(np.int32)
    return {"values": values, "logits": logits, "logp": (logits - top) - np.log(total), "cdf": cdf, "actions": actions,
            "greedy": logits.argmax(axis=1).astype(np.int32)}


def near_boundary(cdf, u, tol=1e-5):
    """rows whose draw lies within ``tol`` of a boundary: the only ones whose action a float32 evaluation may decide otherwise"""
    return (np.abs(np.asarray(u, np.float64)[:, None] - cdf) <= tol).any(axis=1)


def torch_forward32(module, rows):
    """torch's float32 CPU evaluation, as the reference calls it (the (N, W, H, F) view, cast to float): values (n,) and
    log-probabilities (n, 6) as float64 arrays"""
    with torch.no_grad():
        x = torch.from_numpy(np.array(rows)).transpose(1, 2).float()
        logits = module.actor(x)
        return module.critic(x)[:, 0].double().numpy(), torch.distributions.Categorical(logits=logits).logits.double().numpy()


def margins(module, rows):
    """d per kind on one case's rows: the largest distance between torch float32 and the twin, for the values and for the
    log-probability of every action"""
    v32, lp32 = torch_forward32(module, rows)
    twin = act(flat(module), rows, np.zeros(len(rows)))
    return float(np.abs(v32 - twin["values"]).max()), float(np.abs(lp32 - twin["logp"]).max())


@functools.lru_cache(maxsize=None)
def case_margins(layout, n, weights, inputs):
    return margins(make_module(layout, weights), rows_of(case_inputs(layout, n, weights, inputs)["obs"]))


@functools.lru_cache(maxsize=None)
def layout_margins(layout, weights):
    """d of a layout at one weight set: the largest over the layout's cases and inputs (as tests/wide_twin.py's users take it)"""
    per_case = [case_margins(l, n, weights, inputs) for l, n in CASES if l == layout for inputs in INPUTS]
    return max(m[0] for m in per_case), max(m[1] for m in per_case)


# ---------------------------------------------------------------- the exact-integer construction

def integer_layers(layout, seed=99):
    """Small integer weights and biases for both nets: the conv weights differ from one (c, f, i, j) to the next along every axis
    (a residue pattern plus noise), fc1's differ from column to column and are one in 16, fc2 and the head are one in 8.  The
    actor's head is non-positive except rows TIE, which are equal and non-negative: on non-negative h2 both are the arg-max."""
    w, h, _, f = shape(layout)
    npos = (w - 2) * (h - 2)
    rng = np.random.default_rng(seed)
    layers = {}
    for name, out in (("actor", A), ("critic", 1)):
        c, ff, i, j = np.meshgrid(np.arange(CHANNELS), np.arange(f), np.arange(3), np.arange(3), indexing="ij")
        conv = ((c * 131 + ff * 31 + i * 7 + j * 3) % 9 - 4 + rng.integers(-1, 2, size=c.shape)).astype(np.int64)
        k2 = CHANNELS * npos
        o, k = np.meshgrid(np.arange(HIDDEN), np.arange(k2), indexing="ij")
        fc1 = (((o * 17 + k * 5) % 7 - 3) * (rng.uniform(size=o.shape) < 1.0 / 16)).astype(np.int64)
        fc2 = (rng.integers(-1, 2, size=(HIDDEN, HIDDEN)) * (rng.uniform(size=(HIDDEN, HIDDEN)) < 1.0 / 8)).astype(np.int64)
        head = (rng.integers(1, 3, size=(out, HIDDEN)) * (rng.uniform(size=(out, HIDDEN)) < 1.0 / 8)).astype(np.int64)
        head_bias = rng.integers(0, 4, size=out).astype(np.int64)
        if name == "actor":
            head, head_bias = -head, -head_bias
            head[TIE[0]] = head[TIE[1]] = np.abs(head[TIE[0]]) + (np.arange(HIDDEN) % 5 == 0)
            head_bias[TIE[0]] = head_bias[TIE[1]] = 2
        layers[name] = [(conv, rng.integers(-3, 4, size=CHANNELS).astype(np.int64)),
                        (fc1, rng.integers(-3, 4, size=HIDDEN).astype(np.int64)),
                        (fc2, rng.integers(-3, 4, size=HIDDEN).astype(np.int64)), (head, head_bias)]
    return layers


def integer_params(layers):
    return np.concatenate([x.reshape(-1) for name in ("actor", "critic") for weight, bias in layers[name] for x in (weight, bias)]).astype(np.float32)


def integer_observations(layout, n=INTEGER_N, seed=5):
    """(N, P, H, W, F) int8 in -1..3, one entry in five nonzero"""
    w, h, p, f = shape(layout)
    rng = np.random.default_rng(seed)
    size = (n, p, h, w, f)
    return (rng.integers(-1, 4, size=size) * (rng.uniform(size=size) < 0.2)).astype(np.int8)


def integer_forward(layers, rows):
    """(values (n,), logits (n, 6)) in int64 and the largest sum of absolute terms over every output of every layer: below 2^24
    every partial sum is an integer float32 holds exactly, in whatever order it is taken"""
    bound = [0]
    values = net_forward(layers["critic"], rows, bound)[:, 0]
    logits = net_forward(layers["actor"], rows, bound)
    return values, logits, bound[0]


# ---------------------------------------------------------------- float32 restatement of mrl_gae (include/mrl_envs.h)

def gae32(rewards, values, dones, next_value, next_done, gamma, gae_lambda):
    f = np.float32
    rewards, values, dones = (np.asarray(a, f) for a in (rewards, values, dones))
    num_steps = rewards.shape[0]
    gamma32, gl = f(gamma), f(float(gamma) * float(gae_lambda))
    adv = np.zeros_like(rewards)
    nextvalue, nextdone, last = np.asarray(next_value, f), np.asarray(next_done, f), np.zeros(rewards.shape[1], f)
    for t in reversed(range(num_steps)):
        nnt = f(1.0) - nextdone
        delta = rewards[t] + gamma32 * nextvalue * nnt - values[t]
        last = delta + gl * nnt * last
        adv[t] = last
        nextvalue, nextdone = values[t], dones[t]
    return adv, adv + values
