"""GPU: ``agent_update`` (mrl_agent_update: list, forward, loss head, backward, clip + Adam) against the float64 twin of
tests/wide_update_twin.py, and ``CleanPPOAgent`` with ``device_update = True``.

Margins: d is the distance of torch's float32 CPU run of the same epoch from the twin; the device must be within 8 d.  For a
gradient, parameters and moments d is the largest over the elements of the case at hand; for a scalar stat, of which one case
holds a single draw of a rounding error, it is the largest over ``wide_update_twin.CASES`` at the same weight set and flags
(``stat_margins``).  d never comes from the device.  The batches are synthetic records filled on the
host, whose samples meet the input conditions tests/test_agent_update_api.py asserts: no hidden pre-activation within 8 x the
float32-vs-twin pre-activation distance of 0, no sample within 1e-5 of a kink of the loss, a quarter at least on either clipped
branch.  Each test prints the ratios it measured."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wide_twin  # noqa: E402
import wide_update_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import (AgentRecord, BalanceBeamSimulator, ExecMode, HanabiSimulator,  # noqa: E402
                                                         WideOptimizer, WidePolicy, agent_act, agent_credit, agent_update)

DEV = torch.device("cuda", 0)
WEIGHTS = sorted(wide_twin.WEIGHTS)
COL = {name: i for i, name in enumerate(twin.STATS)}
RECORD_ARRAYS = ("obs", "states", "action_masks", "active", "actions", "logprobs", "values", "advantages", "returns")


def cuda(array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(DEV)


def cpu(tensor):
    return tensor.cpu().numpy().copy()


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what} differs"


class Device:
    """A policy, its optimizer and a record (numpy arrays by name, ``wide_update_twin.make_record``) on the GPU."""

    def __init__(self, params, rec, cfg, step=0, moments=None):
        steps, n = rec["active"].shape
        d, s, a = rec["obs"].shape[2], rec["states"].shape[2], rec["action_masks"].shape[2]
        self.policy = WidePolicy(d, s, a, device=DEV)
        self.policy.params.copy_(cuda(np.asarray(params, np.float32)))
        self.optimizer = WideOptimizer(self.policy, lr=cfg.lr, betas=(cfg.beta1, cfg.beta2), eps=cfg.eps)
        self.optimizer.step = step
        if moments is not None:
            self.optimizer.exp_avg.copy_(cuda(moments[0]))
            self.optimizer.exp_avg_sq.copy_(cuda(moments[1]))
        self.cfg = cfg
        self.record = AgentRecord(steps, n, d, s, a, torch.from_numpy(rec["obs"]).dtype, torch.from_numpy(rec["states"]).dtype, DEV)
        for name in RECORD_ARRAYS:
            getattr(self.record, name).copy_(cuda(rec[name]))

    def update(self, epochs=1, grads=True, capacity=None):
        c = self.cfg
        result = agent_update(self.policy, self.optimizer, self.record, epochs=epochs, clip_coef=c.clip_coef, ent_coef=c.ent_coef,
                              vf_coef=c.vf_coef, max_grad_norm=c.max_grad_norm, norm_adv=c.norm_adv, clip_vloss=c.clip_vloss,
                              capacity=capacity, stats=True, grads=grads)
        return cpu(result.stats), cpu(result.grads) if grads else None

    def state(self):
        return cpu(self.policy.params), cpu(self.optimizer.exp_avg), cpu(self.optimizer.exp_avg_sq)


def check_row(what, got_stats, got_grad, exact, single, size, stat_d):
    """One stats row and gradient of the device against the twin's epoch ``exact``; ``single`` is float32's."""
    d_grad = twin.distance(single["grad"], exact["grad"])
    ratios = {"grad": twin.distance(got_grad, exact["grad"]) / d_grad}
    for name in twin.LOSS_STATS:
        ratios[name] = abs(float(got_stats[COL[name]]) - exact["stats"][name]) / stat_d[name]
    print(what, "measured / d:", {k: round(v, 2) for k, v in ratios.items()}, "d(grad) = %.2e" % d_grad)
    assert got_stats[COL["samples"]] == size and got_stats[COL["status"]] == 0, what
    assert got_stats[COL["clipfrac"]] == np.float32(round(exact["stats"]["clipfrac"] * size) / size), what
    for name, ratio in ratios.items():
        assert ratio <= twin.FACTOR, (what, name, ratio)


def run_parity(game, weights, size, flags=()):
    batch, exact, single = twin.parity(game, weights, size, flags)
    steps, n = twin.record_shape(size)
    rec = twin.make_record(batch, steps, n, batch["seed"])
    assert rec["active"].sum() == size < steps * n
    dev = Device(batch["params"], rec, twin.config(**dict(flags)))
    stats, grads = dev.update()
    check_row(f"{game} {weights} B={size} {dict(flags)}", stats[0], grads[0], exact, single, size, twin.stat_margins(weights, flags))
    return dev, batch, rec, stats, grads


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,size", twin.CASES)
def test_gradient_and_stats_parity(game, size, weights, hip_lib):
    """Guards every kernel of an epoch: int32 rows with K = 7 (balance) and int8 rows with D = 187 odd, S = 212 (Hanabi) through
    the gather; B = 2 one sample pair, 31 / 33 either side of a 32-row tile, 65 three tiles and an odd tail, 257 more than one
    workgroup of the loss head; hanabi_full 658 / 783 / 20."""
    run_parity(game, weights, size)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,size,flags", twin.FLAG_CASES)
def test_flag_variants(game, size, flags, weights, hip_lib):
    """NORM_ADV off once and CLIP_VLOSS off once: the raw advantages, and the plain value loss."""
    run_parity(game, weights, size, tuple(sorted(flags.items())))


def test_list_of_more_than_one_pass(hip_lib):
    """A record of 5 x 257 = 1285 cells, more than one pass of 1024 of the list kernel, with 257 active cells on both sides of
    the pass boundary: the list read back from the workspace is the ascending active cells and the gradient is the twin's.  A
    carry dropped between the passes fails here."""
    game, weights, size = "hanabi_very_small", "orthogonal", 257
    batch, exact, single = twin.parity(game, weights, size)
    rec = twin.make_record(batch, 5, 257, 3)
    assert (rec["cells"] < 1024).sum() > 32 and (rec["cells"] >= 1024).sum() > 32
    dev = Device(batch["params"], rec, twin.config())
    stats, grads = dev.update()
    torch.cuda.synchronize()
    words = dev.optimizer._workspace.view(torch.int32)
    same_bits(cpu(words[:size]), rec["cells"].astype(np.int32), "the sample list")
    slot = (5 * 257 * 4 + 255) // 256 * 256 // 4  # behind the list of `capacity` = T N entries
    assert cpu(words[slot:slot + 3]).tolist() == [size, size, 0]
    check_row("1285 cells", stats[0], grads[0], exact, single, size, twin.stat_margins(weights))


def make_sim(game, n):
    if game == "balance":
        return BalanceBeamSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n)
    c = wide_twin.config_of(game)
    return HanabiSimulator(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, colors=c["colors"], ranks=c["ranks"], players=c["players"],
                           max_information_tokens=c["max_information_tokens"], max_life_tokens=c["max_life_tokens"])


@pytest.mark.parametrize("game", ["balance", "hanabi_very_small"])
def test_recompute_is_the_acts(game, hip_lib):
    """On a record filled by real ``agent_act`` calls, the env stepped in between, the first epoch on unchanged parameters
    recomputes the record's own log-probs and values bit for bit: both KL estimates and clipfrac are exactly 0, and with the
    record's values as returns and CLIP_VLOSS off the value loss and the critic's gradient are exactly 0.  Any forward pass that
    is not the act's chain fails here."""
    n, steps = 33, 4
    d, s, a = wide_twin.dims(game)
    sim = make_sim(game, n)
    policy = WidePolicy.from_module(wide_twin.make_agent(game, "peaked", seed=21), device=DEV)
    other = WidePolicy.from_module(wide_twin.make_agent(game, "orthogonal", seed=22), device=DEV)
    record = AgentRecord(steps, n, d, s, a, sim.observation_tensor().to_torch().dtype, sim.agent_state_tensor().to_torch().dtype, DEV)
    for t in range(steps):
        agent_act(sim, 0, policy, record, row=t, seed=9, step=t)
        agent_act(sim, 1, other, None, seed=9, step=t, workspace=record.workspace)
        sim.step()
        agent_credit(record, sim.reward_tensor().to_torch()[0], sim.done_tensor().to_torch())
    size = int(record.active.sum())
    assert 2 <= size and (size < steps * n or game == "balance")  # (on the beam both seats act in every step)
    optimizer = WideOptimizer(policy)
    advantages = cuda(np.random.default_rng(1).normal(size=(steps, n)).astype(np.float32))
    result = agent_update(policy, optimizer, record, advantages, record.values.clone(), epochs=1, clip_vloss=False, grads=True)
    stats, grad = cpu(result.stats)[0], cpu(result.grads)[0]
    sim.close()
    assert stats[COL["samples"]] == size and stats[COL["status"]] == 0
    for name in ("approx_kl", "old_approx_kl", "clipfrac", "v_loss"):
        assert stats[COL[name]] == 0, (name, stats[COL[name]])
    critic = int(_lib.lib().mrl_wide_policy_num_params(d, s, a)) - (d * 512 + 512 + 2 * (512 * 512 + 512) + 512 * a + a)
    assert not grad[:critic].any() and grad[critic:].any()


@pytest.mark.parametrize("size", [32, 64])
def test_operand_maps_with_exact_integers(size, hip_lib):
    """Integer weights, inputs and returns, B a power of two: every product and partial sum of the critic's backward pass is
    an integer over B that float32 holds exactly, so the critic's gradient is the twin's bit for bit whatever the order -- and
    any wrong row, column or sample in the operand maps of either backward product changes it."""
    params, rec, expected, bound = twin.integer_case(size)
    assert bound < 2 ** 24
    cfg = twin.config(norm_adv=False, clip_vloss=False, vf_coef=1.0)
    dev = Device(params, rec, cfg)
    stats, grads = dev.update()
    assert stats[0][COL["samples"]] == size
    same_bits(grads[0][:len(expected)], expected.astype(np.float32), "the critic's gradient")
    assert np.count_nonzero(expected) > len(expected) // 8


@pytest.mark.parametrize("step,lr,max_grad_norm", [(0, 2.5e-4, 0.05), (7, 2.5e-4, 0.05), (7, 1e-2, 0.0), (0, 1e-2, 100.0)])
def test_the_step_on_the_devices_own_gradient(step, lr, max_grad_norm, hip_lib):
    """clip_grad_norm_ and Adam: from the device's own gradient row ``update_twin.clip_adam`` reproduces the parameters, both
    moments and total_norm within 8 d, d = float32 torch's distance from float64 torch on the same step.  0.05 clips (the norm
    is asserted to be above it), 100 does not, 0 turns clipping off; steps 0 and 7 differ in the bias corrections."""
    import update_twin
    game, weights, size = "hanabi_very_small", "peaked", 65
    batch, _, _ = twin.parity(game, weights, size)
    cfg = twin.config(lr=lr, max_grad_norm=max_grad_norm)
    steps, n = twin.record_shape(size)
    moments = update_twin.moments(len(batch["params"]), 5)
    dev = Device(batch["params"], twin.make_record(batch, steps, n, batch["seed"]), cfg, step=step, moments=moments)
    stats, grads = dev.update()
    got = dev.state()
    clip = max_grad_norm if max_grad_norm > 0 else None
    want = update_twin.clip_adam(batch["params"], moments[0], moments[1], grads[0], step, clip, lr, cfg)
    single = update_twin.clip_adam_torch(batch["params"], moments[0], moments[1], grads[0], step, clip, lr, cfg, torch.float32)
    exact = update_twin.clip_adam_torch(batch["params"], moments[0], moments[1], grads[0], step, clip, lr, cfg, torch.float64)
    ratios = {}
    for i, name in enumerate(("total_norm", "params", "exp_avg", "exp_avg_sq")):
        value = stats[0][COL["total_norm"]] if i == 0 else got[i - 1]
        d = twin.distance(single[i], exact[i])
        if i == 0:
            d = max(d, float(np.spacing(np.float32(want[0]))) / 2)  # a scalar: half an ulp where torch's float32 norm happens to be exact
        ratios[name] = twin.distance(value, want[i]) / d
    print(f"step {step} lr {lr} clip {max_grad_norm}: measured / d", {k: round(v, 2) for k, v in ratios.items()},
          "total_norm %.3f" % want[0])
    assert 0.05 < want[0] < 100 and all(r <= twin.FACTOR for r in ratios.values()), ratios
    assert dev.optimizer.step == step + 1


@functools.lru_cache(maxsize=None)
def three_epochs():
    """one call of three epochs on one case, shared: (batch, record, stats, grads, state afterwards)"""
    game, weights, size = "hanabi_very_small", "peaked", 65
    batch, _, _ = twin.parity(game, weights, size)
    steps, n = twin.record_shape(size)
    rec = twin.make_record(batch, steps, n, batch["seed"])
    dev = Device(batch["params"], rec, twin.config(lr=1e-3))
    stats, grads = dev.update(epochs=3)
    return batch, rec, stats, grads, dev.state()


def test_three_epochs_teacher_forced(hip_lib):
    """Rows 1 and 2 against something that is not the device: the twin takes the device's three gradients through its own
    clip and Adam, and each row's losses must be the twin's losses at the twin's parameters after k steps, within 8 d (d: float32
    torch at those parameters)."""
    batch, rec, stats, grads, _ = three_epochs()
    cfg = twin.config(lr=1e-3)
    p, m, v = batch["params"].astype(np.float64), np.zeros(len(batch["params"])), np.zeros(len(batch["params"]))
    for k in range(3):
        exact, single = twin.epoch(p, batch, cfg, torch.float64), twin.epoch(p.astype(np.float32), batch, cfg, torch.float32)
        ratios, moved = {}, False
        for name in ("pg_loss", "v_loss", "entropy", "approx_kl"):
            d = max(abs(single["stats"][name] - exact["stats"][name]), twin.stat_margins("peaked")[name])
            ratios[name] = abs(float(stats[k][COL[name]]) - exact["stats"][name]) / d
            moved = moved or (k > 0 and abs(exact["stats"][name] - first[name]) > 100 * twin.FACTOR * d)
        print(f"epoch {k}: measured / d", {name: round(r, 2) for name, r in ratios.items()})
        assert all(r <= twin.FACTOR for r in ratios.values()), (k, ratios)
        if k:
            assert moved  # the parameters moved: a row that repeats row 0 fails
        else:
            first = exact["stats"]
        _, p, m, v = twin.step(p, m, v, grads[k], k, cfg)


def test_reproducibility(hip_lib):
    """One call of three epochs, three calls of one, a second run and a side stream: equal bytes of parameters, moments, stats
    and gradients."""
    batch, rec, stats, grads, state = three_epochs()
    cfg = twin.config(lr=1e-3)

    def compare(what, got_stats, got_grads, got_state):
        same_bits(got_stats, stats, f"{what}: stats")
        same_bits(got_grads, grads, f"{what}: grads")
        for a, b, name in zip(got_state, state, ("params", "exp_avg", "exp_avg_sq")):
            same_bits(a, b, f"{what}: {name}")
    dev = Device(batch["params"], rec, cfg)
    rows = [dev.update() for _ in range(3)]
    assert dev.optimizer.step == 3
    compare("three calls of one", np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), dev.state())
    dev = Device(batch["params"], rec, cfg)
    compare("a second run", *dev.update(epochs=3), dev.state())
    dev = Device(batch["params"], rec, cfg)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = dev.update(epochs=3)
    compare("a side stream", *got, dev.state())


def test_status_rows(hip_lib):
    """B = 0 and B = 1 report status 1, capacity = B - 1 status 2; in each the parameters, the moments and the gradient rows keep
    their bytes and the loss columns are 0.  capacity = B runs."""
    import update_twin
    game, weights, size = "balance", "orthogonal", 33
    batch, _, _ = twin.parity(game, weights, size)
    steps, n = twin.record_shape(size)
    full = twin.make_record(batch, steps, n, batch["seed"])
    moments = update_twin.moments(len(batch["params"]), 6)
    for what, keep, capacity, status in (("B = 0", 0, None, 1), ("B = 1", 1, None, 1), ("capacity = B - 1", size, size - 1, 2),
                                         ("capacity = B", size, size, 0)):
        rec = dict(full)
        active = np.zeros(steps * n, np.uint8)
        active[full["cells"][:keep]] = 1
        rec["active"] = active.reshape(steps, n)
        dev = Device(batch["params"], rec, twin.config(), step=3, moments=moments)
        before = dev.state()
        # the rows go to tensors of the test's own, filled with 7, so that untouched bytes can be told from written ones
        marker = torch.full((2, len(batch["params"])), 7.0, device=DEV)
        raw_stats = torch.full((2, 10), 7.0, device=DEV)
        assert raw_update(dev, 2, capacity if capacity is not None else steps * n, raw_stats, marker) == _lib.MRL_OK
        stats = cpu(raw_stats)
        assert (stats[:, COL["samples"]] == keep).all() and (stats[:, COL["status"]] == status).all(), what
        if status:
            assert not stats[:, :8].any(), what
            assert (cpu(marker) == 7.0).all(), what
            for a, b, name in zip(dev.state(), before, ("params", "exp_avg", "exp_avg_sq")):
                same_bits(a, b, f"{what}: {name}")
        else:
            assert stats[:, :8].all() and not (cpu(marker) == 7.0).all() and not np.array_equal(dev.state()[0], before[0])


def raw_update(dev, epochs, capacity, stats, grads, workspace=None, stream=None):
    """``mrl_agent_update`` itself, with a workspace of the caller's"""
    c, p, o = dev.cfg, dev.policy, dev.optimizer
    if workspace is None:
        workspace = o.workspace(capacity)
    desc = p.desc()
    opt = _lib.PpoOptimizerDesc(p.params.data_ptr(), o.exp_avg.data_ptr(), o.exp_avg_sq.data_ptr(), o.step)
    cfg = _lib.PpoConfig(c.clip_coef, c.ent_coef, c.vf_coef, c.max_grad_norm, o.lr, o.betas[0], o.betas[1], o.eps,
                         (_lib.PPO_NORM_ADV if c.norm_adv else 0) | (_lib.PPO_CLIP_VLOSS if c.clip_vloss else 0))
    r = dev.record
    types = {torch.int8: _lib.MRL_INT8, torch.int32: _lib.MRL_INT32}
    return _lib.lib().mrl_agent_update(ctypes.byref(desc), ctypes.byref(opt), ctypes.byref(r.struct), types[r.obs.dtype],
                                       types[r.states.dtype], r.advantages.data_ptr(), r.returns.data_ptr(), epochs, ctypes.byref(cfg),
                                       capacity, workspace.data_ptr(), workspace.numel(), stats.data_ptr(), grads.data_ptr(), 0,
                                       stream if stream is not None else torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("size", [33, 257])
def test_an_update_stays_inside_its_workspace(size, hip_lib):
    """``mrl_agent_update_workspace_bytes(capacity = B)`` bytes between two 4096-byte guards of 0xA5: the guards are intact and
    the results carry the bits of a run in a larger workspace."""
    game, weights = "hanabi_very_small", "orthogonal"
    batch, _, _ = twin.parity(game, weights, size)
    steps, n = twin.record_shape(size)
    rec = twin.make_record(batch, steps, n, batch["seed"])
    cfg = twin.config()
    roomy = Device(batch["params"], rec, cfg)
    want_stats, want_grads = roomy.update()  # capacity T N
    dev = Device(batch["params"], rec, cfg)
    need = dev.optimizer.workspace_bytes(size)
    assert need < roomy.optimizer.workspace_bytes(steps * n) and need % 256 == 0
    guarded = torch.full((need + 8192,), 0xA5, dtype=torch.uint8, device=DEV)
    stats, grads = torch.zeros(1, 10, device=DEV), torch.zeros(1, len(batch["params"]), device=DEV)
    assert raw_update(dev, 1, size, stats, grads, workspace=guarded[4096:4096 + need]) == _lib.MRL_OK
    torch.cuda.synchronize()
    assert (cpu(guarded[:4096]) == 0xA5).all() and (cpu(guarded[4096 + need:]) == 0xA5).all()
    same_bits(cpu(stats), want_stats, "stats")
    same_bits(cpu(grads), want_grads, "grads")
    for a, b, name in zip(dev.state(), roomy.state(), ("params", "exp_avg", "exp_avg_sq")):
        same_bits(a, b, name)


def rollout(env, ego, num_steps, obs):
    for _ in range(num_steps):
        action = ego.get_action(obs)
        obs, reward, done, _ = env.step(action)
        ego.update(reward, done)
    return obs


@pytest.mark.parametrize("game", ["hanabi_very_small", "balance"])
def test_clean_ppo_agent_with_the_update_on_the_device(game, hip_lib):
    """Two updates of ``CleanPPOAgent`` with ``device_update = True``: finite losses under the torch path's keys, ``samples`` the number
    of active cells, the parameters changed in place (the act behind the update and ``agent.agent`` read them), and the first
    update's losses within 8 d of the twin run on the record read back."""
    from madrona_rl_envs_playground_amd.envs import BalanceMadronaTorch
    from madrona_rl_envs_playground_amd.envs.hanabi_env import HanabiMadrona
    from madrona_rl_envs_playground_amd.pantheonrl_extension import CleanPPOAgent
    n, num_steps = 33, 8
    torch.manual_seed(0)
    env = BalanceMadronaTorch(n, 0) if game == "balance" else HanabiMadrona(n, 0, config=wide_twin.config_of(game))
    kwargs = dict(num_updates=2, verbose=False, num_steps=num_steps, anneal_lr=False)
    ego = CleanPPOAgent(env, "ego", DEV, seed=5, **kwargs)
    partner = CleanPPOAgent(env.getDummyEnv(1), "partner", DEV, **kwargs)
    env.add_partner_agent(partner, player_num=1)
    assert isinstance(ego.optimizer, torch.optim.Adam) and not ego.device_update  # the default is the torch path
    ego.device_update = True
    assert isinstance(ego.optimizer, WideOptimizer) and isinstance(partner.optimizer, torch.optim.Adam)
    torch_keys = {"value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac", "explained_variance",
                  "learning_rate", "samples"}
    before, where = ego.policy.params.clone(), ego.policy.params.data_ptr()
    obs = env.reset()
    for update in (1, 2):
        previous = ego.policy.params.clone()
        obs = rollout(env, ego, num_steps, obs)
        ego.step = 0
        ego._learn()  # the update boundary of get_action, without the act behind it: the record stays as the update saw it
        torch.cuda.synchronize()
        after = ego.policy.params
        assert ego.updates == update + 1 and ego.optimizer.step == update * ego.update_epochs
        assert not torch.equal(after, previous) and torch.isfinite(after).all() and after.data_ptr() == where
        first = next(ego.agent.parameters())  # the aliasing module sees the new parameters
        assert first.data_ptr() == after.data_ptr() and torch.equal(first.reshape(-1), after[:first.numel()])
        assert set(ego.last_losses) == torch_keys and set(partner.last_losses) in (set(), torch_keys)
        for key, value in ego.last_losses.items():
            assert np.isfinite(value) or key == "explained_variance", key
        assert ego.last_losses["samples"] == int(ego.record.active.sum()) > 1
        ego.global_step = 0  # the boundary is behind us: the next get_action is row 0 of a rollout and must not update again
    # the act after the update reads the new parameters: its values are the new parameters', not the old ones'
    ego.get_action(obs)
    torch.cuda.synchronize()
    r = ego.record
    active = cpu(r.active)[0] != 0
    d, s, a = wide_twin.dims(game)
    values = cpu(r.values)[0][active]
    new_twin, old_twin = (wide_twin.forward(cpu(p).astype(np.float64), cpu(r.obs)[0][active], cpu(r.states)[0][active], a)[0]
                          for p in (ego.policy.params, previous))
    assert np.abs(values - new_twin).max() < 0.01 * np.abs(values - old_twin).max()
    env.close()

    # the first update's losses against the twin: a fresh agent of one epoch on the first agent's initial parameters, its own
    # rollout, and the record read back behind the update, which reads the record and does not write it
    torch.manual_seed(0)
    env = BalanceMadronaTorch(n, 0) if game == "balance" else HanabiMadrona(n, 0, config=wide_twin.config_of(game))
    ego2 = CleanPPOAgent(env, "ego", DEV, seed=5, update_epochs=1, **kwargs)
    ego2.device_update = True
    partner2 = CleanPPOAgent(env.getDummyEnv(1), "partner", DEV, **kwargs)
    env.add_partner_agent(partner2, player_num=1)
    ego2.policy.params.copy_(before)
    obs = rollout(env, ego2, num_steps, env.reset())
    ego2.step = 0
    ego2._learn()  # the boundary's update without the act behind it
    torch.cuda.synchronize()
    r = ego2.record
    rec = {name: cpu(getattr(r, name)).reshape((-1,) + getattr(r, name).shape[2:]) for name in RECORD_ARRAYS}
    cells = np.flatnonzero(rec["active"])
    assert ego2.last_losses["samples"] == len(cells) > 1
    batch = {"obs": rec["obs"][cells], "state": rec["states"][cells], "mask": rec["action_masks"][cells], "actions": rec["actions"][cells],
             "logprobs": rec["logprobs"][cells], "values": rec["values"][cells], "advantages": rec["advantages"][cells],
             "returns": rec["returns"][cells]}
    cfg = twin.config()
    exact, single = twin.epoch(cpu(before), batch, cfg, torch.float64), twin.epoch(cpu(before), batch, cfg, torch.float32)
    pooled = twin.stat_margins("orthogonal")
    names = {"policy_loss": "pg_loss", "value_loss": "v_loss", "entropy": "entropy", "approx_kl": "approx_kl", "old_approx_kl": "old_approx_kl"}
    ratios = {key: abs(ego2.last_losses[key] - exact["stats"][name]) / max(pooled[name], abs(single["stats"][name] - exact["stats"][name]))
              for key, name in names.items()}
    print(game, "first update, measured / d:", {k: round(v, 2) for k, v in ratios.items()})
    assert all(ratio <= twin.FACTOR for ratio in ratios.values()), ratios
    assert ego2.last_losses["clipfrac"] == np.float32(exact["stats"]["clipfrac"])
    env.close()


def test_refusals_on_a_live_device(hip_lib):
    """A capturing stream, and arrays on another device (the host)."""
    game, weights, size = "balance", "orthogonal", 33
    batch, _, _ = twin.parity(game, weights, size)
    steps, n = twin.record_shape(size)
    dev = Device(batch["params"], twin.make_record(batch, steps, n, batch["seed"]), twin.config())
    before = dev.state()
    with pytest.raises(ValueError, match="advantages"):
        agent_update(dev.policy, dev.optimizer, dev.record, advantages=dev.record.advantages.cpu())
    with pytest.raises(ValueError, match="returns"):
        agent_update(dev.policy, dev.optimizer, dev.record, returns=dev.record.returns.cpu())
    dev.optimizer.workspace(steps * n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    scratch = torch.zeros(4, device=DEV)
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="captured"):
                agent_update(dev.policy, dev.optimizer, dev.record, stats=False)
            scratch.add_(0)
    torch.cuda.synchronize()
    assert dev.optimizer.step == 0
    for a, b, name in zip(dev.state(), before, ("params", "exp_avg", "exp_avg_sq")):
        same_bits(a, b, name)
