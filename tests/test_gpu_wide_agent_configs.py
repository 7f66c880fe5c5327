"""GPU: ``mrl_agent_act`` / ``mrl_agent_credit`` / ``mrl_gae_active`` on every Hanabi configuration of tests/hanabi_configs.py.

What the named games of tests/test_gpu_wide_agent.py never gave the act kernels: a simulator in code variant 0 (ranks != 5),
five-rank games other than the two named ones, 15, 17, 18 and 19 actions laid over the simulator's 20-wide mask row,
observation and state widths that are odd or no multiple of four through the one-byte record copies, and first layers whose K
is the configuration's own width (last k-chunks of 2, 3, 5, 32 and 62).

Forward cases (``twin.CONFIG_CASES`` x WEIGHTS, 65 worlds: three 32-row tiles with a last tile of one row): everything
test_gpu_wide_agent.py asserts of a case, through the same check functions, with d = ``twin.config_margins`` -- one
configuration's own, pooled over three input sets.  The closed loop (``twin.WALK_SEEDS``): the device collects both seats on
the live simulator while the oracle is fed the device's actions and tests/wide_twin.py walks the same game on the CPU;
tests/test_wide_agent_api.py asserts that no active row of that walk is near a boundary, that every action is chosen, that
a seat-step has no active world and that episodes end.  Bound 8 d everywhere (DESIGN.md sections 13 and 14); each test
prints its ratios."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hanabi_configs  # noqa: E402
import wide_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import WidePolicy, agent_act, agent_credit, gae_active  # noqa: E402
from test_gpu_hanabi import compare  # noqa: E402
from test_gpu_wide_agent import (DEV, WEIGHTS, check_all_rows_and_greedy, check_forward_pass_and_head, check_operand_maps,  # noqa: E402
                                 check_values, cpu, forward_case, make_sim, new_record, record_arrays_no_logits, same_bits)


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("game,n", twin.CONFIG_CASES)
def test_forward_pass_head_and_record(game, n, weights, hip_lib):
    """Every assertion of test_forward_pass_and_head, test_values_within_8_d_of_the_twin and test_all_rows_and_greedy."""
    d, s, a = twin.dims(game)
    d_value, d_logp = twin.config_margins(game, weights)
    ratio_logp = check_forward_pass_and_head(game, n, weights, d_logp)
    ratio_value = check_values(game, n, weights, d_value)
    ratio_all = check_all_rows_and_greedy(game, n, weights, d_logp)
    got = forward_case(game, n, weights)["runs"]["default"]
    # the widths: D and S of the configuration, A of the simulator's 20 mask columns; logits beyond A stay 0
    assert got["obs"].shape == (2, n, d) and got["states"].shape == (2, n, s) and got["action_masks"].shape == (2, n, a)
    assert got["logits"][:, :a].any() and not got["logits"][:, a:].any()
    print(f"RATIO forward {game} {weights}: values {ratio_value:.2f} d, log-probs {max(ratio_logp, ratio_all):.2f} d")


@pytest.mark.parametrize("game,n", twin.CONFIG_CASES)
def test_operand_maps_with_exact_integers(game, n, hip_lib):
    """Integer weights, ALL_ROWS: logits [:, :A] and values bit for bit, with a first layer as wide as the configuration's rows.
    tests/test_wide_agent_api.py bounds every sum of absolute terms below 2^24."""
    check_operand_maps(game, n, 1)


def flags(x):
    return (np.asarray(x) != 0).astype(np.uint8)


@pytest.mark.parametrize("cid", list(twin.WALK_SEEDS))
def test_closed_loop_against_the_oracle_and_the_twin(cid, hip_lib, oracle_lib):
    """Both seats collect ``twin.WALK_STEPS`` steps on the live simulator, ``mrl_agent_credit`` after every step.  After every step
    the simulator's tensors equal the oracle's, fed the device's actions, and those actions equal the CPU walk's in every row
    (0 where a seat is not the one to act).  Log-probs of the recorded actions and values within 8 d of the twin, d = torch
    float32's distance from the twin on those same rows: the seat's active rows of the whole walk.  The record's bookkeeping
    equals ``twin.book`` / ``twin.credit`` bit for bit; then a VALUE_ONLY act and ``mrl_gae_active``, against ``twin.gae_active`` fed
    the device's own values."""
    game, cfg, n, num_steps, seed = "hanabi_" + cid, hanabi_configs.BY_ID[cid], twin.WALK_N, twin.WALK_STEPS, twin.WALK_SEEDS[cid]
    d, s, a = twin.dims(game)
    walk = twin.walked(cid)
    agents = [twin.make_agent(game, w, seed=21 + p) for p, w in enumerate(WEIGHTS)]
    policies = [WidePolicy.from_module(agent, device=DEV) for agent in agents]
    sim, orc = make_sim(game, n), oracle_lib.HanabiOracle(cfg, n)
    records = [new_record(sim, game, num_steps) for _ in range(2)]
    numpy_recs, returns = [twin.new_record(num_steps, n) for _ in range(2)], [[], []]
    mask = sim.action_mask_tensor().to_torch()
    compare(sim, orc, "initial", cfg)
    finished = 0
    for t, step in enumerate(walk):
        sim.action_tensor().to_torch().fill_(-7)
        for p in range(2):
            agent_act(sim, p, policies[p], records[p], row=t, seed=seed, step=t)
        actions = cpu(sim.action_tensor())[:, :, 0]
        assert np.array_equal(actions, step["actions"]), f"step {t}: the device's actions are not the walk's"
        orc.step(actions)
        sim.step()
        compare(sim, orc, f"step {t}", cfg)
        assert not mask[..., a:].any(), f"step {t}: a legal move beyond the game's {a}"
        rewards, dones = sim.reward_tensor().to_torch(), sim.done_tensor().to_torch()
        for p in range(2):
            agent_credit(records[p], rewards[p], dones)
            twin.book(numpy_recs[p], t, step["seats"][p]["active"])
            returns[p].append(twin.credit(numpy_recs[p], orc.reward[p], orc.done))
        finished += int(orc.done.sum())
    torch.cuda.synchronize()
    assert finished > 0 and finished == sum(int(step["after"]["done"].sum()) for step in walk)
    ratios = []
    for p in range(2):
        rec = dict(record_arrays_no_logits(records[p]), running_rewards=cpu(records[p].running_rewards), totals=cpu(records[p].totals))
        err_value = err_logp = d_value = d_logp = 0.0
        for t, step in enumerate(walk):
            before, seat = step["before"], step["seats"][p]
            active, want = seat["active"], seat["twin"]
            same_bits(rec["obs"][t], before["obs"][p][:, :d].view(np.int8), f"seat {p}: obs row {t}")
            same_bits(rec["states"][t], before["state"][p][:, :s].view(np.int8), f"seat {p}: states row {t}")
            same_bits(rec["action_masks"][t], flags(before["mask"][p][:, :a]), f"seat {p}: masks row {t}")
            same_bits(rec["actions"][t], step["actions"][p], f"seat {p}: actions row {t}")
            for name in ("logprobs", "values"):
                assert (rec[name][t][~active] == 0).all(), f"seat {p}: {name} of the inactive rows of row {t}"
            if not active.any():
                continue
            chosen = want["logp"][np.arange(active.sum()), want["actions"]]
            err_logp = max(err_logp, np.abs(rec["logprobs"][t][active].astype(np.float64) - chosen).max())
            err_value = max(err_value, np.abs(rec["values"][t][active] - want["values"]).max())
            d_value, d_logp = max(d_value, seat["d"][0]), max(d_logp, seat["d"][1])
        print(f"RATIO loop {game} seat {p} ({WEIGHTS[p]}): values {err_value / d_value:.2f} d (d = {d_value:.3e}), log-probs "
              f"{err_logp / d_logp:.2f} d (d = {d_logp:.3e}); {finished} episodes ended")
        ratios.append((err_value / d_value, err_logp / d_logp))
        assert err_value <= 8 * d_value
        assert err_logp <= 8 * d_logp
        for name in ("active", "dones", "rewards", "last_active", "new_game", "next_done", "running_rewards"):
            same_bits(rec[name], numpy_recs[p][name], f"seat {p}: {name}")
        assert rec["dones"].any() and rec["rewards"].any() and rec["new_game"].any()  # (the end of an episode reached the record)
        assert rec["totals"][:, 0].sum() == finished == numpy_recs[p]["totals"][:, 0].sum()
        assert np.array_equal(rec["totals"][:, 2:], numpy_recs[p]["totals"][:, 2:])
        every = np.concatenate(returns[p])
        assert len(every) == finished
        assert abs(rec["totals"][0, 1] - numpy_recs[p]["totals"][0, 1]) <= 8 * twin.sum_margin(every)
        # the bootstrap value and the advantage pass on this record: alternating seats, episodes that end every few moves
        agent_act(sim, p, policies[p], records[p], row=num_steps, seed=seed, step=num_steps, value_only=True)
        torch.cuda.synchronize()
        now_active = orc.active[p] != 0
        next_value, next_active = cpu(records[p].next_value), cpu(records[p].next_active)
        same_bits(next_active, flags(now_active), f"seat {p}: next_active")
        assert (next_value[~now_active] == 0).all()
        if now_active.any():
            inputs = {"obs": orc.obs[p][now_active, :d], "state": orc.state[p][now_active, :s], "mask": orc.mask[p][now_active, :a]}
            d_boot = twin.margins(agents[p], inputs)[0]
            err_boot = np.abs(next_value[now_active] - twin.forward(twin.flat(agents[p]), inputs["obs"], inputs["state"], a)[0]).max()
            print(f"RATIO loop {game} seat {p}: bootstrap values {err_boot / d_boot:.2f} d (d = {d_boot:.3e})")
            assert err_boot <= 8 * d_boot
        want = twin.gae_active(rec["rewards"], rec["values"], rec["dones"], rec["active"], rec["next_done"], next_value, next_active, 0.99, 0.95)
        adv, ret = gae_active(records[p], 0.99, 0.95)
        torch.cuda.synchronize()
        same_bits(cpu(adv), want[0], f"seat {p}: advantages")
        same_bits(cpu(ret), want[1], f"seat {p}: returns")
        same_bits(cpu(records[p].active), want[2].astype(np.uint8), f"seat {p}: active after the advantage pass")
        assert want[0].any()
    sim.close()
    orc.close()
