"""GPU: ``mrl_cnn_act`` / ``mrl_rollout_cnn`` at ``hidden`` = 512 (the kernel ``mrl_cnn_act_h512``) on the kitchens and team sizes
of tests/kitchen_shape_cases.py (cases: tests/cnn_h512_shape_cases.py), against the float64 torch module.  The kernel had run on
four shapes; here it runs npos 1, 2, 3, 4, 7, 12, 13 and 25 (fc1's per-block range of 32 npos walked over 8 blocks, K2 up to 6400),
F = 31 and 36 with masks over three and four seats, an odd 9 F in the exact-integer test, tile counts with no ragged tail, calls
of one and two samples, its own LDS refusal, a rollout on Simplecooked and one with four seats, and a capturing stream.

Values, log-probs and logits within 8 d, d = the float32 module's distance from the float64 one on the same case; actions equal
off the draw boundaries (tests/test_cnn_h512_shapes_api.py: at most one such row per case).  Each forward case prints its ratios."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import cnn_h512_shape_cases as cases  # noqa: E402
import cnn_twin as twin  # noqa: E402
from madrona_rl_envs_playground_amd import _lib, simulators  # noqa: E402
from madrona_rl_envs_playground_amd.simulators import CnnPolicy, ExecMode, cnn_act  # noqa: E402
from test_gpu_cnn_policy import DEV, cpu, marked_record, put_observations, record_arrays, same_bits  # noqa: E402


def make_sim(key, n, horizon=cases.HORIZON):
    return getattr(simulators, cases.simulator(key))(exec_mode=ExecMode.CUDA, gpu_id=0, num_worlds=n, **cases.layout_params(key, horizon))


def policy_of(key):
    return CnnPolicy.from_module(cases.make_module(key), device=DEV)


def run(sim, policy, players, n, p, **kwargs):
    """one act into row 1 of a marked record over a marked ACTION tensor -> the record's arrays and ACTION"""
    record = marked_record(2, n, p)
    sim.action_tensor().to_torch().fill_(-7)
    cnn_act(sim, policy, players, record, row=1, **kwargs)
    torch.cuda.synchronize()
    return {**record_arrays(record), "action_tensor": cpu(sim.action_tensor())}


@pytest.mark.parametrize("key,n,players", cases.FORWARD, ids=lambda v: v if isinstance(v, str) else ("all" if v is None else str(v)))
def test_forward_pass_and_head(key, n, players, hip_lib):
    """the largest measured / d: DESIGN.md section 30"""
    ref, p = cases.reference(key, n), cases.shape(key)[2]
    policy = policy_of(key)
    sim = make_sim(key, n)
    put_observations(sim, ref["obs"])
    got = run(sim, policy, players, n, p, seed=ref["seed"], step=0)
    again = run(sim, policy, players, n, p, seed=ref["seed"], step=0)
    sim.close()
    seats = [s for s in range(p) if players is None or players >> s & 1]
    rows = np.array([w * p + s for w in range(n) for s in seats])
    pick = lambda name, tail=(): got[name][1][:, seats].reshape((-1,) + tail).astype(np.float64)  # noqa: E731
    actions = got["actions"][1][:, seats].reshape(-1)
    assert ((actions >= 0) & (actions < 6)).all()
    err_value = np.abs(pick("values") - ref["values"][rows]).max()
    err_logp = np.abs(pick("logprobs") - ref["logp"][rows, actions]).max()  # teacher-forced
    err_logits = np.abs(pick("logits", (6,)) - ref["logits"][rows]).max()
    print(f"{key} n={n} players={players}: values {err_value / ref['d_value']:.2f} d (d = {ref['d_value']:.3e}), log-probs "
          f"{err_logp / ref['d_logp']:.2f} d (d = {ref['d_logp']:.3e}), logits {err_logits / ref['d_logits']:.2f} d (d = {ref['d_logits']:.3e})")
    for kind, (own, full) in cases.small_case_unit(key, n).items():  # a condition of the inputs, as in the CPU test, on this host
        assert 8 * own >= full, (key, n, kind, own, full)
    assert err_value <= 8 * ref["d_value"] and err_logp <= 8 * ref["d_logp"] and err_logits <= 8 * ref["d_logits"]
    keep = ~ref["near"][rows]
    assert np.array_equal(actions[keep], ref["actions"][rows][keep])
    same_bits(got["action_tensor"][seats, :, 0].T, got["actions"][1][:, seats], "the ACTION tensor")
    # the seats outside the mask keep their marks, in the record and in ACTION; so does everything outside the act's own cells
    others = [s for s in range(p) if s not in seats]
    assert len(seats) + len(others) == p and (players is None) == (not others)
    assert (got["action_tensor"][others] == -7).all()
    for name in ("actions", "logprobs", "values", "dones", "logits"):
        assert (got[name][0] == -77).all() and (got[name][1][:, others] == -77).all(), name
        assert not (got[name][1][:, seats] == -77).any(), name
    assert (got["rewards"][1] == -77).all() and (got["rewards"][0][:, others] == -77).all() and (got["next_done"] == -77).all()
    assert (got["values"][2] == -77).all()
    for name in got:
        same_bits(again[name], got[name], f"second run: {name}")


@pytest.mark.parametrize("key", cases.INTEGER_KEYS)
def test_operand_and_index_maps_with_exact_integers(key, hip_lib):
    """float32 is exact in any order: a wrong channel-block offset, flatten index, per-block conv-weight reload (the zero behind an
    odd 9 F must stay where the first load put it) or C/D row map changes a bit"""
    (w, h, p, f), (layers, obs) = cases.shape(key), cases.integer_case(key)
    values, logits, bound = twin.integer_forward(layers, twin.rows_of(obs))
    assert bound < 2 ** 24
    policy = CnnPolicy(w, h, f, hidden=512, device=DEV)
    policy.params.copy_(torch.from_numpy(twin.integer_params(layers)))
    sim = make_sim(key, obs.shape[0])
    put_observations(sim, obs)
    got = run(sim, policy, None, obs.shape[0], p, greedy=True)
    sim.close()
    same_bits(got["logits"][1].reshape(-1, 6), logits.astype(np.float32), "logits")
    same_bits(got["values"][1].reshape(-1), values.astype(np.float32), "values")
    assert np.array_equal(got["actions"][1].reshape(-1), logits.argmax(axis=1))


@pytest.mark.parametrize("key", cases.REFUSED_KEYS)
def test_kitchens_past_the_lds_limit_are_refused_at_512(key, hip_lib):
    """the refusal names the 512 image's byte count; the record, ACTION and the ring keep every bit"""
    L, (w, h, p, f), t = _lib.lib(), cases.shape(key), 2
    assert cases.LDS[key] > cases.LDS_LIMIT
    sim = make_sim(key, cases.N)
    assert tuple(sim.observation_world_major_tensor().shape) == (cases.N, p, h, w, f)
    policy = CnnPolicy(w, h, f, hidden=512, device=DEV)
    record = marked_record(t, cases.N, p)
    sim.action_tensor().to_torch().fill_(-7)
    ws = torch.empty(int(L.mrl_cnn_workspace_bytes(cases.N, p)), dtype=torch.uint8, device=DEV)
    ring = torch.zeros((t + 1, cases.N, p, h, w, f), dtype=torch.int8, device=DEV)
    desc, rec, every_seat = policy.desc(), record.struct, (1 << p) - 1
    assert desc.hidden == 512
    needs = f"a {w} x {h} kitchen with {f} channels needs an LDS image of {cases.LDS[key]} bytes per workgroup, the limit is {cases.LDS_LIMIT}"
    rc = L.mrl_cnn_act(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), 0, 1, 0, 0, ws.data_ptr(), ws.numel(), None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_cnn_act: {needs}"
    rc = L.mrl_rollout_cnn(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), ring.data_ptr(), 1, 0, None)
    assert rc == _lib.MRL_ERR_INVALID and L.mrl_last_error().decode() == f"mrl_rollout_cnn: {needs}"
    with pytest.raises(_lib.MrlError) as refused:
        cnn_act(sim, policy, None, record, row=0)
    assert str(refused.value) == f"mrl_cnn_act: {needs}"
    torch.cuda.synchronize()
    for name, value in record_arrays(record).items():
        assert (value == -77).all(), name
    assert (cpu(sim.action_tensor()) == -7).all() and not cpu(ring).any()
    sim.close()


@pytest.mark.parametrize("key", ["k8x5p4", "multiplayer_schelling/1p"])
def test_the_two_images_nearest_the_limit_are_accepted(key, hip_lib):
    L, (w, h, p, f), n, t = _lib.lib(), cases.shape(key), 3, 1
    assert cases.LDS_LIMIT - 4096 < cases.LDS[key] <= cases.LDS_LIMIT
    sim, policy, record = make_sim(key, n), policy_of(key), marked_record(t, n, p)
    ws = torch.empty(int(L.mrl_cnn_workspace_bytes(n, p)), dtype=torch.uint8, device=DEV)
    ring = torch.zeros((t + 1, n, p, h, w, f), dtype=torch.int8, device=DEV)
    desc, rec, every_seat = policy.desc(), record.struct, (1 << p) - 1
    assert L.mrl_cnn_act(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), 0, 1, 0, 0, ws.data_ptr(), ws.numel(), None) == _lib.MRL_OK
    torch.cuda.synchronize()
    first = cpu(record.values)[0]
    assert (first != -77).all()
    assert L.mrl_rollout_cnn(sim._handle, every_seat, ctypes.byref(desc), ctypes.byref(rec), ring.data_ptr(), 1, 0, None) == _lib.MRL_OK
    torch.cuda.synchronize()
    same_bits(cpu(record.values)[0], first, "the rollout's first values against the act's on the same observations")
    assert (cpu(record.values)[1] != -77).all() and cpu(ring)[1].any()
    sim.close()


@pytest.mark.parametrize("key,n,t,horizon", cases.ROLLOUTS)
def test_rollout_equals_hand_issued_acts_and_steps(key, n, t, horizon, hip_lib):
    """Simplecooked (F = 15) and four seats: the whole record and the observation ring bit for bit, episodes ending inside"""
    w, h, p, f = cases.shape(key)
    policy = policy_of(key)
    sim = make_sim(key, n, horizon)
    record = marked_record(t, n, p)
    ring = torch.zeros((t + 1, n, p, h, w, f), dtype=torch.int8, device=DEV)
    sim.rollout_cnn(policy, record, ring, seed=21, first_step=100)
    torch.cuda.synchronize()
    got, got_ring = record_arrays(record), cpu(ring)
    sim.close()
    assert got["dones"].sum() > 0 and not got["dones"].all()
    sim = make_sim(key, n, horizon)
    by_hand = marked_record(t, n, p)
    slots = torch.zeros_like(ring)
    slots[0].copy_(sim.observation_world_major_tensor().to_torch())
    for k in range(t):
        cnn_act(sim, policy, None, by_hand, row=k, seed=21, step=100 + k)
        sim.set_observation_output(slots[k + 1])
        sim.step()
    cnn_act(sim, policy, None, by_hand, row=t, value_only=True)
    sim.set_observation_output(None)
    torch.cuda.synchronize()
    for name, value in record_arrays(by_hand).items():
        assert not (value == -77).any(), name  # every cell of every row was written, every seat's column
        same_bits(got[name], value, f"rollout against hand-issued calls: {name}")
    same_bits(got_ring, cpu(slots), "the observation ring")
    assert not np.array_equal(got_ring[0], got_ring[t])
    # the closing value is a full act's on the same slot
    put_observations(sim, got_ring[t])
    greedy = run(sim, policy, None, n, p, seed=21, step=100 + t, greedy=True)
    same_bits(greedy["values"][1], got["values"][t], "the closing value against a full act's on the same slot")
    assert np.array_equal(greedy["actions"][1].reshape(-1), greedy["logits"][1].reshape(-1, 6).argmax(axis=1))
    sim.close()


def test_a_capturing_stream_is_refused_and_nothing_is_recorded(hip_lib):
    """``mrl_cnn_act`` carries the row and the step number in kernel arguments and refuses a capturing stream at every width (the
    plain act's test holds the same at 64): at 512 the refusal enqueues nothing and leaves the capture whole, and the same act
    run eagerly on the side stream has the bits of the default stream's, over two observation sets"""
    key, n, seed = "cramped_room", 33, 5
    p, policy = cases.shape(key)[2], policy_of(key)
    sim = make_sim(key, n)
    side, eager, on_side = torch.cuda.Stream(), [], []
    for obs_seed in (77, 78):
        put_observations(sim, twin.synthetic_observations(key, n, obs_seed))
        eager.append(run(sim, policy, None, n, p, seed=seed, step=0))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side.append(run(sim, policy, None, n, p, seed=seed, step=0))
        for name in eager[-1]:
            same_bits(on_side[-1][name], eager[-1][name], f"the side stream, observations {obs_seed}: {name}")
    assert not np.array_equal(eager[0]["values"], eager[1]["values"])
    record = marked_record(2, n, p)
    sim.action_tensor().to_torch().fill_(-7)
    graph, scratch = torch.cuda.CUDAGraph(), torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.MrlError, match="mrl_cnn_act: the row and the step number travel in kernel arguments, a captured call"):
                cnn_act(sim, policy, None, record, row=1, seed=seed, step=0)
            scratch.add_(0)  # (a capture must record something)
    torch.cuda.synchronize()
    for name, value in record_arrays(record).items():
        assert (value == -77).all(), name
    assert (cpu(sim.action_tensor()) == -7).all()
    after = run(sim, policy, None, n, p, seed=seed, step=0)  # and the simulator still acts, with the same bits
    for name in after:
        same_bits(after[name], eager[1][name], f"behind the refused capture: {name}")
    sim.close()
