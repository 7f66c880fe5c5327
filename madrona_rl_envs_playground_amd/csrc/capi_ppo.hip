// The C API of the MLP learner (include/mrl_envs.h): the policy rollout of Cartpole, Acrobot and the balance beam, GAE and the PPO update, and the
// tail every update's refusals share (update_refusal, capi_internal.hpp).
#include "capi_internal.hpp"
#include "policy_rollout.hpp"
#include "ppo_update.hpp"

namespace mrl {

// what mrl_ppo_update and mrl_mappo_update (`what`) refuse alike, after their own checks: a workspace smaller than `sizer` asks
// for, arrays or a workspace off their boundaries (`arrays_rule` says which arrays, `arrays_off` whether one of them is), and a
// capturing stream
int update_refusal(const char *what, const char *sizer, uint64_t workspace_bytes, uint64_t need_bytes, const void *workspace_dev,
                   bool arrays_off, const char *arrays_rule, void *hip_stream)
{
    if (workspace_bytes < need_bytes) {
        mrl::set_error("%s: workspace of %llu bytes, %s asks for %llu", what, (unsigned long long)workspace_bytes, sizer,
                       (unsigned long long)need_bytes);
        return MRL_ERR_INVALID;
    }
    if (arrays_off || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) {
        mrl::set_error("%s: %s and the workspace on a 16-byte one", what, arrays_rule);
        return MRL_ERR_INVALID;
    }
    if (mrl::capturing(hip_stream)) {
        mrl::set_error("%s: the Adam step number travels in kernel arguments, so the call cannot be captured in a HIP graph: a replay "
                       "would repeat the same step's bias correction", what);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

}  // namespace mrl

using mrl::guarded;
using mrl::update_refusal;

extern "C" {

uint64_t mrl_mlp_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions)
{
    return mrl::mlp_net_params(obs_dim, hidden, 1) + mrl::mlp_net_params(obs_dim, hidden, num_actions);
}

int mrl_rollout_policy(mrl_sim *sim, const mrl_mlp_policy *policy, const mrl_rollout_buffers *buffers, uint64_t seed,
                       uint32_t first_step, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_rollout_policy")) return rc;
    const bool beam = sim->game == MRL_GAME_BALANCE;
    if (sim->game != MRL_GAME_CARTPOLE && sim->game != MRL_GAME_ACROBOT && !beam) {
        mrl::set_error("mrl_rollout_policy: game %d has no policy rollout (Cartpole, Acrobot and the balance beam do)", sim->game);
        return MRL_ERR_INVALID;
    }
    if (sim->exchange.mine) {
        mrl::set_error("mrl_rollout_policy: this simulator is a rank of an exchanged batch (mrl_exchange_create); its step needs the other ranks");
        return MRL_ERR_INVALID;
    }
    if (beam && mrl::capturing(hip_stream)) {  // (after mrl_prepare_graph_capture mrl_step would let the capture pass)
        mrl::set_error("mrl_rollout_policy: the row index travels in kernel arguments, so a rollout cannot be captured in a HIP graph");
        return MRL_ERR_INVALID;
    }
    if (!policy || !buffers || !policy->params_dev) {
        mrl::set_error("mrl_rollout_policy: null policy, parameter array or buffer description");
        return MRL_ERR_INVALID;
    }
    if (beam && (policy->hidden != mrl::kPolicyHidden || policy->obs_dim != 7 || policy->num_actions != 4 ||
                 policy->obs_mode != MRL_OBS_BALANCE)) {
        mrl::set_error("mrl_rollout_policy: the balance beam takes hidden = 64, obs_dim = 7, num_actions = 4, MRL_OBS_BALANCE; (4, RAW) and "
                       "(6, ACROBOT_GYM) are the shapes of Cartpole and Acrobot; got hidden %u, num_actions %u, obs_dim %u, obs_mode %u",
                       policy->hidden, policy->num_actions, policy->obs_dim, policy->obs_mode);
        return MRL_ERR_INVALID;
    }
    const uint32_t actions = sim->game == MRL_GAME_CARTPOLE ? 2u : 3u;
    const bool raw = policy->obs_dim == 4 && policy->obs_mode == MRL_OBS_RAW;
    const bool gym = policy->obs_dim == 6 && policy->obs_mode == MRL_OBS_ACROBOT_GYM && sim->game == MRL_GAME_ACROBOT;
    if (!beam && (policy->hidden != mrl::kPolicyHidden || policy->num_actions != actions || !(raw || gym))) {
        mrl::set_error("mrl_rollout_policy: need hidden = 64, num_actions = %u and (obs_dim, obs_mode) = (4, MRL_OBS_RAW)%s for game %d; got "
                       "hidden %u, num_actions %u, obs_dim %u, obs_mode %u", actions,
                       sim->game == MRL_GAME_ACROBOT ? " or (6, MRL_OBS_ACROBOT_GYM)" : "", sim->game, policy->hidden,
                       policy->num_actions, policy->obs_dim, policy->obs_mode);
        return MRL_ERR_INVALID;
    }
    const mrl_rollout_buffers &b = *buffers;
    const uint32_t T = b.num_steps;
    if (!b.next_obs || !b.next_value || !b.next_done ||
        (T && (!b.obs || !b.actions || !b.logprobs || !b.values || !b.rewards || !b.dones))) {
        mrl::set_error("mrl_rollout_policy: null rollout buffer");
        return MRL_ERR_INVALID;
    }
    // the observation rows are stored 16 / 8 bytes at a time, the beam's seven floats one by one
    const uintptr_t row_align = policy->obs_dim == 4 ? 15u : policy->obs_dim == 6 ? 7u : 3u;
    if ((reinterpret_cast<uintptr_t>(b.obs) | reinterpret_cast<uintptr_t>(b.next_obs)) & row_align) {
        mrl::set_error("mrl_rollout_policy: obs and next_obs must start on a %u-byte boundary", (unsigned)row_align + 1u);
        return MRL_ERR_INVALID;
    }
    // a bank (num_members != 0): equal shares of the batch, the member in blockIdx.z
    const uint32_t K = policy->num_members;
    if (K && (K > 65535u || K > sim->num_worlds || sim->num_worlds % K)) {
        mrl::set_error("mrl_rollout_policy: a bank of %u members on %u worlds; every member owns the same number of worlds, at least "
                       "one, so num_worlds must be a multiple of num_members, and num_members at most 65535", K, sim->num_worlds);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        hipStream_t stream = (hipStream_t)hip_stream;
        mrl_tensor_desc state{}, reset{}, reward{}, action{};
        const size_t N = sim->num_worlds, D = policy->obs_dim;
        mrl::PolicyActArgs args{};
        if (beam) {
            // seat 0 is the ego: the first N rows of OBSERVATION (2, N, 7), REWARD (2, N) and ACTION (2, N, 1); DONE is (N)
            if (!sim->tensor(MRL_BALANCE_OBSERVATION, &state) || !sim->tensor(MRL_BALANCE_DONE, &reset) ||
                !sim->tensor(MRL_BALANCE_REWARD, &reward) || !sim->tensor(MRL_BALANCE_ACTION, &action))
                throw std::runtime_error("mrl_rollout_policy: the simulator does not export OBSERVATION / DONE / REWARD / ACTION");
            if (state.dtype != MRL_INT32 || state.shape[0] != 2 || state.shape[2] != 7 || reward.dtype != MRL_FLOAT32 ||
                action.dtype != MRL_INT32 || reset.dtype != MRL_INT32)
                throw std::runtime_error("mrl_rollout_policy: unexpected tensor layout (OBSERVATION int32 (2, N, 7), REWARD float32, "
                                         "ACTION and DONE int32)");
            args.obs_i32 = static_cast<const int32_t *>(state.data);
            args.partner_action = static_cast<int32_t *>(action.data) + N;
        } else {
            // (the slot numbers are the same for both games: MRL_CARTPOLE_* == MRL_ACROBOT_*)
            if (!sim->tensor(MRL_CARTPOLE_STATE, &state) || !sim->tensor(MRL_CARTPOLE_RESET, &reset) ||
                !sim->tensor(MRL_CARTPOLE_REWARD, &reward) || !sim->tensor(MRL_CARTPOLE_ACTION, &action))
                throw std::runtime_error("mrl_rollout_policy: the simulator does not export STATE / RESET / REWARD / ACTION");
            args.state = static_cast<const float *>(state.data);
        }
        args.params = policy->params_dev;
        args.reset = static_cast<const int32_t *>(reset.data);
        args.reward = static_cast<const float *>(reward.data);
        args.action_tensor = static_cast<int32_t *>(action.data);
        args.seed = seed;
        args.num_worlds = sim->num_worlds;
        args.member_worlds = K ? sim->num_worlds / K : 0;
        args.flags = policy->flags;
        for (uint32_t k = 0; k <= T; k++) {
            const bool closing = k == T;
            args.obs_row = closing ? b.next_obs : b.obs + k * N * D;
            args.done_row = closing ? b.next_done : b.dones + k * N;
            args.value_row = closing ? b.next_value : b.values + k * N;
            args.reward_row = k ? b.rewards + (k - 1) * N : nullptr;
            args.action_row = closing ? nullptr : b.actions + k * N;
            args.logprob_row = closing ? nullptr : b.logprobs + k * N;
            args.step = first_step + k;
            mrl::launch_policy_act(*policy, args, stream);
            if (closing) break;
            sim->step(nullptr, stream);
            mrl::completed_step(sim, stream);
        }
    });
}

int mrl_gae(const float *rewards, const float *values, const float *dones, const float *next_value, const float *next_done,
            uint32_t num_steps, uint32_t num_worlds, float gamma, float lambda, float *advantages, float *returns, int gpu_id,
            void *hip_stream)
{
    if (!next_value || !next_done || (num_steps && (!rewards || !values || !dones || !advantages || !returns))) {
        mrl::set_error("mrl_gae: null array");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_gae(rewards, values, dones, next_value, next_done, num_steps, num_worlds, gamma, lambda, advantages, returns,
                        (hipStream_t)hip_stream);
    });
}

static bool ppo_shape_ok(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions)
{
    return hidden == mrl::kPolicyHidden && ((obs_dim == 4 && (num_actions == 2 || num_actions == 3)) || (obs_dim == 6 && num_actions == 3) ||
                                            (obs_dim == 7 && num_actions == 4));
}

// The shapes a refusal lists.  A call that has nothing of the balance beam's shape is told the float-state games' three, in the
// words these refusals have always had; one with obs_dim 7 or num_actions 4, which could not be mistaken before the beam had a
// shape here, is told all four.
static const char *ppo_shapes(uint32_t obs_dim, uint32_t num_actions)
{
    return obs_dim == 7 || num_actions == 4 ? "(4, 2), (4, 3), (6, 3), (7, 4)" : "(4, 2), (4, 3), (6, 3)";
}

int mrl_ppo_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions, uint32_t minibatch_size,
                            uint32_t num_minibatches, uint64_t *out)
{
    if (!out || !ppo_shape_ok(obs_dim, hidden, num_actions) || minibatch_size == 0) {
        mrl::set_error("mrl_ppo_workspace_bytes: need an output pointer, hidden = 64, (obs_dim, num_actions) one of %s and "
                       "minibatch_size > 0; got hidden %u, obs_dim %u, num_actions %u, minibatch_size %u", ppo_shapes(obs_dim, num_actions),
                       hidden, obs_dim, num_actions, minibatch_size);
        return MRL_ERR_INVALID;
    }
    const uint64_t params = mrl_mlp_policy_num_params(obs_dim, hidden, num_actions);
    *out = mrl::ppo_workspace(params, minibatch_size, num_minibatches).total * sizeof(float);
    return MRL_OK;
}

int mrl_ppo_update(const mrl_mlp_policy *shape, const mrl_ppo_optimizer *opt, const mrl_ppo_batch *batch,
                   const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config *cfg,
                   void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null, int gpu_id,
                   void *hip_stream)
{
    if (!shape || !opt || !batch || !indices_dev || !cfg || !workspace_dev) {
        mrl::set_error("mrl_ppo_update: null shape, optimizer, batch, index array, configuration or workspace");
        return MRL_ERR_INVALID;
    }
    if (!opt->params_dev || !opt->exp_avg || !opt->exp_avg_sq || !batch->obs || !batch->actions || !batch->logprobs ||
        !batch->advantages || !batch->returns || !batch->values) {
        mrl::set_error("mrl_ppo_update: null parameter, moment or batch array");
        return MRL_ERR_INVALID;
    }
    if (!ppo_shape_ok(shape->obs_dim, shape->hidden, shape->num_actions)) {
        mrl::set_error("mrl_ppo_update: need hidden = 64 and (obs_dim, num_actions) one of %s; got hidden %u, obs_dim %u, num_actions %u",
                       ppo_shapes(shape->obs_dim, shape->num_actions), shape->hidden, shape->obs_dim, shape->num_actions);
        return MRL_ERR_INVALID;
    }
    if (minibatch_size == 0 || batch->size == 0 || (minibatch_size < 2 && (cfg->flags & MRL_PPO_NORM_ADV))) {
        mrl::set_error("mrl_ppo_update: need minibatch_size > 0 (> 1 with MRL_PPO_NORM_ADV: the unbiased std of one sample does not "
                       "exist) and a batch of at least one sample; got minibatch_size %u, batch size %u", minibatch_size, batch->size);
        return MRL_ERR_INVALID;
    }
    const uint64_t params = mrl_mlp_policy_num_params(shape->obs_dim, shape->hidden, shape->num_actions);
    // a bank update (opt->num_members != 0) takes one slice per member
    const uint64_t need_bytes = mrl::ppo_workspace(params, minibatch_size, num_minibatches).total * sizeof(float) *
                                (opt->num_members ? opt->num_members : 1u);
    // the observation rows are loaded 16 / 8 bytes at a time, the beam's seven floats one by one
    const uint32_t D = shape->obs_dim;
    const char *rule = D == 4 ? "obs must start on a 16-byte boundary"
                     : D == 6 ? "obs must start on a 8-byte boundary"
                              : "obs must start on a 4-byte boundary for (7, 4) (16 bytes for (4, 2) and (4, 3), 8 for (6, 3))";
    if (int rc = update_refusal("mrl_ppo_update", "mrl_ppo_workspace_bytes", workspace_bytes, need_bytes, workspace_dev,
                                reinterpret_cast<uintptr_t>(batch->obs) & (D == 4 ? 15u : D == 6 ? 7u : 3u), rule, hip_stream))
        return rc;
    if (opt->num_members > 65535u) {
        mrl::set_error("mrl_ppo_update: %u members; the member travels in the launch grid's third dimension, so at most 65535",
                       opt->num_members);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_ppo_update(*shape, *opt, *batch, indices_dev, num_minibatches, minibatch_size, *cfg,
                               static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream);
    });
}

}  // extern "C"
