// Policy rollouts on the device for Cartpole, Acrobot and the balance beam's single-agent trainer (C ABI: mrl_rollout_policy,
// mrl_gae in include/mrl_envs.h).  The kernels live in policy_rollout.hip; capi_ppo.hip drives them around the simulator's
// ordinary step.
#pragma once

#include "common.hpp"

namespace mrl {

constexpr uint32_t kPolicyHidden = 64;  // the only width the kernel is written for (scripts/cartpole_train_torch.py:105-121)

// parameters of one three-layer net Linear(d, h), Linear(h, h), Linear(h, out), weights row-major, each followed by its bias
constexpr uint64_t mlp_net_params(uint64_t d, uint64_t h, uint64_t out) { return d * h + h + h * h + h + h * out + out; }

// What one mrl_policy_act launch reads and writes: the simulator's tensors as they stand and the rows of the rollout
// buffer that belong to this call (row k of the (T, ...) arrays, or the next_* arrays for the closing call).  The beam's
// fields come last, so that the other instances find theirs where they always were.
struct PolicyActArgs {
    const float *params;       // critic net, then actor net (mrl_mlp_policy::params_dev)
    const float *state;        // STATE, (N, 4); unused on the beam
    const int32_t *reset;      // RESET, (N, 1): the previous step's flag; the beam's DONE, (N)
    const float *reward;       // REWARD, (N, 1): the previous step's reward; the beam's REWARD[0], the ego's
    int32_t *action_tensor;    // ACTION, (N, 1): what the step behind this launch reads; the beam's ACTION[0]
    float *obs_row;            // (N, D)
    float *done_row;           // (N)
    float *value_row;          // (N)
    float *reward_row;         // (N) row k - 1, nullptr for k = 0
    int32_t *action_row;       // (N), nullptr for the closing call, which draws nothing
    float *logprob_row;        // (N), with action_row
    uint64_t seed;
    uint32_t step;             // first_step + k of the sampling hash
    uint32_t num_worlds;
    uint32_t flags;            // MRL_POLICY_GREEDY
    const int32_t *obs_i32;    // the beam only: OBSERVATION[0], (N, 7) int32
    int32_t *partner_action;   // the beam only: ACTION[1], (N, 1), written by every launch that draws
    uint32_t member_worlds;    // a bank only (policy.num_members != 0): W = N / num_members, the worlds of one member
};

// one launch; the policy's shape has been validated (obs_dim / num_actions / obs_mode one of the four supported).  With
// policy.num_members = K != 0 the launch is (ceil(W / 64), nets, K): member z acts for worlds [z W, (z + 1) W) under the
// parameters z P floats behind args.params.
void launch_policy_act(const mrl_mlp_policy &policy, const PolicyActArgs &args, hipStream_t stream);

void launch_gae(const float *rewards, const float *values, const float *dones, const float *next_value, const float *next_done,
                uint32_t num_steps, uint32_t num_worlds, float gamma, float lambda, float *advantages, float *returns,
                hipStream_t stream);

}  // namespace mrl
