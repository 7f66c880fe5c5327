// mrl_policy_act and mrl_gae: the collection phase of PPO for Cartpole and Acrobot without the host in the loop
// (include/mrl_envs.h, mrl_rollout_policy).
//
// The reference's trainer runs, per step, two three-layer tanh MLPs, a Categorical sample, a log_prob and six buffer row
// copies in torch (scripts/cartpole_train_torch.py:204-218, Agent :105-131).  Here that is ONE launch in front of the
// simulator's ordinary step: a lane per world, the weights read in place from the flat parameter array -- their
// addresses are the same in every lane, so they arrive through scalar loads and sit in SGPRs --, the 64 activations of
// the first hidden layer in VGPRs, the second hidden layer folded into the output layer one unit at a time.  Critic and
// actor are independent, so they run in different workgroups (blockIdx.y): at 1024 worlds that halves the dependent
// chain, at large batches it costs one more 16-byte read of the state per world.
//
// The balance beam (MRL_OBS_BALANCE, D = 7, A = 4) is the same launch on seat 0's int32 observation row; its actor workgroups
// also write the other seat's uniformly random move, so the step behind the launch finds both seats' actions (DESIGN.md
// section 25).
//
// Arithmetic: every dot product is bias first, then fmaf over the inputs in ascending order (the Makefile compiles with
// -ffp-contract=off, so nothing else is fused); tanhf / expf / logf / sinf / cosf are the accurate library versions.
#include "policy_rollout.hpp"
#include "random_policy.hpp"

namespace mrl {

constexpr int kH = (int)kPolicyHidden;
constexpr int kActThreads = 64;  // one wavefront per workgroup: small batches spread over as many CUs as they have waves

// p: one net (weight, bias) x 3.  out[o] = the net's o-th output for input x.
template <int D, int OUT>
__device__ __forceinline__ void mlp_forward(const float *__restrict__ p, const float (&x)[D], float (&out)[OUT])
{
    const float *__restrict__ w1 = p, *__restrict__ b1 = w1 + kH * D;
    const float *__restrict__ w2 = b1 + kH, *__restrict__ b2 = w2 + kH * kH;
    const float *__restrict__ w3 = b2 + kH, *__restrict__ b3 = w3 + OUT * kH;
    float h1[kH];
#pragma unroll
    for (int j = 0; j < kH; j++) {
        float acc = b1[j];
#pragma unroll
        for (int i = 0; i < D; i++) acc = fmaf(w1[j * D + i], x[i], acc);
        h1[j] = tanhf(acc);
    }
#pragma unroll
    for (int o = 0; o < OUT; o++) out[o] = b3[o];
    // hidden unit j of the second layer is complete before the output layer needs it: no second activation array
#pragma unroll 1
    for (int j = 0; j < kH; j++) {
        float acc = b2[j];
#pragma unroll
        for (int i = 0; i < kH; i++) acc = fmaf(w2[j * kH + i], h1[i], acc);
        const float h2 = tanhf(acc);
#pragma unroll
        for (int o = 0; o < OUT; o++) out[o] = fmaf(w3[o * kH + j], h2, out[o]);
    }
}

// MEMBERS: a bank of K policies on one batch of N = K W worlds.  Member blockIdx.z owns worlds
// [z W, (z + 1) W) and its parameters lie z P floats behind a.params: an address that is still the same in every lane, so the
// weights still arrive through scalar loads.  Everything behind these four lines is the plain body on the world's number in the
// batch of N.  The MEMBERS = false instance, which every plain rollout launches, reads neither blockIdx.z nor member_worlds.
template <int D, int A, int MODE, bool MEMBERS>
__global__ void __launch_bounds__(kActThreads) mrl_policy_act(PolicyActArgs a)
{
    const uint32_t local = blockIdx.x * kActThreads + threadIdx.x;
    if (local >= (MEMBERS ? a.member_worlds : a.num_worlds)) return;
    const uint32_t w = MEMBERS ? blockIdx.z * a.member_worlds + local : local;
    const float *__restrict__ params =
        MEMBERS ? a.params + (size_t)blockIdx.z * (mlp_net_params(D, kH, 1) + mlp_net_params(D, kH, A)) : a.params;
    float x[D];
    if constexpr (MODE == MRL_OBS_BALANCE) {
        // Seat 0's int32 row.  Rows lie 28 bytes apart, so nothing wider than a dword is aligned: every lane reads its own
        // seven dwords (the seven loads of a wavefront touch the same 1792 bytes, every cache line of them in full) and
        // the critic's workgroup stores them the same way.  The values are 0..8 and 0..2: the conversion is exact.
        const int32_t *__restrict__ in = a.obs_i32 + (size_t)w * D;
#pragma unroll
        for (int i = 0; i < D; i++) x[i] = (float)in[i];
    } else {
        const float4 s = reinterpret_cast<const float4 *>(a.state)[w];
        if (MODE == MRL_OBS_ACROBOT_GYM) {  // envs/acrobot_env.py:_observe
            x[0] = cosf(s.x);
            x[1] = sinf(s.x);
            x[2] = cosf(s.y);
            x[3] = sinf(s.y);
            x[D - 2] = s.z;
            x[D - 1] = s.w;
        } else {
            x[0] = s.x;
            x[1] = s.y;
            x[2] = s.z;
            x[3] = s.w;
        }
    }
    if (blockIdx.y == 0) {  // critic, and everything that is copied
        float v[1];
        mlp_forward<D, 1>(params, x, v);
        if (D % 2) {
            float *__restrict__ row = a.obs_row + (size_t)w * D;
#pragma unroll
            for (int i = 0; i < D; i++) row[i] = x[i];
        } else if (D == 4) {
            reinterpret_cast<float4 *>(a.obs_row)[w] = make_float4(x[0], x[1], x[2], x[3]);
        } else {
            float2 *row = reinterpret_cast<float2 *>(a.obs_row) + (size_t)w * (D / 2);
#pragma unroll
            for (int i = 0; i < D / 2; i++) row[i] = make_float2(x[2 * i], x[2 * i + 1]);
        }
        a.done_row[w] = a.reset[w] != 0 ? 1.0f : 0.0f;
        a.value_row[w] = v[0];
        if (a.reward_row) a.reward_row[w] = a.reward[w];
        return;
    }
    float l[A];
    mlp_forward<D, A>(params + mlp_net_params(D, kH, 1), x, l);
    int action;
    float logprob;
    categorical_sample<A>(l, policy_hash(a.seed, a.step, w, 0), a.flags & MRL_POLICY_GREEDY, action, logprob);
    a.action_row[w] = action;
    a.action_tensor[w] = action;
    a.logprob_row[w] = logprob;
    // the beam's other seat moves uniformly at random whatever the ego's flags: mrl_rollout_random's draw of (step, w, player 1)
    if constexpr (MODE == MRL_OBS_BALANCE) a.partner_action[w] = (int32_t)scale(policy_hash(a.seed, a.step, w, 1), A);
}

template <bool MEMBERS>
static void launch_policy_act_shape(const mrl_mlp_policy &policy, const PolicyActArgs &args, const dim3 &grid, hipStream_t stream)
{
    if (policy.obs_mode == MRL_OBS_BALANCE)
        hipLaunchKernelGGL((mrl_policy_act<7, 4, MRL_OBS_BALANCE, MEMBERS>), grid, dim3(kActThreads), 0, stream, args);
    else if (policy.obs_mode == MRL_OBS_ACROBOT_GYM)
        hipLaunchKernelGGL((mrl_policy_act<6, 3, MRL_OBS_ACROBOT_GYM, MEMBERS>), grid, dim3(kActThreads), 0, stream, args);
    else if (policy.num_actions == 3)
        hipLaunchKernelGGL((mrl_policy_act<4, 3, MRL_OBS_RAW, MEMBERS>), grid, dim3(kActThreads), 0, stream, args);
    else
        hipLaunchKernelGGL((mrl_policy_act<4, 2, MRL_OBS_RAW, MEMBERS>), grid, dim3(kActThreads), 0, stream, args);
    MRL_HIP(hipGetLastError());
}

void launch_policy_act(const mrl_mlp_policy &policy, const PolicyActArgs &args, hipStream_t stream)
{
    const uint32_t nets = args.action_row ? 2 : 1;
    if (policy.num_members) {  // (validated: num_worlds is num_members times member_worlds)
        const dim3 grid((args.member_worlds + kActThreads - 1) / kActThreads, nets, policy.num_members);
        launch_policy_act_shape<true>(policy, args, grid, stream);
    } else {
        launch_policy_act_shape<false>(policy, args, dim3((args.num_worlds + kActThreads - 1) / kActThreads, nets), stream);
    }
}

// scripts/cartpole_train_torch.py:247-256 with a lane per world: every load and store is one row, coalesced over w.
// gamma_lambda is the script's `args.gamma * args.gae_lambda`, formed by the caller.
__global__ void __launch_bounds__(256) mrl_gae(const float *__restrict__ rewards, const float *__restrict__ values,
                                               const float *__restrict__ dones, const float *__restrict__ next_value,
                                               const float *__restrict__ next_done, uint32_t num_steps, uint32_t num_worlds,
                                               float gamma, float gamma_lambda, float *__restrict__ advantages,
                                               float *__restrict__ returns)
{
    const uint32_t w = blockIdx.x * 256 + threadIdx.x;
    if (w >= num_worlds) return;
    float nextvalue = next_value[w], nextdone = next_done[w], last = 0.0f;
    for (uint32_t t = num_steps; t-- > 0;) {
        const size_t at = (size_t)t * num_worlds + w;
        const float nnt = 1.0f - nextdone, v = values[at];
        const float delta = rewards[at] + gamma * nextvalue * nnt - v;
        last = delta + gamma_lambda * nnt * last;
        advantages[at] = last;
        returns[at] = last + v;
        nextvalue = v;
        nextdone = dones[at];
    }
}

void launch_gae(const float *rewards, const float *values, const float *dones, const float *next_value, const float *next_done,
                uint32_t num_steps, uint32_t num_worlds, float gamma, float lambda, float *advantages, float *returns,
                hipStream_t stream)
{
    if (num_worlds == 0) return;
    const float gamma_lambda = (float)((double)gamma * (double)lambda);
    hipLaunchKernelGGL(mrl_gae, dim3((num_worlds + 255) / 256), dim3(256), 0, stream, rewards, values, dones, next_value, next_done,
                       num_steps, num_worlds, gamma, gamma_lambda, advantages, returns);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
