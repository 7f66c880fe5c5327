// The update phase of PPO on the device (C ABI: mrl_ppo_update, mrl_ppo_workspace_bytes in include/mrl_envs.h).
// The kernels live in ppo_update_kernels.hpp, compiled into ppo_update.hip (one policy) and ppo_update_bank.hip (the members of a
// bank); capi_ppo.hip validates the arguments and calls launch_ppo_update.  DESIGN.md sections 13 and 26.
#pragma once

#include "adam_step.hpp"
#include "policy_rollout.hpp"

namespace mrl {

constexpr uint32_t kPpoTile = 64;        // samples a gradient workgroup (one wavefront) takes at a time: a lane per sample
constexpr uint32_t kPpoMaxGroups = 256;  // workgroups per net, hence partial gradient vectors per row, however large B is
constexpr uint32_t kPpoStats = 8;        // columns of a stats row

// The caller's scratch, in floats: [mean, std + 1e-8] of every row's advantages; the workgroups' partial gradients
// (groups, P) and partial stats (groups, 8), doubles; the summed gradient (P); the reduce launch's per-block sums of g^2.
struct PpoWorkspace {
    uint64_t mean_std, partial_grads, partial_stats, grad, sumsq, total;
};

inline PpoWorkspace ppo_workspace(uint64_t num_params, uint32_t minibatch_size, uint32_t num_minibatches)
{
    const auto pad = [](uint64_t n) { return (n + 3) & ~uint64_t(3); };  // every array on a 16-byte boundary
    // room for min(tiles, cap) workgroups, which never shrinks as B grows; share_samples may use fewer (no empty workgroup)
    const uint64_t tiles = ((uint64_t)minibatch_size + kPpoTile - 1) / kPpoTile;
    const uint64_t groups = tiles < kPpoMaxGroups ? tiles : kPpoMaxGroups;
    PpoWorkspace w;
    w.mean_std = 0;
    w.partial_grads = pad(2 * (uint64_t)num_minibatches);
    w.partial_stats = w.partial_grads + pad(groups * num_params);
    w.grad = w.partial_stats + pad(2 * groups * kPpoStats);
    w.sumsq = w.grad + pad(num_params);
    w.total = w.sumsq + pad((num_params + kAdamThreads - 1) / kAdamThreads);
    return w;
}

// K rows enqueued on `stream`; every argument has been validated (capi_ppo.hip, mrl_ppo_update).  With opt.num_members = M != 0
// every row steps M members in the same three launches (blockIdx.z): opt's arrays are the first of M dense rows, indices
// (M, K, B), stats (M, K, 8), grads (M, K, P), and workspace M slices of ppo_workspace(...).total floats.
void launch_ppo_update(const mrl_mlp_policy &shape, const mrl_ppo_optimizer &opt, const mrl_ppo_batch &batch,
                       const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config &cfg,
                       float *workspace, float *stats, float *grads, hipStream_t stream);

// what launch_ppo_update hands a call with opt.num_members != 0 to (ppo_update_bank.hip)
void launch_ppo_update_members(const mrl_mlp_policy &shape, const mrl_ppo_optimizer &opt, const mrl_ppo_batch &batch,
                               const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config &cfg,
                               float *workspace, float *stats, float *grads, hipStream_t stream);

}  // namespace mrl
