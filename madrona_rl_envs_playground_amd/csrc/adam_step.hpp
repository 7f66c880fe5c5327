// The second half of every device update (ppo_update.hip, cnn_update.hip; DESIGN.md section 13, "The optimiser tail"): the
// workgroups' partial gradient vectors become one gradient, clip_grad_norm_ and torch.optim.Adam's single-tensor step, TWO
// launches after the algorithm's own gradient kernel.  The parameters are up to two SEGMENTS (blockIdx.y), each with its own
// norm, clip and learning rate: PPO's two nets are one segment, MAPPO's actor and critic one each.  A bank update (DESIGN.md
// section 22) steps several MEMBERS in the same two launches (blockIdx.z), each on its own arrays a fixed number of floats behind
// the previous member's: the MEMBERS = true instances of the two kernels.  The MEMBERS = false instances, which every other
// update launches, read neither blockIdx.z nor the strides and compile to the instructions the kernels had without members.
// No float atomics and no wait on another workgroup: the same inputs give the same bits on every run.
#pragma once

#include "common.hpp"

#include <cmath>

namespace mrl {

constexpr uint32_t kAdamThreads = 256;
constexpr uint32_t kAdamSegments = 2;

// a fixed tree over the workgroup's values; the result is in every thread
template <int THREADS, typename T>
__device__ __forceinline__ T block_sum(T v, T *scratch)
{
    __syncthreads();
    scratch[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int width = THREADS / 2; width > 0; width /= 2) {
        if ((int)threadIdx.x < width) scratch[threadIdx.x] += scratch[threadIdx.x + width];
        __syncthreads();
    }
    return scratch[0];
}

// How the B samples of a row are shared out: workgroup g of `groups` owns samples [g * share, min(B, (g + 1) * share)),
// share a whole number of tiles.  Every workgroup owns at least one sample.
struct SampleShare {
    uint32_t groups;
    uint64_t share;
};

inline SampleShare share_samples(uint32_t minibatch_size, uint32_t tile, uint32_t max_groups)
{
    const uint64_t tiles = ((uint64_t)minibatch_size + tile - 1) / tile;
    const uint64_t want = tiles < max_groups ? tiles : max_groups;
    const uint64_t tiles_each = want ? (tiles + want - 1) / want : 1;
    SampleShare s;
    s.groups = (uint32_t)(tiles_each ? (tiles + tiles_each - 1) / tiles_each : 0);
    s.share = tiles_each * tile;
    return s;
}

struct AdamStepArgs {
    const float *partial_grads;  // [segment][groups][stride]
    float *grad, *sumsq;         // [segment][stride], [segment][blocks]
    float *grads_row;            // the row's unclipped gradient in parameter order, or nullptr
    float *params, *exp_avg, *exp_avg_sq;
    const uint32_t *skip;  // nullptr, or a device word: non-zero leaves grad, grads_row, the parameters and the moments as they are
    uint64_t stride;
    uint32_t segments, groups, blocks;      // blocks of kAdamThreads per segment, the same for both
    uint32_t clip;                          // 0: no clip_grad_norm_
    uint32_t num_params[kAdamSegments];     // the segment's parameters ...
    uint32_t at[kAdamSegments];             // ... and where they start in params, exp_avg, exp_avg_sq and grads_row
    float step_size[kAdamSegments];
    float max_grad_norm, bias2_sqrt, beta1, beta2, one_minus_beta1, one_minus_beta2, eps;
    // MEMBERS only -- floats from a member's arrays to the next member's: the scratch (partial_grads, grad, sumsq), the bank's
    // rows (params, exp_avg, exp_avg_sq), grads_row.  (Last, so that every other field is where it was.)
    uint64_t member_scratch, member_params, member_grads_row;
};

// what does not change from row to row; the caller adds the arrays and the segments
inline AdamStepArgs adam_step_args(float beta1, float beta2, float eps, bool clip, float max_grad_norm)
{
    AdamStepArgs a{};
    a.clip = clip ? 1u : 0u;
    a.max_grad_norm = max_grad_norm;
    a.beta1 = beta1;
    a.beta2 = beta2;
    a.one_minus_beta1 = (float)(1.0 - (double)beta1);
    a.one_minus_beta2 = (float)(1.0 - (double)beta2);
    a.eps = eps;
    return a;
}

// Adam's step t (from 1) with the segments' learning rates.  torch's _single_tensor_adam forms these in Python floats:
// step_size = lr / (1 - beta1^t), sqrt(1 - beta2^t)
inline void adam_set_step(AdamStepArgs &a, double t, const float (&lr)[kAdamSegments])
{
    const double bias1 = 1.0 - std::pow((double)a.beta1, t);
    for (uint32_t s = 0; s < kAdamSegments; s++) a.step_size[s] = (float)((double)lr[s] / bias1);
    a.bias2_sqrt = (float)std::sqrt(1.0 - std::pow((double)a.beta2, t));
}

// member blockIdx.z's array behind the first member's (MEMBERS), or the array itself: the kernels below never write to their
// argument struct, which would send all of it to scratch memory
template <bool MEMBERS, typename T>
__device__ __forceinline__ T *member_array(T *first, uint64_t stride)
{
    return MEMBERS ? first + (size_t)blockIdx.z * stride : first;
}

// adds the partial vectors in ascending workgroup order and forms per-block sums of g^2.  (A template, as mrl_clip_adam has to
// be one: the header is compiled into more than one object.)
template <int THREADS, bool MEMBERS = false>
__global__ void __launch_bounds__(THREADS) mrl_grad_reduce(AdamStepArgs a)
{
    __shared__ float scratch[THREADS];
    if (a.skip && *a.skip) return;  // (uniform over the grid)
    const uint32_t seg = blockIdx.y, p = blockIdx.x * THREADS + threadIdx.x;
    const float *__restrict__ partial = member_array<MEMBERS>(a.partial_grads, a.member_scratch) + (size_t)seg * a.groups * a.stride;
    float g = 0.0f;
    if (p < a.num_params[seg]) {
        for (uint32_t w = 0; w < a.groups; w++) g += partial[(size_t)w * a.stride + p];
        member_array<MEMBERS>(a.grad, a.member_scratch)[(size_t)seg * a.stride + p] = g;
        if (a.grads_row) member_array<MEMBERS>(a.grads_row, a.member_grads_row)[a.at[seg] + p] = g;
    }
    const float total = block_sum<THREADS>(g * g, scratch);  // (a block past the segment's end adds 0 to its norm)
    if (threadIdx.x == 0) member_array<MEMBERS>(a.sumsq, a.member_scratch)[seg * a.blocks + blockIdx.x] = total;
}

// clip_grad_norm_ and torch.optim.Adam's single-tensor step, per segment.  Thread 0 of block 0 of each segment then calls
// stats(segment, total norm), the algorithm's own end of the stats row (with a non-zero skip word: stats(segment, 0) alone); a
// functor that serves several members reads blockIdx.z itself.
template <typename STATS, bool MEMBERS = false>
__global__ void __launch_bounds__(kAdamThreads) mrl_clip_adam(AdamStepArgs a, STATS stats)
{
    const uint32_t seg = blockIdx.y;
    if (a.skip && *a.skip) {
        if (blockIdx.x == 0 && threadIdx.x == 0) stats(seg, 0.0f);
        return;
    }
    float squares = 0.0f;
    for (uint32_t b = 0; b < a.blocks; b++) squares += member_array<MEMBERS>(a.sumsq, a.member_scratch)[seg * a.blocks + b];
    const float total = sqrtf(squares);
    const float scale = a.clip ? fminf(a.max_grad_norm / (total + 1e-6f), 1.0f) : 1.0f;
    const uint32_t p = blockIdx.x * kAdamThreads + threadIdx.x;
    if (p < a.num_params[seg]) {
        const size_t at = (size_t)a.at[seg] + p;
        float *exp_avg = member_array<MEMBERS>(a.exp_avg, a.member_params), *exp_avg_sq = member_array<MEMBERS>(a.exp_avg_sq, a.member_params);
        const float g = member_array<MEMBERS>(a.grad, a.member_scratch)[(size_t)seg * a.stride + p] * scale;
        const float m = a.beta1 * exp_avg[at] + a.one_minus_beta1 * g;
        const float v = a.beta2 * exp_avg_sq[at] + a.one_minus_beta2 * (g * g);
        exp_avg[at] = m;
        exp_avg_sq[at] = v;
        member_array<MEMBERS>(a.params, a.member_params)[at] -= a.step_size[seg] * (m / (sqrtf(v) / a.bias2_sqrt + a.eps));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) stats(seg, total);
}

// the two launches that follow a row's gradient kernel
template <typename STATS>
inline void launch_adam_step(const AdamStepArgs &a, const STATS &stats, hipStream_t stream)
{
    const dim3 grid(a.blocks, a.segments);
    hipLaunchKernelGGL(mrl_grad_reduce<(int)kAdamThreads>, grid, dim3(kAdamThreads), 0, stream, a);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(mrl_clip_adam<STATS>, grid, dim3(kAdamThreads), 0, stream, a, stats);
    MRL_HIP(hipGetLastError());
}

// the same two launches for `members` members of a bank (a's member strides set; `stats` reads blockIdx.z itself)
template <typename STATS>
inline void launch_adam_step_members(const AdamStepArgs &a, const STATS &stats, uint32_t members, hipStream_t stream)
{
    const dim3 grid(a.blocks, a.segments, members);
    hipLaunchKernelGGL((mrl_grad_reduce<(int)kAdamThreads, true>), grid, dim3(kAdamThreads), 0, stream, a);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL((mrl_clip_adam<STATS, true>), grid, dim3(kAdamThreads), 0, stream, a, stats);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
