// The scaffold of MAPPO's two gradient kernels (mrl_mappo_grad in cnn_update.hip, mrl_mappo_mlp_grad in mlpbase_update.hip;
// DESIGN.md sections 16 and 18) and of their host launches: what a tile of 32 samples goes through whatever the network -- the
// sample table, the loss head, the head's backward pass, a 64 x 64 Linear layer's dW and d(in), the bias-column sums, the stats'
// tail -- and the row loop that runs a gradient launch and the optimiser tail per minibatch.  The per-sample losses and the
// accumulator tiles are mappo_loss.hpp's.  Both networks have 64 hidden units and keep their 64-wide LDS rows 65 floats apart.
#pragma once

#include "mappo_loss.hpp"

namespace mrl {

// a net's hidden width and workgroup size; kMappoTile (mappo_loss.hpp) is its tile.  Each gradient kernel asserts that its own
// net has these and keeps its 64-wide LDS rows 65 floats apart (kMappoLd).
constexpr uint32_t kMappoHidden = 64, kMappoThreads = 256, kMappoLd = kMappoHidden + 1;
constexpr uint32_t kMappoAbsent = 0xFFFFFFFFu;  // the sample table's entry of a row past the share's end

// what both gradient kernels are handed, whatever the network
struct MappoGradCommon {
    const void *obs;         // the batch's observation rows: int8 (S, H, W, F) for the CNN, int32 (S, 7) for the MLP
    const int32_t *actions;
    const float *logprobs, *value_preds, *returns, *advantages;
    const int32_t *indices;  // this row's B sample numbers
    const float *row_norm;   // this row's ValueNorm (mean, sqrt(var)); nullptr without MRL_MAPPO_VALUENORM
    float *partial_grads;    // (2, groups, stride)
    double *partial_stats;   // (2, groups, 8)
    uint64_t share, stride;
    uint32_t minibatch_size, batch_size, groups;
    MappoLoss loss;
};

// A bank update (MappoMembers, mappo_loss.hpp) runs each gradient kernel's MEMBERS = true instance with the member as
// blockIdx.z: floats (words) from a member's arrays to the next member's -- the parameters, the row of indices, the scratch
// (row_norm, partial_grads, partial_stats).  The last field of a kernel's arguments; the MEMBERS = false instance, which the
// plain update launches, does not read it and compiles to the instructions the kernel had without members.
struct MappoMemberStrides {
    uint64_t params, indices, scratch;
};

// the arguments as member blockIdx.z sees them: its own indices, row_norm and partial vectors (uniform over the workgroup; the
// caller adds the parameters' stride to its parameter pointer)
__device__ __forceinline__ MappoGradCommon mappo_member_view(const MappoGradCommon &a, const MappoMemberStrides &m)
{
    MappoGradCommon c = a;
    const size_t z = blockIdx.z;
    c.indices += z * m.indices;
    if (c.row_norm) c.row_norm += z * m.scratch;
    c.partial_grads += z * m.scratch;
    c.partial_stats += z * (m.scratch / 2u);  // (the scratch is a whole number of 16-byte units)
    return c;
}

// the tile's samples; a lane past the end runs on a zero observation with zero upstream gradient.  The caller's barrier follows.
__device__ __forceinline__ void mappo_tile_samples(const MappoGradCommon &a, uint32_t *sample, uint64_t base, uint64_t end, uint32_t tid)
{
    if (tid < kMappoTile) {
        uint32_t s = kMappoAbsent;
        if (base + tid < end) {
            s = (uint32_t)a.indices[base + tid];
            s = s < a.batch_size ? s : a.batch_size - 1u;  // outside the contract, but memory-safe
        }
        sample[tid] = s;
    }
}

// the loss head, a lane per sample: d_out (row stride 8) = dLoss / d(head output)
template <int A>
__device__ __forceinline__ void mappo_loss_head(const MappoGradCommon &a, uint32_t net, const uint32_t *sample, const float *outs,
                                                float *d_out, float count, double (&stat)[4], uint32_t tid)
{
    if (tid >= kMappoTile) return;
    float d[A];
#pragma unroll
    for (int i = 0; i < A; i++) d[i] = 0.0f;
    const uint32_t at = sample[tid];
    if (at != kMappoAbsent && net == 0u) {
        float lg[A];
#pragma unroll
        for (int i = 0; i < A; i++) lg[i] = outs[tid * 8u + i];
        mappo_actor_sample<A>(lg, a.actions[at], a.logprobs[at], a.advantages[at], a.loss, count, d, stat);
    } else if (at != kMappoAbsent) {
        d[0] = mappo_critic_sample(outs[tid * 8u], a.value_preds[at], a.returns[at], a.row_norm, a.loss, count, stat);
    }
#pragma unroll
    for (int i = 0; i < A; i++) d_out[tid * 8u + i] = d[i];
#pragma unroll
    for (int i = A; i < 8; i++) d_out[tid * 8u + i] = 0.0f;
}

// sum over the tile's samples of v[s * ld + col] (* w[s * w_ld + col]) on top of what the previous tile left, a lane per column
__device__ __forceinline__ void column_sum(float *__restrict__ g, bool first, const float *__restrict__ v, const float *__restrict__ w,
                                           uint32_t ld, uint32_t w_ld, uint32_t col)
{
    float sum = first ? 0.0f : g[col];
    for (uint32_t s = 0; s < kMappoTile; s++) sum += w ? v[s * ld + col] * w[s * w_ld + col] : v[s * ld + col];
    g[col] = sum;
}

// The head's backward pass: dW_head = d_out^T in (rows: outputs, k: samples) on waves 0 and 1, a 32-column slab each; db_head on
// wave 2; d_in[sample][j] = sum_o W_head[o][j] d_out[sample][o], GATED: kept only where gate > 0 (the ReLU in front of the head's
// input; a compile-time choice: the compiler cannot know that an LDS pointer is not null and would test it in the store loops).
// in, d_in and gate have rows of `ld` floats.
template <bool GATED>
__device__ __forceinline__ void mappo_head_backward(const float *__restrict__ head_w, float *__restrict__ g_head_w, float *__restrict__ g_head_b,
                                                    uint32_t out_dim, const float *d_out, const float *in, float *d_in, const float *gate,
                                                    uint32_t ld, bool first, uint32_t tid)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    if (wave < 2u) {
        const uint32_t col = 32u * wave + r;
        mappo_f32x16 acc = acc_load(g_head_w, kMappoHidden, out_dim, col, true, first, half);
#pragma unroll 4
        for (uint32_t kk = 0; kk < kMappoTile / 2u; kk++) {
            const uint32_t s = 2u * kk + half;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(r < out_dim ? d_out[s * 8u + r] : 0.0f, in[s * ld + col], acc, 0, 0, 0);
        }
        acc_store(g_head_w, kMappoHidden, out_dim, col, true, half, acc);
    } else if (wave == 2u && lane < out_dim) {
        column_sum(g_head_b, first, d_out, nullptr, 8u, 0u, lane);
    }
    for (uint32_t idx = tid; idx < kMappoTile * kMappoHidden; idx += kMappoThreads) {
        const uint32_t s = idx >> 6, j = idx & 63u;
        float sum = 0.0f;
        for (uint32_t o = 0; o < out_dim; o++) sum = fmaf(head_w[o * kMappoHidden + j], d_out[s * 8u + o], sum);
        d_in[s * ld + j] = !GATED || gate[s * ld + j] > 0.0f ? sum : 0.0f;
    }
}

// dW = dz^T in of a Linear(64, 64), one 32 x 32 block per wave, k = the tile's samples
__device__ __forceinline__ void mappo_dw_block(float *__restrict__ g_w, const float *dz, const float *in, uint32_t ld, bool first,
                                               uint32_t wave, uint32_t r, uint32_t half)
{
    const uint32_t jt = wave >> 1, it = wave & 1u, col = 32u * it + r;
    float *__restrict__ g = g_w + (size_t)32u * jt * kMappoHidden;
    mappo_f32x16 acc = acc_load(g, kMappoHidden, 32u, col, true, first, half);
#pragma unroll 4
    for (uint32_t kk = 0; kk < kMappoTile / 2u; kk++) {
        const uint32_t s = 2u * kk + half;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[s * ld + 32u * jt + r], in[s * ld + col], acc, 0, 0, 0);
    }
    acc_store(g, kMappoHidden, 32u, col, true, half, acc);
}

// d_in[sample][i] = sum_j dz[sample][j] W[j][i] of a Linear(64, 64), GATED: kept only where gate > 0; rows samples, k = the
// layer's units; waves 0 and 1 call it, a 32-column slab each
template <bool GATED>
__device__ __forceinline__ void mappo_d_in(const float *dz, const float *__restrict__ w, float *d_in, const float *gate, uint32_t ld,
                                           uint32_t wave, uint32_t r, uint32_t half)
{
    const uint32_t col = 32u * wave + r;
    mappo_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 4
    for (uint32_t kk = 0; kk < kMappoHidden / 2u; kk++) {
        const uint32_t j = 2u * kk + half;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[r * ld + j], w[j * kMappoHidden + col], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t row = tile_row(e, half);
        d_in[row * ld + col] = !GATED || gate[row * ld + col] > 0.0f ? acc[e] : 0.0f;
    }
}

// the stats' sums of workgroup (blockIdx.x, net): lanes in ascending order; `sums` is LDS nobody reads any more
__device__ __forceinline__ void mappo_stats_tail(const MappoGradCommon &a, uint32_t net, double *sums, const double (&stat)[4], uint32_t tid)
{
    if (tid < kMappoTile) {
#pragma unroll
        for (int c = 0; c < 4; c++) sums[c * kMappoTile + tid] = stat[c];
    }
    __syncthreads();
    if (tid < kMappoStats) {
        double sum = 0.0;
        if (tid < 4u)
            for (uint32_t s = 0; s < kMappoTile; s++) sum += sums[tid * kMappoTile + s];
        a.partial_stats[((size_t)net * a.groups + blockIdx.x) * kMappoStats + tid] = sum;
    }
}

// The host side of an update of K rows, enqueued on `stream`: ValueNorm's recurrence up front, then per row the net's gradient
// launch -- launch_grad(common arguments, workgroups per net) -- and the optimiser tail with two segments, the actor's `actor`
// parameters and then the critic's `critic` (two clip_grad_norm_ and two Adam steps).  `members` (MappoMembers): every launch
// serves that many members at once (blockIdx.z), opt, indices, value_norm_state, workspace, stats and grads being the first
// member's; launch_grad(common arguments, workgroups per net, the members' strides, their count) then launches the MEMBERS instance.
// What a row's SAMPLES are where its indices are not sample numbers (the recurrent update's rows are chunk ids): the (K, count)
// sample numbers ValueNorm's recurrence reads (nullptr: the rows' own indices) and the number of samples every mean of a row runs
// over (0: minibatch_size).
struct MappoRowSamples {
    const int32_t *indices;
    uint32_t count;
};

template <class Batch, class LaunchGrad>
inline void mappo_update_rows(uint32_t actor, uint32_t critic, const mrl_mappo_optimizer &opt, const Batch &batch, const int32_t *indices,
                              uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                              float *workspace, float *stats, float *grads, hipStream_t stream, const MappoMembers &members,
                              LaunchGrad launch_grad, const MappoRowSamples &samples = MappoRowSamples{nullptr, 0})
{
    const uint32_t row_samples = samples.count ? samples.count : minibatch_size;
    const SampleShare share = share_samples(minibatch_size, kMappoTile, kMappoMaxGroups);
    const MappoWorkspace ws = mappo_workspace(actor, minibatch_size, num_minibatches);
    const bool norm = cfg.flags & MRL_MAPPO_VALUENORM, one = members.count == 1;
    const uint64_t member_scratch = one ? 0 : ws.total, member_rows = one ? 0 : num_minibatches;
    if (norm)
        launch_mappo_value_norm(batch.returns, samples.indices ? samples.indices : indices, num_minibatches, row_samples, batch.size, cfg, value_norm_state,
                                workspace + ws.row_sums, workspace + ws.row_norm, stream, members.count, member_scratch);
    MappoGradCommon g{};
    g.obs = batch.obs;
    g.actions = batch.actions;
    g.logprobs = batch.logprobs;
    g.value_preds = batch.value_preds;
    g.returns = batch.returns;
    g.advantages = batch.advantages;
    g.partial_grads = workspace + ws.partial_grads;
    g.partial_stats = reinterpret_cast<double *>(workspace + ws.partial_stats);
    g.share = share.share;
    g.stride = ws.stride;
    const MappoMemberStrides strides{one ? 0 : members.params_stride, member_rows * minibatch_size, member_scratch};
    g.minibatch_size = minibatch_size;
    g.batch_size = batch.size;
    g.groups = share.groups;
    g.loss = MappoLoss{cfg.clip_param, cfg.entropy_coef, cfg.value_loss_coef, cfg.huber_delta, cfg.flags};
    AdamStepArgs ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.opti_eps, cfg.flags & MRL_MAPPO_MAX_GRAD_NORM, cfg.max_grad_norm);
    ad.partial_grads = g.partial_grads;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = ws.stride;
    ad.member_scratch = member_scratch;
    ad.member_params = strides.params;
    ad.member_grads_row = member_rows * ((uint64_t)actor + critic);
    ad.segments = 2;
    ad.groups = share.groups;
    ad.blocks = (uint32_t)ws.blocks;
    ad.num_params[0] = actor, ad.num_params[1] = critic;
    ad.at[0] = 0, ad.at[1] = actor;
    MappoBankStatsRow rows{{g.partial_stats, nullptr, share.groups, row_samples}, member_scratch / 2, member_rows * kMappoStats};
    MappoStatsRow &row = rows.first;
    for (uint32_t k = 0; k < num_minibatches; k++) {
        g.indices = indices + (size_t)k * minibatch_size;
        g.row_norm = norm ? workspace + ws.row_norm + 2 * (size_t)k : nullptr;
        launch_grad(g, share.groups, strides, members.count);
        MRL_HIP(hipGetLastError());
        ad.grads_row = grads ? grads + (size_t)k * ((size_t)actor + critic) : nullptr;
        adam_set_step(ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.critic_lr});
        row.row = stats ? stats + (size_t)k * kMappoStats : nullptr;
        if (one)
            launch_adam_step(ad, row, stream);
        else
            launch_adam_step_members(ad, rows, members.count, stream);
    }
}

}  // namespace mrl
