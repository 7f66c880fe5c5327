// mrl_mappo_update: MAPPO's update for the Overcooked CNN actor-critic without torch in the loop (include/mrl_envs.h,
// mrl_mappo_update).
//
// The reference runs, per minibatch, a float copy of the observations, two CNN forward and backward passes, ValueNorm, two
// clip_grad_norm_ and two Adam steps in torch (train/MAPPO/r_mappo.py:91-164).  Here one row is THREE launches, after TWO up
// front for every row's ValueNorm statistics (they depend on no parameter):
//   mrl_mappo_grad    workgroup (g, net) of four wavefronts owns samples [g * share, (g + 1) * share) of the row for the actor
//                     (net 0) or the critic (net 1) and takes them 32 at a time.  Per tile: the forward pass of mrl_cnn_act into
//                     LDS (the same device functions, hence the same bits), the loss head (a lane per sample), then
//                     back-propagation through head, fc2, fc1 and the convolution's ReLU.  Every product with a sample or a
//                     unit dimension to sum over runs on v_mfma_f32_32x32x2_f32: the weight gradients with k = the tile's
//                     samples (dW_conv: k = (position, sample)), the activation gradients with k = the layer's units.  The
//                     accumulators live in the workgroup's own partial vector in global memory: a tile's products start from
//                     the value the same lane stored after the previous tile (0 for the first), so a sum over the share is ONE
//                     chain of fused multiply-adds in sample order, and nothing but its owner ever touches the vector.
//   mrl_grad_reduce   adds the partial vectors in ascending workgroup order and forms per-block sums of g^2, per net.
//   mrl_clip_adam     per net: total norm, clip, Adam with the net's learning rate, and the net's columns of the stats row
//                     (adam_step.hpp: the tail every update shares; each net is a segment).
// mrl_mappo_bank_update is the same launches with a third grid dimension, the member of the bank: a
// member's workgroups read its own parameters, indices and ValueNorm rows and write its own partial vectors (the kernels'
// MEMBERS = true instances; the plain update runs the MEMBERS = false ones, which are the kernels as they were).
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run.
// The per-sample losses, the accumulator tiles and the stats row's end are mappo_loss.hpp's; the sample table, the loss head, the
// backward pass of the head and of fc2, the bias-column sums, the stats' tail and the host's row loop are mappo_grad.hpp's: both
// shared with the balance beam's update (mlpbase_update.hip).  What is left here is what a convolution net has of its own.  The
// ValueNorm launches are defined here and declared in mappo_loss.hpp.
#include "cnn_update.hpp"
#include "cnn_forward.hpp"
#include "mappo_grad.hpp"

#include <cmath>

namespace mrl {

namespace {

constexpr uint32_t kStatThreads = 1024;

static_assert(kCnnHidden == kMappoHidden && kCnnThreads == kMappoThreads && kCnnTile == kMappoTile && kCnnFcLd == kMappoLd,
              "mappo_grad.hpp's functions are written for this net's width, workgroup, tile and LDS row stride");

extern __shared__ __attribute__((aligned(16))) unsigned char upd_lds_image[];

struct MappoGradArgs {
    MappoGradCommon common;
    CnnActArgs fwd;  // W, H, F and the LDS image of the forward pass; params
    uint32_t tail_at;
    MappoMemberStrides members;  // MEMBERS only
};

// MEMBERS: member blockIdx.z of a bank update, on its own parameters, indices, ValueNorm rows and partial vectors
template <bool MEMBERS>
__global__ void __launch_bounds__(kCnnThreads) mrl_mappo_grad(MappoGradArgs a)
{
    const MappoGradCommon own = MEMBERS ? mappo_member_view(a.common, a.members) : MappoGradCommon{};
    const MappoGradCommon &c = MEMBERS ? own : a.common;
    const CnnActArgs &f = a.fwd;
    const CnnLds &l = f.lds;
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x;
    const uint32_t k1 = l.k1, npos = l.npos, K2 = kCnnChannels * npos, out_dim = net ? 1u : kCnnActions, act_ld = l.act_ld;
    const size_t net_at = net ? cnn_net_params(f.W, f.H, f.F, kCnnActions) : 0;
    const float *__restrict__ conv_w = f.params + (MEMBERS ? (size_t)blockIdx.z * a.members.params : 0) + net_at;
    const float *__restrict__ conv_b = conv_w + (size_t)kCnnChannels * k1;
    const float *__restrict__ fc1_w = conv_b + kCnnChannels, *__restrict__ fc1_b = fc1_w + (size_t)kCnnHidden * K2;
    const float *__restrict__ fc2_w = fc1_b + kCnnHidden, *__restrict__ fc2_b = fc2_w + kCnnHidden * kCnnHidden;
    const float *__restrict__ head_w = fc2_b + kCnnHidden, *__restrict__ head_b = head_w + out_dim * kCnnHidden;
    // this workgroup's partial vector, in the net's parameter order
    float *__restrict__ g_conv_w = c.partial_grads + ((size_t)net * c.groups + blockIdx.x) * c.stride;
    float *__restrict__ g_conv_b = g_conv_w + (size_t)kCnnChannels * k1;
    float *__restrict__ g_fc1_w = g_conv_b + kCnnChannels, *__restrict__ g_fc1_b = g_fc1_w + (size_t)kCnnHidden * K2;
    float *__restrict__ g_fc2_w = g_fc1_b + kCnnHidden, *__restrict__ g_fc2_b = g_fc2_w + kCnnHidden * kCnnHidden;
    float *__restrict__ g_head_w = g_fc2_b + kCnnHidden, *__restrict__ g_head_b = g_head_w + out_dim * kCnnHidden;

    unsigned char *lds = upd_lds_image;
    const uint16_t *koff = reinterpret_cast<const uint16_t *>(lds + l.koff_at);
    float *act = reinterpret_cast<float *>(lds + l.act_at);
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + a.tail_at), *shifts = sample + kCnnTile;
    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt);
    float *h1 = reinterpret_cast<float *>(lds + kCnnH1At), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt);
    float *d_out = reinterpret_cast<float *>(lds + kUpdDoutAt), *d_h2 = reinterpret_cast<float *>(lds + kUpdDh2At);
    float *d_h1 = reinterpret_cast<float *>(lds + kUpdDh1At);

    const uint64_t begin = blockIdx.x * c.share;
    const uint64_t end = begin + c.share < c.minibatch_size ? begin + c.share : c.minibatch_size;
    const float count = (float)c.minibatch_size;
    // a row of the tile in the batch, or nullptr where the tile has no such row
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        const uint32_t s = sample[rr];
        return s == kMappoAbsent ? nullptr : static_cast<const uint8_t *>(c.obs) + (size_t)s * (f.W * f.H * f.F);
    };
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    for (uint64_t base = begin; base < end; base += kCnnTile) {
        const bool first = base == begin;
        const uint32_t tid = opaque(tid0), lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
        mappo_tile_samples(c, sample, base, end, tid);
        __syncthreads();
        cnn_load_tile(f, lds, row_address, shifts, conv_w, true);
        __syncthreads();
        // ---- the forward pass of mrl_cnn_act
        cnn_conv_tile(f, lds, shifts[r], conv_b, wave, r, half);
        __syncthreads();  // the activation image is complete; the convolution's operands are dead
        cnn_fc_layer(act, act_ld, K2, fc1_w, fc1_b, kCnnHidden, true, chunk, h1, kCnnFcLd, wave, lane);
        cnn_fc_layer(h1, kCnnFcLd, kCnnHidden, fc2_w, fc2_b, kCnnHidden, true, chunk, h2, kCnnFcLd, wave, lane);
        cnn_fc_layer(h2, kCnnFcLd, kCnnHidden, head_w, head_b, out_dim, false, chunk, outs, 8u, wave, lane);

        mappo_loss_head<(int)kCnnActions>(c, net, sample, outs, d_out, count, stat, tid);
        __syncthreads();
        // ---- head: dW_head, db_head and d_h2 behind fc2's ReLU
        mappo_head_backward<true>(head_w, g_head_w, g_head_b, out_dim, d_out, h2, d_h2, h2, kCnnFcLd, first, tid);
        __syncthreads();
        // ---- fc2: dW_fc2 = d_h2^T h1; d_h1 behind fc1's ReLU on waves 0 and 1; db_fc2
        mappo_dw_block(g_fc2_w, d_h2, h1, kCnnFcLd, first, wave, r, half);
        if (wave < 2u)
            mappo_d_in<true>(d_h2, fc2_w, d_h1, h1, kCnnFcLd, wave, r, half);
        else if (wave == 2u)
            column_sum(g_fc2_b, first, d_h2, nullptr, kCnnFcLd, 0u, lane);
        __syncthreads();

        // ---- fc1: dW_fc1 = d_h1^T act (64 x 32 npos) while act is intact: wave w takes the column slabs w, w + 4, ..., both row
        // blocks of a slab on one read of act
#pragma unroll 1
        for (uint32_t ct = wave; ct < npos; ct += 4u) {
            const uint32_t col = 32u * ct + r;
            float *__restrict__ g0 = g_fc1_w, *__restrict__ g1 = g_fc1_w + (size_t)32u * K2;
            f32x16 acc0 = acc_load(g0, K2, 32u, col, true, first, half), acc1 = acc_load(g1, K2, 32u, col, true, first, half);
#pragma unroll 4
            for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                const uint32_t s = 2u * kk + half;
                const float b = act[s * act_ld + col];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[s * kCnnFcLd + r], b, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[s * kCnnFcLd + 32u + r], b, acc1, 0, 0, 0);
            }
            acc_store(g0, K2, 32u, col, true, half, acc0);
            acc_store(g1, K2, 32u, col, true, half, acc1);
        }
        if (wave == 3u) column_sum(g_fc1_b, first, d_h1, nullptr, kCnnFcLd, 0u, lane);
        __syncthreads();
        // act in place becomes dL/d(conv pre-activation) = (act > 0) sum_j d_h1[sample][j] W_fc1[j][.]: rows samples, k = units
#pragma unroll 1
        for (uint32_t ct = wave; ct < npos; ct += 4u) {
            const uint32_t col = 32u * ct + r;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 4
            for (uint32_t kk = 0; kk < kCnnHidden / 2u; kk++) {
                const uint32_t j = 2u * kk + half;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[r * kCnnFcLd + j], fc1_w[(size_t)j * K2 + col], acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                float *p = act + tile_row(e, half) * act_ld + col;
                *p = *p > 0.0f ? acc[e] : 0.0f;
            }
        }
        __syncthreads();  // d_h1 and everything else in region A is dead

        // ---- convolution: the observation rows again (out of L2), then dW_conv[c][k] = sum over (position, sample) of
        // d_conv[sample][c][position] * patch[sample][position][k]: rows channels, columns k in slabs of 32, wave w takes slabs w, w + 4
        cnn_load_tile(f, lds, row_address, shifts, conv_w, false);
        __syncthreads();
        {
            const uint32_t hh = f.H - 2u, slabs = (k1 + 31u) / 32u;
#pragma unroll 1
            for (uint32_t kt = wave; kt < slabs; kt += 4u) {
                const uint32_t k = 32u * kt + r;
                const bool ok = k < k1;
                const uint32_t off = ok ? koff[k] : 0u;
                f32x16 acc = acc_load(g_conv_w, k1, kCnnChannels, k, ok, first, half);
#pragma unroll 1
                for (uint32_t pos = 0; pos < npos; pos++) {
                    const uint32_t ow = pos / hh, oh = pos - ow * hh, at = (oh * f.W + ow) * f.F + off;
#pragma unroll 4
                    for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                        const uint32_t s = 2u * kk + half;
                        const int8_t byte = reinterpret_cast<const int8_t *>(lds)[s * l.obs_ld + shifts[s] + at];
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(act[s * act_ld + r * npos + pos], ok ? (float)byte : 0.0f, acc, 0, 0, 0);
                    }
                }
                acc_store(g_conv_w, k1, kCnnChannels, k, ok, half, acc);
            }
            if (slabs % 4u == wave && lane < kCnnChannels) {  // the wave with the fewest slabs: db_conv
                float sum = first ? 0.0f : g_conv_b[lane];
                for (uint32_t s = 0; s < kCnnTile; s++)
                    for (uint32_t pos = 0; pos < npos; pos++) sum += act[s * act_ld + lane * npos + pos];
                g_conv_b[lane] = sum;
            }
        }
        __syncthreads();  // the next tile overwrites what the loops above read
    }

    mappo_stats_tail(c, net, reinterpret_cast<double *>(lds), stat, tid0);
}

// ValueNorm, first launch: the mean and the mean of squares of every row's gathered returns, one workgroup per (row, member);
// a member's row_sums lie member_scratch floats behind the previous member's
__global__ void __launch_bounds__(kStatThreads) mrl_mappo_row_sums(const float *__restrict__ returns, const int32_t *__restrict__ indices,
                                                                  uint32_t minibatch_size, uint32_t batch_size, float *__restrict__ row_sums,
                                                                  uint64_t member_scratch)
{
    __shared__ double scratch[kStatThreads];
    const int32_t *row = indices + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * minibatch_size;
    row_sums += (size_t)blockIdx.y * member_scratch;
    double sum = 0.0, squares = 0.0;
    for (uint64_t b = threadIdx.x; b < minibatch_size; b += kStatThreads) {  // (64 bits: B may be within 1024 of 2^32)
        uint32_t s = (uint32_t)row[b];
        s = s < batch_size ? s : batch_size - 1u;
        const float v = returns[s];
        sum += (double)v;
        squares += (double)(v * v);
    }
    const double total = block_sum<(int)kStatThreads>(sum, scratch), total_sq = block_sum<(int)kStatThreads>(squares, scratch);
    if (threadIdx.x == 0) {
        row_sums[2 * blockIdx.x] = (float)(total / (double)minibatch_size);
        row_sums[2 * blockIdx.x + 1] = (float)(total_sq / (double)minibatch_size);
    }
}

// ValueNorm, second launch: utils/valuenorm.py's update and running_mean_var over the K rows, one thread per member (a
// workgroup each), float32 as torch's; member blockIdx.x has state row blockIdx.x of (members, 3)
__global__ void mrl_mappo_value_norm(const float *__restrict__ row_sums, uint32_t rows, float beta, float one_minus_beta, float epsilon,
                                     float *__restrict__ state, float *__restrict__ row_norm, uint64_t member_scratch)
{
    if (threadIdx.x != 0) return;
    row_sums += (size_t)blockIdx.x * member_scratch;
    row_norm += (size_t)blockIdx.x * member_scratch;
    state += 3u * blockIdx.x;
    float mean = state[0], mean_sq = state[1], debias = state[2];
    for (uint32_t k = 0; k < rows; k++) {
        mean = mean * beta + row_sums[2 * k] * one_minus_beta;
        mean_sq = mean_sq * beta + row_sums[2 * k + 1] * one_minus_beta;
        debias = debias * beta + one_minus_beta;
        const float floor = fmaxf(debias, epsilon);
        const float m = mean / floor, var = fmaxf(mean_sq / floor - m * m, 1e-2f);
        row_norm[2 * k] = m;
        row_norm[2 * k + 1] = sqrtf(var);
    }
    state[0] = mean;
    state[1] = mean_sq;
    state[2] = debias;
}

}  // namespace

void launch_mappo_value_norm(const float *returns, const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size,
                             uint32_t batch_size, const mrl_mappo_config &cfg, float *state, float *row_sums, float *row_norm,
                             hipStream_t stream, uint32_t members, uint64_t member_scratch)
{
    hipLaunchKernelGGL(mrl_mappo_row_sums, dim3(num_minibatches, members), dim3(kStatThreads), 0, stream, returns, indices, minibatch_size,
                       batch_size, row_sums, member_scratch);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(mrl_mappo_value_norm, dim3(members), dim3(64), 0, stream, row_sums, num_minibatches, cfg.valuenorm_beta,
                       cfg.valuenorm_one_minus_beta, cfg.valuenorm_epsilon, state, row_norm, member_scratch);
    MRL_HIP(hipGetLastError());
}

void launch_mappo_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_batch &batch,
                         const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                         float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream,
                         const MappoMembers &members)
{
    if (num_minibatches == 0) return;
    const uint32_t W = policy.width, H = policy.height, F = policy.channels;
    const CnnUpdateLds lds = cnn_update_lds(W, H, F);
    allow_large_dynamic_lds<&mrl_mappo_grad<false>>(lds.total);
    allow_large_dynamic_lds<&mrl_mappo_grad<true>>(lds.total);
    MappoGradArgs g{};
    g.fwd.params = opt.params_dev;
    g.fwd.W = W;
    g.fwd.H = H;
    g.fwd.F = F;
    g.fwd.lds = lds.fwd;
    g.tail_at = lds.tail_at;
    mappo_update_rows((uint32_t)cnn_net_params(W, H, F, kCnnActions), (uint32_t)cnn_net_params(W, H, F, 1), opt, batch, indices, num_minibatches,
                      minibatch_size, cfg, value_norm_state, workspace, stats, grads, stream, members,
                      [&](const MappoGradCommon &common, uint32_t groups, const MappoMemberStrides &strides, uint32_t count) {
                          g.common = common;
                          g.members = strides;
                          if (count == 1)
                              hipLaunchKernelGGL(mrl_mappo_grad<false>, dim3(groups, 2), dim3(kCnnThreads), lds.total, stream, g);
                          else
                              hipLaunchKernelGGL(mrl_mappo_grad<true>, dim3(groups, 2, count), dim3(kCnnThreads), lds.total, stream, g);
                      });
}

}  // namespace mrl
