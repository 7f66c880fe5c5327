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
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run.
// The per-sample loss head, the accumulator tiles and the stats row's end are mappo_loss.hpp's, shared with the balance beam's
// update (mlpbase_update.hip); the ValueNorm launches are defined here and declared there.
#include "cnn_update.hpp"
#include "cnn_forward.hpp"

#include <cmath>

namespace mrl {

namespace {

constexpr uint32_t kStatThreads = 1024;

extern __shared__ __attribute__((aligned(16))) unsigned char upd_lds_image[];

struct MappoGradArgs {
    CnnActArgs fwd;  // W, H, F and the LDS image of the forward pass; params
    const int8_t *obs;
    const int32_t *actions;
    const float *logprobs, *value_preds, *returns, *advantages;
    const int32_t *indices;  // this row's B sample numbers
    const float *row_norm;   // this row's ValueNorm (mean, sqrt(var)); nullptr without MRL_MAPPO_VALUENORM
    float *partial_grads;    // (2, groups, stride)
    double *partial_stats;   // (2, groups, 8)
    uint64_t share, stride;
    uint32_t minibatch_size, batch_size, groups, tail_at;
    MappoLoss loss;
};

// the tile's observation rows (mrl_cnn_act's loader with the row taken from the sample table), the patch offsets of k and, for
// the forward pass, the conv weights
__device__ __forceinline__ void load_rows(const MappoGradArgs &a, unsigned char *lds, const uint32_t *sample, uint32_t *shifts,
                                          const float *__restrict__ conv_w, bool with_weights)
{
    const CnnLds &l = a.fwd.lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t S = a.fwd.W * a.fwd.H * a.fwd.F, k1 = l.k1;
    uint32_t *obs_words = reinterpret_cast<uint32_t *>(lds);
    for (uint32_t rr = wave; rr < kCnnTile; rr += 4u) {
        uint32_t *__restrict__ dst = obs_words + rr * (l.obs_ld / 4u);
        const uint32_t s = sample[rr];
        if (s == 0xFFFFFFFFu) {
            for (uint32_t d = lane; d < (S + 3u) / 4u; d += 64u) dst[d] = 0u;
            if (lane == 0) shifts[rr] = 0u;
            continue;
        }
        const uint8_t *__restrict__ row = reinterpret_cast<const uint8_t *>(a.obs) + (size_t)s * S;
        const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(row) & 3u), words = (shift + S + 3u) / 4u;
        if (lane == 0) shifts[rr] = shift;
        for (uint32_t d = lane; d < words; d += 64u) {
            const int32_t g = (int32_t)(4u * d) - (int32_t)shift;  // the dword's first byte, counted from the row's start
            uint32_t v = 0u;
            if (g >= 0 && (uint32_t)g + 4u <= S) {
                v = *reinterpret_cast<const uint32_t *>(row + g);
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int32_t at = g + b;
                    if (at >= 0 && (uint32_t)at < S) v |= (uint32_t)row[at] << (8 * b);
                }
            }
            dst[d] = v;
        }
    }
    if (with_weights) {
        float *w_lds = reinterpret_cast<float *>(lds + l.conv_w_at);
        for (uint32_t e = tid; e < kCnnChannels * k1; e += kCnnThreads) {
            const uint32_t c = e / k1, k = e - c * k1;
            w_lds[c * l.conv_ld + k] = conv_w[e];
        }
        if (k1 != l.k1_padded && tid < kCnnChannels) w_lds[tid * l.conv_ld + k1] = 0.0f;
    }
    uint16_t *koff = reinterpret_cast<uint16_t *>(lds + l.koff_at);
    for (uint32_t k = tid; k < l.k1_padded; k += kCnnThreads) {
        const uint32_t f = k / 9u, ij = k - 9u * f, i = ij / 3u, j = ij - 3u * i;
        koff[k] = k < k1 ? (uint16_t)((j * a.fwd.W + i) * a.fwd.F + f) : (uint16_t)0;
    }
}

__global__ void __launch_bounds__(kCnnThreads) mrl_mappo_grad(MappoGradArgs a)
{
    const CnnActArgs &f = a.fwd;
    const CnnLds &l = f.lds;
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x;
    const uint32_t k1 = l.k1, npos = l.npos, K2 = kCnnChannels * npos, out_dim = net ? 1u : kCnnActions, act_ld = l.act_ld;
    const size_t net_at = net ? cnn_net_params(f.W, f.H, f.F, kCnnActions) : 0;
    const float *__restrict__ conv_w = f.params + net_at;
    const float *__restrict__ conv_b = conv_w + (size_t)kCnnChannels * k1;
    const float *__restrict__ fc1_w = conv_b + kCnnChannels, *__restrict__ fc1_b = fc1_w + (size_t)kCnnHidden * K2;
    const float *__restrict__ fc2_w = fc1_b + kCnnHidden, *__restrict__ fc2_b = fc2_w + kCnnHidden * kCnnHidden;
    const float *__restrict__ head_w = fc2_b + kCnnHidden, *__restrict__ head_b = head_w + out_dim * kCnnHidden;
    // this workgroup's partial vector, in the net's parameter order
    float *__restrict__ g_conv_w = a.partial_grads + ((size_t)net * a.groups + blockIdx.x) * a.stride;
    float *__restrict__ g_conv_b = g_conv_w + (size_t)kCnnChannels * k1;
    float *__restrict__ g_fc1_w = g_conv_b + kCnnChannels, *__restrict__ g_fc1_b = g_fc1_w + (size_t)kCnnHidden * K2;
    float *__restrict__ g_fc2_w = g_fc1_b + kCnnHidden, *__restrict__ g_fc2_b = g_fc2_w + kCnnHidden * kCnnHidden;
    float *__restrict__ g_head_w = g_fc2_b + kCnnHidden, *__restrict__ g_head_b = g_head_w + out_dim * kCnnHidden;

    unsigned char *lds = upd_lds_image;
    float *w_lds = reinterpret_cast<float *>(lds + l.conv_w_at);
    uint16_t *koff = reinterpret_cast<uint16_t *>(lds + l.koff_at);
    float *act = reinterpret_cast<float *>(lds + l.act_at);
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + a.tail_at), *shifts = sample + kCnnTile;
    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt);
    float *h1 = reinterpret_cast<float *>(lds + kCnnH1At), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt);
    float *d_out = reinterpret_cast<float *>(lds + kUpdDoutAt), *d_h2 = reinterpret_cast<float *>(lds + kUpdDh2At);
    float *d_h1 = reinterpret_cast<float *>(lds + kUpdDh1At);

    const uint64_t begin = blockIdx.x * a.share;
    const uint64_t end = begin + a.share < a.minibatch_size ? begin + a.share : a.minibatch_size;
    const float count = (float)a.minibatch_size;
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    for (uint64_t base = begin; base < end; base += kCnnTile) {
        const bool first = base == begin;
        const uint32_t tid = opaque(tid0), lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
        // ---- the tile's samples; a lane past the end runs on a zero observation with zero upstream gradient
        if (tid < kCnnTile) {
            uint32_t s = 0xFFFFFFFFu;
            if (base + tid < end) {
                s = (uint32_t)a.indices[base + tid];
                s = s < a.batch_size ? s : a.batch_size - 1u;  // outside the contract, but memory-safe
            }
            sample[tid] = s;
        }
        __syncthreads();
        load_rows(a, lds, sample, shifts, conv_w, true);
        __syncthreads();
        // ---- the forward pass of mrl_cnn_act
        {
            const int8_t *__restrict__ my_obs = reinterpret_cast<const int8_t *>(lds) + r * l.obs_ld + shifts[r];
            const float *__restrict__ my_w = w_lds + r * l.conv_ld;
            const float bias = conv_b[r];
            for (uint32_t p0 = wave; p0 < npos; p0 += 12u) {
                const uint32_t n = (npos - p0 + 3u) / 4u;  // positions p0, p0 + 4, p0 + 8 that exist
                if (n >= 3u)
                    cnn_conv_pass<3>(f, my_obs, my_w, koff, act, bias, p0, r, half);
                else if (n == 2u)
                    cnn_conv_pass<2>(f, my_obs, my_w, koff, act, bias, p0, r, half);
                else
                    cnn_conv_pass<1>(f, my_obs, my_w, koff, act, bias, p0, r, half);
            }
        }
        __syncthreads();  // the activation image is complete; the convolution's operands are dead
        cnn_fc_layer(act, act_ld, K2, fc1_w, fc1_b, kCnnHidden, true, chunk, h1, kCnnFcLd, wave, lane);
        cnn_fc_layer(h1, kCnnFcLd, kCnnHidden, fc2_w, fc2_b, kCnnHidden, true, chunk, h2, kCnnFcLd, wave, lane);
        cnn_fc_layer(h2, kCnnFcLd, kCnnHidden, head_w, head_b, out_dim, false, chunk, outs, 8u, wave, lane);

        // ---- the loss head, a lane per sample: d_out = dLoss / d(head output)
        if (tid < kCnnTile) {
            float d[kCnnActions] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t at = sample[tid];
            if (at != 0xFFFFFFFFu && net == 0u) {
                const float lg[kCnnActions] = {outs[tid * 8u], outs[tid * 8u + 1], outs[tid * 8u + 2], outs[tid * 8u + 3], outs[tid * 8u + 4],
                                               outs[tid * 8u + 5]};
                mappo_actor_sample<(int)kCnnActions>(lg, a.actions[at], a.logprobs[at], a.advantages[at], a.loss, count, d, stat);
            } else if (at != 0xFFFFFFFFu) {
                d[0] = mappo_critic_sample(outs[tid * 8u], a.value_preds[at], a.returns[at], a.row_norm, a.loss, count, stat);
            }
#pragma unroll
            for (int i = 0; i < (int)kCnnActions; i++) d_out[tid * 8u + i] = d[i];
            d_out[tid * 8u + 6] = d_out[tid * 8u + 7] = 0.0f;
        }
        __syncthreads();

        // ---- head: dW_head = d_out^T h2 (rows: outputs, k: samples) on waves 0 and 1, a 32-column slab each; db_head; d_h2
        if (wave < 2u) {
            const uint32_t col = 32u * wave + r;
            f32x16 acc = acc_load(g_head_w, kCnnHidden, out_dim, col, true, first, half);
#pragma unroll 4
            for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                const uint32_t s = 2u * kk + half;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(r < out_dim ? d_out[s * 8u + r] : 0.0f, h2[s * kCnnFcLd + col], acc, 0, 0, 0);
            }
            acc_store(g_head_w, kCnnHidden, out_dim, col, true, half, acc);
        } else if (wave == 2u && lane < out_dim) {
            float sum = first ? 0.0f : g_head_b[lane];
            for (uint32_t s = 0; s < kCnnTile; s++) sum += d_out[s * 8u + lane];
            g_head_b[lane] = sum;
        }
        for (uint32_t idx = tid; idx < kCnnTile * kCnnHidden; idx += kCnnThreads) {
            const uint32_t s = idx >> 6, j = idx & 63u;
            float sum = 0.0f;
            for (uint32_t o = 0; o < out_dim; o++) sum = fmaf(head_w[o * kCnnHidden + j], d_out[s * 8u + o], sum);
            d_h2[s * kCnnFcLd + j] = h2[s * kCnnFcLd + j] > 0.0f ? sum : 0.0f;
        }
        __syncthreads();

        // ---- fc2: dW_fc2 = d_h2^T h1, one 32 x 32 block per wave, k = samples
        {
            const uint32_t jt = wave >> 1, it = wave & 1u, col = 32u * it + r;
            float *__restrict__ g = g_fc2_w + (size_t)32u * jt * kCnnHidden;
            f32x16 acc = acc_load(g, kCnnHidden, 32u, col, true, first, half);
#pragma unroll 4
            for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                const uint32_t s = 2u * kk + half;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h2[s * kCnnFcLd + 32u * jt + r], h1[s * kCnnFcLd + col], acc, 0, 0, 0);
            }
            acc_store(g, kCnnHidden, 32u, col, true, half, acc);
        }
        // d_h1[sample][i] = (h1 > 0) sum_j d_h2[sample][j] W_fc2[j][i]: rows samples, k = units of fc2; waves 0 and 1
        if (wave < 2u) {
            const uint32_t col = 32u * wave + r;
            f32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 4
            for (uint32_t kk = 0; kk < kCnnHidden / 2u; kk++) {
                const uint32_t j = 2u * kk + half;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h2[r * kCnnFcLd + j], fc2_w[j * kCnnHidden + col], acc, 0, 0, 0);
            }
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const uint32_t row = tile_row(e, half);
                d_h1[row * kCnnFcLd + col] = h1[row * kCnnFcLd + col] > 0.0f ? acc[e] : 0.0f;
            }
        } else if (wave == 2u) {
            float sum = first ? 0.0f : g_fc2_b[lane];
            for (uint32_t s = 0; s < kCnnTile; s++) sum += d_h2[s * kCnnFcLd + lane];
            g_fc2_b[lane] = sum;
        }
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
        if (wave == 3u) {
            float sum = first ? 0.0f : g_fc1_b[lane];
            for (uint32_t s = 0; s < kCnnTile; s++) sum += d_h1[s * kCnnFcLd + lane];
            g_fc1_b[lane] = sum;
        }
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
        load_rows(a, lds, sample, shifts, conv_w, false);
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

    // ---- the stats' sums: lanes in ascending order
    const uint32_t tid = tid0;
    double *sums = reinterpret_cast<double *>(lds);
    if (tid < kCnnTile) {
#pragma unroll
        for (int c = 0; c < 4; c++) sums[c * kCnnTile + tid] = stat[c];
    }
    __syncthreads();
    if (tid < kMappoStats) {
        double sum = 0.0;
        if (tid < 4u)
            for (uint32_t s = 0; s < kCnnTile; s++) sum += sums[tid * kCnnTile + s];
        a.partial_stats[((size_t)net * a.groups + blockIdx.x) * kMappoStats + tid] = sum;
    }
}

// ValueNorm, first launch: the mean and the mean of squares of every row's gathered returns, one workgroup per row
__global__ void __launch_bounds__(kStatThreads) mrl_mappo_row_sums(const float *__restrict__ returns, const int32_t *__restrict__ indices,
                                                                  uint32_t minibatch_size, uint32_t batch_size, float *__restrict__ row_sums)
{
    __shared__ double scratch[kStatThreads];
    const int32_t *row = indices + (size_t)blockIdx.x * minibatch_size;
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

// ValueNorm, second launch: utils/valuenorm.py's update and running_mean_var over the K rows, one thread, float32 as torch's
__global__ void mrl_mappo_value_norm(const float *__restrict__ row_sums, uint32_t rows, float beta, float one_minus_beta, float epsilon,
                                     float *__restrict__ state, float *__restrict__ row_norm)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
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
                             hipStream_t stream)
{
    hipLaunchKernelGGL(mrl_mappo_row_sums, dim3(num_minibatches), dim3(kStatThreads), 0, stream, returns, indices, minibatch_size, batch_size,
                       row_sums);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(mrl_mappo_value_norm, dim3(1), dim3(64), 0, stream, row_sums, num_minibatches, cfg.valuenorm_beta,
                       cfg.valuenorm_one_minus_beta, cfg.valuenorm_epsilon, state, row_norm);
    MRL_HIP(hipGetLastError());
}

void launch_mappo_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_batch &batch,
                         const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                         float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    const uint32_t W = policy.width, H = policy.height, F = policy.channels;
    const uint32_t actor = (uint32_t)cnn_net_params(W, H, F, kCnnActions), critic = (uint32_t)cnn_net_params(W, H, F, 1);
    const SampleShare share = share_samples(minibatch_size, kCnnTile, kMappoMaxGroups);
    const MappoWorkspace ws = mappo_workspace(actor, minibatch_size, num_minibatches);
    const CnnUpdateLds lds = cnn_update_lds(W, H, F);
    const bool norm = cfg.flags & MRL_MAPPO_VALUENORM;
    if (norm)
        launch_mappo_value_norm(batch.returns, indices, num_minibatches, minibatch_size, batch.size, cfg, value_norm_state,
                                workspace + ws.row_sums, workspace + ws.row_norm, stream);
    allow_large_dynamic_lds<&mrl_mappo_grad>(lds.total);
    MappoGradArgs g{};
    g.fwd.params = opt.params_dev;
    g.fwd.W = W;
    g.fwd.H = H;
    g.fwd.F = F;
    g.fwd.lds = lds.fwd;
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
    g.minibatch_size = minibatch_size;
    g.batch_size = batch.size;
    g.groups = share.groups;
    g.tail_at = lds.tail_at;
    g.loss = MappoLoss{cfg.clip_param, cfg.entropy_coef, cfg.value_loss_coef, cfg.huber_delta, cfg.flags};
    // two clip_grad_norm_ and two Adam steps: the actor's segment, then the critic's
    AdamStepArgs ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.opti_eps, cfg.flags & MRL_MAPPO_MAX_GRAD_NORM, cfg.max_grad_norm);
    ad.partial_grads = g.partial_grads;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = ws.stride;
    ad.segments = 2;
    ad.groups = share.groups;
    ad.blocks = (uint32_t)ws.blocks;
    ad.num_params[0] = actor, ad.num_params[1] = critic;
    ad.at[0] = 0, ad.at[1] = actor;
    MappoStatsRow row{g.partial_stats, nullptr, share.groups, minibatch_size};
    for (uint32_t k = 0; k < num_minibatches; k++) {
        g.indices = indices + (size_t)k * minibatch_size;
        g.row_norm = norm ? workspace + ws.row_norm + 2 * (size_t)k : nullptr;
        hipLaunchKernelGGL(mrl_mappo_grad, dim3(share.groups, 2), dim3(kCnnThreads), lds.total, stream, g);
        MRL_HIP(hipGetLastError());
        ad.grads_row = grads ? grads + (size_t)k * ((size_t)actor + critic) : nullptr;
        adam_set_step(ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.critic_lr});
        row.row = stats ? stats + (size_t)k * kMappoStats : nullptr;
        launch_adam_step(ad, row, stream);
    }
}

}  // namespace mrl
