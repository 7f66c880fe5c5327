// mrl_mappo_mlp_update with MRL_MLPBASE_H512: MAPPO's update for the MLPBase actor-critic at hidden_size 512 without torch in the
// loop (include/mrl_envs.h; the slabs, the workspace and the order of every sum are in
// mlpbase_h512_update.hpp).
//
// A row is cut into slabs of at most kMlpH512Slab samples.  Per slab, for both nets at once (the net is a grid dimension):
//   mrl_mlp512_forward   the act's computation (mlpbase_h512_forward.hpp: the same chains, hence the same bits) on the samples the
//                        index list names, a workgroup of four waves per tile of 32; per hidden layer it stores the post-ReLU row z,
//                        LayerNorm's (mean, rstd) and its output y, and LayerNorm(7)'s input, output and statistics and the head's
//                        outputs.  A row past the slab's end is a zero observation.
//   mrl_mlp512_loss      a lane per sample (mappo_loss.hpp): dL/d(head output) and the stats' double sums per tile.
//   mrl_mlp512_backward  one launch per hidden layer l = layer_N .. 0, a workgroup per tile of 32 rows and all 512 columns:
//                        (a) dy = d_pre_{l+1} W_{l+1}, k = 512 on v_mfma_f32_32x32x2_f32.  d_pre_{l+1}'s tile lies in LDS (rows of 513:
//                            lane r reads bank r + k); W is streamed from L2 straight into the B operand -- the transposed access of
//                            the act: wave w owns the column blocks 4 w .. 4 w + 3, lane (r, half) column r of each and reads W[j][c]
//                            for j = half, half + 2, ..., so the 32 lanes of a half read 32 adjacent floats; the 16 loads of the
//                            next 8 j are issued before the products of the current 8.  The 64 accumulator registers wait until
//                            every wave has read the tile, then dy replaces it.  Below the head dy = d_out W_head, plain fmaf.
//                        (c) the tile's dgamma = sum dy xhat and dbeta = sum dy, a lane per column in ascending row order, one
//                            vector per tile.
//                        (b) LayerNorm backward in place, a wavefront per row, a lane eight columns 64 apart (no bank conflict),
//                            with the stored mean and rstd, the ReLU gate z > 0, and d_pre_l stored.
//                        For l = 0 it then forms d_in0 = d_pre_0 W_fc1 from the tile in LDS.
//   launch_h512_dw       dW_head = d_out^T y_top and dW_l = d_pre_l^T y_{l-1} with their biases (mrl_h512_dw, cnn_h512_update.hip:
//                        128 x 128 tiles, eight shares, both operands staged through LDS).
//   mrl_mlp512_small     dW_fc1, db_fc1 and feature_norm's dgamma and dbeta: a thread per output, one chain per share.
//   mrl_mlp512_fold      the shares' sums in ascending q, the tiles' LayerNorm vectors in ascending tile order, zeros for fc_h, onto
//                        the running gradient; the tiles' stats onto the running stats.
// Per row the optimiser tail (adam_step.hpp) then runs on the one running vector per net.  Tiles are 32 rows at every size: the
// 64-row form of the act (two row blocks behind one read of the weights) would need 128 accumulator registers beside the 32 of
// the double-buffered operand, and the update's time is in the weight gradients, not here.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "mlpbase_h512_update.hpp"
#include "mlpbase_h512_forward.hpp"
#include "mappo_grad.hpp"

namespace mrl {

namespace {

constexpr uint32_t kH = kMlpH512Hidden, kTile = kMlpH512Tile;
static_assert(kMlpH512Slab % 64u == 0 && kTile == kMappoTile && kMlpH512Threads == kMappoThreads, "whole tiles; mappo_grad.hpp's tile and workgroup");
static_assert(kMlpH512Threads == 8u * kTile, "a thread per (row, observation column) of a tile");

extern __shared__ __attribute__((aligned(16))) unsigned char mlp512_upd_lds_image[];

// where hidden layer l's tensors start in a net's vector: Linear weight, bias, LayerNorm weight, LayerNorm bias
__host__ __device__ constexpr uint32_t layer_bias_at(uint32_t l) { return mlpbase_h512_layer_at(l) + kH * (l ? kH : kMlpBaseObs); }

// ---------------------------------------------------------------- the forward pass, storing activations

struct Mlp512ForwardArgs {
    const float *params;
    const int32_t *obs;      // the batch's rows (S, 7)
    const int32_t *indices;  // the slab's sample numbers
    float *in0, *y0, *stat0, *z, *y, *stat, *out;
    uint32_t count, batch_size, rows, layer_N;  // the slab's samples, S, the workspace's rows per net
};

// rows of 513 in LDS to (or from) rows of 512 in global memory, the tile's 32
__device__ __forceinline__ void tile_to_global(float *__restrict__ dst, const float *h, uint32_t tid)
{
    for (uint32_t e = tid; e < kTile * kH; e += kMlpH512Threads) dst[e] = h[(e >> 9) * kMlpH512Ld + (e & 511u)];
}

// mrl_mlpbase_act_h512's body (mlpbase_h512.hip, RB = 1) on gathered samples, every layer's row, statistics and output stored
__global__ void __launch_bounds__(kMlpH512Threads) mrl_mlp512_forward(Mlp512ForwardArgs g)
{
    const uint32_t net = blockIdx.y, layers = g.layer_N + 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const bool odd = half != 0u;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = g.params + (net ? mlpbase_h512_net_params(g.layer_N, kMlpBaseActions) : 0u);
    float *h = reinterpret_cast<float *>(mlp512_upd_lds_image);
    float *in0 = h + mlpbase_h512_in0_at(kTile), *outs = h + mlpbase_h512_out_at(kTile), *stats = h + kMlpH512FwdStatAt;
    const uint32_t tile0 = blockIdx.x * kTile;
    const size_t row0 = (size_t)net * g.rows + tile0;  // the tile's first row of the net's narrow arrays
    const uint32_t rr = tid >> 3, k = tid & 7u;

    {
        float v = 0.0f;
        if (tile0 + rr < g.count && k < kMlpBaseObs) {
            uint32_t s = (uint32_t)g.indices[tile0 + rr];
            s = s < g.batch_size ? s : g.batch_size - 1u;  // outside the contract, but memory-safe
            v = (float)g.obs[(size_t)s * kMlpBaseObs + k];
        }
        in0[rr * kMlpLd0 + k] = v;
        g.in0[(row0 + rr) * 8u + k] = v;
    }
    __syncthreads();
    mlp512_layer_norm<1, true>(in0, kMlpLd0, kTile, kMlpBaseObs, params, params + kMlpBaseObs, wave, lane, stats);
    g.y0[(row0 + rr) * 8u + k] = in0[rr * kMlpLd0 + k];
    if (tid < 2u * kTile) g.stat0[row0 * 2u + tid] = stats[tid];

    f32x16 acc[1][4];
    const float *a_row = h + r * kMlpH512Ld + half;
    for (uint32_t layer = 0; layer < layers; layer++) {
        const float *__restrict__ w = params + mlpbase_h512_layer_at(layer);
        const float *__restrict__ bias = params + layer_bias_at(layer);
        const size_t wide0 = ((size_t)(net * layers + layer) * g.rows + tile0);  // the tile's first row of the layer's wide arrays
        if (layer == 0) {
            mlp512_fc1<1>(in0, w, wave, r, half, acc);
        } else {
            const float *w_row[4];
#pragma unroll
            for (int j = 0; j < 4; j++) w_row[j] = w + (size_t)((wave * 4u + j) * 32u + r) * kH;
            mlp512_products<1>(a_row, w_row, odd, acc);
            __syncthreads();  // every wave has read the previous h: this layer's replaces it
        }
        mlp512_store<1>(acc, bias, h, wave, r, half);
        __syncthreads();
        tile_to_global(g.z + wide0 * kH, h, tid);
        __syncthreads();  // LayerNorm runs in place over what the loop above read
        mlp512_layer_norm<8, true>(h, kMlpH512Ld, kTile, kH, bias + kH, bias + 2u * kH, wave, lane, stats);
        tile_to_global(g.y + wide0 * kH, h, tid);
        if (tid < 2u * kTile) g.stat[wide0 * 2u + tid] = stats[tid];
    }

    if (wave == 0u) {
        // the head: one column block whose columns out_dim .. 31 read row 0 again; columns out_dim .. 7 are stored as zeros
        const float *__restrict__ head_w = params + mlpbase_h512_head_at(g.layer_N), *__restrict__ head_b = head_w + out_dim * kH;
        f32x16 out[1];
        const float *head_row[1] = {head_w + (size_t)(r < out_dim ? r : 0u) * kH};
#pragma unroll
        for (int e = 0; e < 16; e++) out[0][e] = 0.0f;
        h512_products<1>(a_row, kH, head_row, odd, out);
        if (r < 8u) {
            const float bias = r < out_dim ? head_b[r] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; e++) outs[tile_row(e, half) * 8u + r] = r < out_dim ? out[0][e] + bias : 0.0f;
        }
    }
    __syncthreads();
    g.out[row0 * 8u + tid] = outs[tid];
}

// ---------------------------------------------------------------- the loss head

struct Mlp512LossArgs {
    MappoGradCommon common;  // indices: the slab's; groups: the slab's tiles; partial_stats: (2, tiles, 8)
    const float *out;
    float *d_out;
    uint32_t count, rows;
};

__global__ void __launch_bounds__(kMappoThreads) mrl_mlp512_loss(Mlp512LossArgs g)
{
    __shared__ uint32_t sample[kMappoTile];
    __shared__ float d_out[kMappoTile * 8u];
    __shared__ double sums[4 * kMappoTile];
    const MappoGradCommon &c = g.common;
    const uint32_t net = blockIdx.y, tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kMappoTile;
    const size_t row0 = (size_t)net * g.rows + base;
    mappo_tile_samples(c, sample, base, g.count, tid);
    __syncthreads();
    double stat[4] = {0.0, 0.0, 0.0, 0.0};
    mappo_loss_head<(int)kMlpBaseActions>(c, net, sample, g.out + row0 * 8u, d_out, (float)c.minibatch_size, stat, tid);
    __syncthreads();
    g.d_out[row0 * 8u + tid] = d_out[tid];
    mappo_stats_tail(c, net, sums, stat, tid);
}

// ---------------------------------------------------------------- the backward pass through a hidden layer

struct Mlp512BackwardArgs {
    const float *params;
    const float *z, *stat, *d_out;  // (2, L, rows, 512), (2, L, rows, 2), (2, rows, 8)
    float *d_pre, *ln, *d_in0;      // (2, L, rows, 512), (2, L, rows / 32, 1024), (2, rows, 8)
    uint32_t rows, layer_N, layer;
};

// 8 consecutive j of W from j0 on (this lane's half: j0, j0 + 2, j0 + 4, j0 + 6) for the lane's column of each of its four blocks;
// w_col[b] points at W[half][column]
__device__ __forceinline__ void mlp512_fetch_t(const float *const (&w_col)[4], uint32_t j0, float (&b)[4][4])
{
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
        for (int blk = 0; blk < 4; blk++) b[blk][s] = w_col[blk][(size_t)(j0 + 2u * s) * kH];
}

// the products of those 8 j: four matrix instructions per column block, j ascending.  a_row: this lane's LDS row from its own first j
__device__ __forceinline__ void mlp512_multiply_t(const float *__restrict__ a_row, uint32_t j0, const float (&b)[4][4], f32x16 (&acc)[4])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const float av = a_row[j0 + 2u * s];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) acc[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b[blk][s], acc[blk], 0, 0, 0);
    }
}

// TOP: the layer below the head (dy = d_out W_head); else dy = d_pre_{layer + 1} W_{layer + 1}
template <bool TOP>
__global__ void __launch_bounds__(kMlpH512Threads) mrl_mlp512_backward(Mlp512BackwardArgs g)
{
    const uint32_t net = blockIdx.y, layers = g.layer_N + 1u, layer = g.layer;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = g.params + (net ? mlpbase_h512_net_params(g.layer_N, kMlpBaseActions) : 0u);
    float *h = reinterpret_cast<float *>(mlp512_upd_lds_image);
    float *stat = h + kMlpH512BwdStatAt, *d_out = h + kMlpH512BwdDoutAt;
    const uint32_t tile0 = blockIdx.x * kTile;
    const size_t row0 = (size_t)net * g.rows + tile0;
    const size_t wide0 = (size_t)(net * layers + layer) * g.rows + tile0;
    const float *__restrict__ z = g.z + wide0 * kH;

    if (tid < 2u * kTile) stat[tid] = g.stat[wide0 * 2u + tid];
    if (TOP) {
        d_out[tid] = g.d_out[row0 * 8u + tid];
        __syncthreads();
        const float *__restrict__ head_w = params + mlpbase_h512_head_at(g.layer_N);
        for (uint32_t idx = tid; idx < kTile * kH; idx += kMlpH512Threads) {
            const uint32_t s = idx >> 9, c = idx & 511u;
            float sum = 0.0f;
            for (uint32_t o = 0; o < out_dim; o++) sum = fmaf(head_w[o * kH + c], d_out[s * 8u + o], sum);
            h[s * kMlpH512Ld + c] = sum;
        }
    } else {
        // (a) the tile of d_pre_{layer + 1} into LDS, then its product with W_{layer + 1} (512 x 512, row j the output unit)
        const float *__restrict__ above = g.d_pre + (wide0 + g.rows) * kH;
        for (uint32_t e = tid; e < kTile * kH; e += kMlpH512Threads) h[(e >> 9) * kMlpH512Ld + (e & 511u)] = above[e];
        __syncthreads();
        const float *__restrict__ w = params + mlpbase_h512_layer_at(layer + 1u);
        const float *w_col[4];
#pragma unroll
        for (int blk = 0; blk < 4; blk++) w_col[blk] = w + (size_t)half * kH + (wave * 4u + blk) * 32u + r;
        f32x16 acc[4];
#pragma unroll
        for (int blk = 0; blk < 4; blk++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[blk][e] = 0.0f;
        const float *a_row = h + r * kMlpH512Ld + half;
        float b0[4][4], b1[4][4];
        mlp512_fetch_t(w_col, 0u, b0);
        for (uint32_t j = 0; j < kH; j += 16u) {
            mlp512_fetch_t(w_col, j + 8u, b1);
            mlp512_multiply_t(a_row, j, b0, acc);
            if (j + 16u < kH) mlp512_fetch_t(w_col, j + 16u, b0);
            mlp512_multiply_t(a_row, j + 8u, b1, acc);
        }
        __syncthreads();  // every wave has read d_pre_{layer + 1}: dy replaces it
#pragma unroll
        for (int blk = 0; blk < 4; blk++) {
            const uint32_t col = (wave * 4u + blk) * 32u + r;
#pragma unroll
            for (int e = 0; e < 16; e++) h[tile_row(e, half) * kMlpH512Ld + col] = acc[blk][e];
        }
    }
    __syncthreads();

    // (c) the tile's LayerNorm parameter gradients, a lane per column, rows ascending
    {
        float *__restrict__ ln = g.ln + ((size_t)(net * layers + layer) * (g.rows / kTile) + blockIdx.x) * 2u * kH;
        for (uint32_t col = tid; col < kH; col += kMlpH512Threads) {
            float d_gamma = 0.0f, d_beta = 0.0f;
            for (uint32_t row = 0; row < kTile; row++) {
                const float dy = h[row * kMlpH512Ld + col];
                const float xhat = (z[row * kH + col] - stat[2u * row]) * stat[2u * row + 1u];
                d_gamma += dy * xhat;
                d_beta += dy;
            }
            ln[col] = d_gamma, ln[kH + col] = d_beta;
        }
    }
    __syncthreads();

    // (b) LayerNorm backward and the ReLU gate in place, a wavefront per row; d_pre_layer is stored
    {
        const float *__restrict__ gamma = params + layer_bias_at(layer) + kH;
        float *__restrict__ d_pre = g.d_pre + wide0 * kH;
        float weight[8];
#pragma unroll
        for (int j = 0; j < 8; j++) weight[j] = gamma[lane + 64u * j];
        for (uint32_t row = wave; row < kTile; row += 4u) {
            const float mean = stat[2u * row], rstd = stat[2u * row + 1u];
            float xhat[8], grad[8], sum_g = 0.0f, sum_gx = 0.0f;
            bool pass[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t col = lane + 64u * j;
                const float zv = z[row * kH + col];
                pass[j] = zv > 0.0f;
                xhat[j] = (zv - mean) * rstd;
                grad[j] = h[row * kMlpH512Ld + col] * weight[j];
                sum_g += grad[j];
                sum_gx += grad[j] * xhat[j];
            }
            const float mean_g = wave_sum(sum_g) / (float)kH, mean_gx = wave_sum(sum_gx) / (float)kH;
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const uint32_t col = lane + 64u * j;
                const float dz = pass[j] ? rstd * ((grad[j] - mean_g) - xhat[j] * mean_gx) : 0.0f;
                h[row * kMlpH512Ld + col] = dz;
                d_pre[row * kH + col] = dz;
            }
        }
    }
    if (layer != 0u) return;
    __syncthreads();

    // below fc1: d_in0[row][i] = sum over j of W_fc1[j][i] d_pre_0[row][j], thread (row, i)
    {
        const float *__restrict__ w = params + kMlpH512Fc1At;
        const uint32_t row = tid >> 3, i = tid & 7u;
        float sum = 0.0f;
        if (i < kMlpBaseObs)
            for (uint32_t j = 0; j < kH; j++) sum = fmaf(w[j * kMlpBaseObs + i], h[row * kMlpH512Ld + j], sum);
        g.d_in0[(row0 + row) * 8u + i] = sum;
    }
}

// ---------------------------------------------------------------- fc1's and feature_norm's gradients

struct Mlp512SmallArgs {
    const float *d_pre0, *y0, *in0, *stat0, *d_in0;  // net 0's; d_pre0 is layer 0 of (2, L, rows, 512)
    float *partial;                                   // (2, kH512Shares, stride)
    uint64_t wide_net, stride;                        // floats from net 0's d_pre0 to net 1's
    uint32_t rows, nrows, share;
};

constexpr uint32_t kSmallW = kH * kMlpBaseObs, kSmallOutputs = kSmallW + kH + 2u * kMlpBaseObs;

// thread o of (blockIdx.x, share blockIdx.y, net blockIdx.z): one output, ONE chain over the share's samples in ascending order
__global__ void __launch_bounds__(kAdamThreads) mrl_mlp512_small(Mlp512SmallArgs g)
{
    const uint32_t o = blockIdx.x * kAdamThreads + threadIdx.x, q = blockIdx.y, net = blockIdx.z;
    if (o >= kSmallOutputs) return;
    const uint32_t begin = q * g.share, end = begin + g.share < g.nrows ? begin + g.share : g.nrows;
    const float *__restrict__ d_pre0 = g.d_pre0 + net * g.wide_net;
    const size_t narrow = (size_t)net * g.rows;
    const float *__restrict__ y0 = g.y0 + narrow * 8u, *__restrict__ in0 = g.in0 + narrow * 8u, *__restrict__ d_in0 = g.d_in0 + narrow * 8u;
    const float *__restrict__ stat0 = g.stat0 + narrow * 2u;
    float *__restrict__ out = g.partial + ((size_t)net * kH512Shares + q) * g.stride;
    float sum = 0.0f;
    if (o < kSmallW) {  // dW_fc1[j][i] = sum d_pre_0[s][j] y0[s][i]
        const uint32_t j = o / kMlpBaseObs, i = o - j * kMlpBaseObs;
        for (uint32_t s = begin; s < end; s++) sum = fmaf(d_pre0[(size_t)s * kH + j], y0[s * 8u + i], sum);
        out[kMlpH512Fc1At + o] = sum;
    } else if (o < kSmallW + kH) {  // db_fc1[j] = sum d_pre_0[s][j]
        const uint32_t j = o - kSmallW;
        for (uint32_t s = begin; s < end; s++) sum += d_pre0[(size_t)s * kH + j];
        out[kMlpH512Fc1At + o] = sum;
    } else if (o < kSmallW + kH + kMlpBaseObs) {  // feature_norm's dgamma[i] = sum d_in0[s][i] xhat0[s][i]
        const uint32_t i = o - kSmallW - kH;
        for (uint32_t s = begin; s < end; s++) sum = fmaf(d_in0[s * 8u + i], (in0[s * 8u + i] - stat0[2u * s]) * stat0[2u * s + 1u], sum);
        out[i] = sum;
    } else {  // feature_norm's dbeta[i] = sum d_in0[s][i]
        const uint32_t i = o - kSmallW - kH - kMlpBaseObs;
        for (uint32_t s = begin; s < end; s++) sum += d_in0[s * 8u + i];
        out[kMlpBaseObs + i] = sum;
    }
}

// ---------------------------------------------------------------- the slab's sums onto the running gradient

struct Mlp512FoldArgs {
    const float *partial, *ln;  // (2, kH512Shares, stride), (2, L, rows / 32, 1024)
    float *run;                 // (2, stride)
    const double *slab_stats;   // (2, tiles, 8)
    double *run_stats;          // (2, 8)
    uint64_t stride;
    uint32_t num_params[2], layers, ln_tiles, tiles, first;  // ln_tiles: the workspace's rows / 32; tiles: the slab's
};

__global__ void __launch_bounds__(kAdamThreads) mrl_mlp512_fold(Mlp512FoldArgs g)
{
    const uint32_t net = blockIdx.y, p = blockIdx.x * kAdamThreads + threadIdx.x;
    if (p < g.num_params[net]) {
        float sum = 0.0f;
        bool shares = p < kMlpH512FcHAt || p >= kMlpH512FcHAt + kMlpH512Block;  // fc_h: no forward pass reads it, its gradient is zero
        for (uint32_t l = 0; l < g.layers; l++) {
            const uint32_t at = layer_bias_at(l) + kH;  // the layer's LayerNorm weight, then its bias
            if (p >= at && p < at + 2u * kH) {
                const float *__restrict__ ln = g.ln + (size_t)(net * g.layers + l) * g.ln_tiles * 2u * kH + (p - at);
                for (uint32_t t = 0; t < g.tiles; t++) sum += ln[(size_t)t * 2u * kH];
                shares = false;
            }
        }
        if (shares)
            for (uint32_t q = 0; q < kH512Shares; q++) sum += g.partial[((size_t)net * kH512Shares + q) * g.stride + p];
        float *run = g.run + (size_t)net * g.stride + p;
        *run = g.first ? sum : *run + sum;
    }
    if (blockIdx.x == 0 && threadIdx.x < kMappoStats) {
        double sum = 0.0;
        for (uint32_t t = 0; t < g.tiles; t++) sum += g.slab_stats[((size_t)net * g.tiles + t) * kMappoStats + threadIdx.x];
        double *run = g.run_stats + net * kMappoStats + threadIdx.x;
        *run = g.first ? sum : *run + sum;
    }
}

}  // namespace

void launch_mappo_mlp_h512_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_batch &batch, const int32_t *indices,
                                  uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                                  float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    const MlpH512Workspace ws = mlp_h512_workspace(layer_N, minibatch_size, num_minibatches);
    const uint32_t actor = mlpbase_h512_net_params(layer_N, kMlpBaseActions), critic = mlpbase_h512_net_params(layer_N, 1);
    const uint32_t rows = (uint32_t)ws.rows, layers = (uint32_t)ws.layers;
    const uint64_t wide_layer = (uint64_t)rows * kH, wide_net = layers * wide_layer;
    constexpr uint32_t forward_lds = kMlpH512FwdFloats * 4u, backward_lds = kMlpH512BwdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mlp512_forward>(forward_lds);
    allow_large_dynamic_lds<&mrl_mlp512_backward<true>>(backward_lds);
    allow_large_dynamic_lds<&mrl_mlp512_backward<false>>(backward_lds);
    const bool norm = cfg.flags & MRL_MAPPO_VALUENORM;
    if (norm)
        launch_mappo_value_norm(batch.returns, indices, num_minibatches, minibatch_size, batch.size, cfg, value_norm_state,
                                workspace + ws.row_sums, workspace + ws.row_norm, stream);
    float *z = workspace + ws.z, *y = workspace + ws.y, *d_pre = workspace + ws.d_pre, *partial = workspace + ws.partial;
    float *out = workspace + ws.out, *d_out = workspace + ws.d_out, *run = workspace + ws.run;
    double *slab_stats = reinterpret_cast<double *>(workspace + ws.slab_stats), *run_stats = reinterpret_cast<double *>(workspace + ws.run_stats);

    Mlp512ForwardArgs fw{};
    fw.params = opt.params_dev;
    fw.obs = static_cast<const int32_t *>(batch.obs);
    fw.in0 = workspace + ws.in0, fw.y0 = workspace + ws.y0, fw.stat0 = workspace + ws.stat0;
    fw.z = z, fw.y = y, fw.stat = workspace + ws.stat, fw.out = out;
    fw.batch_size = batch.size, fw.rows = rows, fw.layer_N = layer_N;

    Mlp512LossArgs ls{};
    MappoGradCommon &c = ls.common;
    c.actions = batch.actions, c.logprobs = batch.logprobs, c.value_preds = batch.value_preds;
    c.returns = batch.returns, c.advantages = batch.advantages;
    c.partial_stats = slab_stats;
    c.minibatch_size = minibatch_size, c.batch_size = batch.size;
    c.loss = MappoLoss{cfg.clip_param, cfg.entropy_coef, cfg.value_loss_coef, cfg.huber_delta, cfg.flags};
    ls.out = out, ls.d_out = d_out, ls.rows = rows;

    Mlp512BackwardArgs bw{};
    bw.params = opt.params_dev;
    bw.z = z, bw.stat = workspace + ws.stat, bw.d_out = d_out;
    bw.d_pre = d_pre, bw.ln = workspace + ws.ln, bw.d_in0 = workspace + ws.d_in0;
    bw.rows = rows, bw.layer_N = layer_N;

    // the head's weight gradient and those of fc2[l - 1], l = 1 .. layer_N; the operands of a slab are set below
    H512DwArgs head{}, fc2[kMlpBaseMaxLayerN]{};
    head.partial = partial, head.stride = ws.stride;
    head.a = d_out, head.b = y + layer_N * wide_layer, head.a_net = (uint64_t)rows * 8, head.b_net = wide_net;
    head.lda = 8, head.ldb = kH, head.a_cols = 8, head.m[0] = kMlpBaseActions, head.m[1] = 1, head.n = kH;
    head.w_at = mlpbase_h512_head_at(layer_N);
    head.bias_at[0] = head.w_at + kMlpBaseActions * kH, head.bias_at[1] = head.w_at + kH;
    for (uint32_t l = 1; l <= layer_N; l++) {
        H512DwArgs &dw = fc2[l - 1];
        dw.partial = partial, dw.stride = ws.stride;
        dw.a = d_pre + l * wide_layer, dw.b = y + (l - 1) * wide_layer, dw.a_net = dw.b_net = wide_net;
        dw.lda = dw.ldb = dw.a_cols = dw.m[0] = dw.m[1] = dw.n = kH;
        dw.w_at = mlpbase_h512_layer_at(l), dw.bias_at[0] = dw.bias_at[1] = layer_bias_at(l);
    }

    Mlp512SmallArgs sm{};
    sm.d_pre0 = d_pre, sm.y0 = fw.y0, sm.in0 = fw.in0, sm.stat0 = fw.stat0, sm.d_in0 = bw.d_in0;
    sm.partial = partial, sm.wide_net = wide_net, sm.stride = ws.stride, sm.rows = rows;

    Mlp512FoldArgs fold{partial, bw.ln, run, slab_stats, run_stats, ws.stride, {actor, critic}, layers, rows / kTile, 0, 0};

    AdamStepArgs ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.opti_eps, cfg.flags & MRL_MAPPO_MAX_GRAD_NORM, cfg.max_grad_norm);
    ad.partial_grads = run;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = ws.stride;
    ad.segments = 2;
    ad.groups = 1;
    ad.blocks = (uint32_t)ws.blocks;
    ad.num_params[0] = actor, ad.num_params[1] = critic;
    ad.at[0] = 0, ad.at[1] = actor;
    MappoStatsRow row{run_stats, nullptr, 1, minibatch_size};

    const dim3 threads(kMlpH512Threads);
    for (uint32_t k = 0; k < num_minibatches; k++) {
        const int32_t *row_indices = indices + (size_t)k * minibatch_size;
        c.row_norm = norm ? workspace + ws.row_norm + 2 * (size_t)k : nullptr;
        for (uint64_t s0 = 0; s0 < minibatch_size; s0 += kMlpH512Slab) {
            const uint32_t count = (uint32_t)(minibatch_size - s0 < kMlpH512Slab ? minibatch_size - s0 : kMlpH512Slab);
            const uint32_t tiles = (count + kTile - 1) / kTile, nrows = tiles * kTile;
            const uint32_t share = (tiles + kH512Shares - 1) / kH512Shares * kTile;
            fw.indices = c.indices = row_indices + s0;
            fw.count = ls.count = count;
            c.groups = fold.tiles = tiles;
            hipLaunchKernelGGL(mrl_mlp512_forward, dim3(tiles, 2), threads, forward_lds, stream, fw);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_mlp512_loss, dim3(tiles, 2), threads, 0, stream, ls);
            MRL_HIP(hipGetLastError());
            head.nrows = nrows, head.share = share;
            launch_h512_dw(head, stream);
            for (uint32_t l = layers; l-- > 0;) {
                bw.layer = l;
                if (l == layer_N)
                    hipLaunchKernelGGL(mrl_mlp512_backward<true>, dim3(tiles, 2), threads, backward_lds, stream, bw);
                else
                    hipLaunchKernelGGL(mrl_mlp512_backward<false>, dim3(tiles, 2), threads, backward_lds, stream, bw);
                MRL_HIP(hipGetLastError());
                if (l) {
                    fc2[l - 1].nrows = nrows, fc2[l - 1].share = share;
                    launch_h512_dw(fc2[l - 1], stream);
                }
            }
            sm.nrows = nrows, sm.share = share;
            hipLaunchKernelGGL(mrl_mlp512_small, dim3((kSmallOutputs + kAdamThreads - 1) / kAdamThreads, kH512Shares, 2), dim3(kAdamThreads), 0,
                               stream, sm);
            MRL_HIP(hipGetLastError());
            fold.first = s0 == 0 ? 1u : 0u;
            hipLaunchKernelGGL(mrl_mlp512_fold, dim3((uint32_t)ws.blocks, 2), dim3(kAdamThreads), 0, stream, fold);
            MRL_HIP(hipGetLastError());
        }
        ad.grads_row = grads ? grads + (size_t)k * ((size_t)actor + critic) : nullptr;
        adam_set_step(ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.critic_lr});
        row.row = stats ? stats + (size_t)k * kMappoStats : nullptr;
        launch_adam_step(ad, row, stream);
    }
}

}  // namespace mrl
