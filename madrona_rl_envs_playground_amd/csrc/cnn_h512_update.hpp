// MAPPO's update for the CNN actor-critic at hidden_size 512 (C ABI: mrl_mappo_h512_update, mrl_mappo_h512_workspace_bytes in
// include/mrl_envs.h).  The kernels live in cnn_h512_update.hip; capi_mappo.hip validates the arguments.
//
// A net of this width has 1.1 to 3.6 million parameters, so a gradient vector per workgroup (mrl_mappo_grad, section 16) is out
// of reach.  The update is LAYERED instead: a row's index list is cut into SLABS of at most kH512Slab consecutive samples, a
// slab's activations of both nets are stored in the workspace, and every layer's gradient is a matrix product of its own launch
// over the slab (cnn_h512_update.hip lists the launches).
//
// THE ORDER OF EVERY SUM.  The forward pass is the act's (cnn_h512.hpp).  A weight gradient is a sum over samples:
//   a slab's n samples, rounded up to whole tiles of 32 (rows past n are zero rows), are cut into kH512Shares contiguous shares
//   of ceil(tiles / kH512Shares) tiles each; workgroup (output tile, q) adds share q's products as ONE chain of fused
//   multiply-adds from 0 in ascending sample order (dW_conv: tile, then position, then sample) and stores it once;
//   mrl_h512_fold adds the share sums in ascending q from 0 and adds that slab sum to the running gradient, which the first slab
//   starts (nothing needs clearing); slabs run in ascending order.  mrl_grad_reduce then reads one vector per net.
// An activation gradient is one chain over k = 0 .. 511 of the layer's outputs from 0.  The stats' terms are double sums: lanes,
// then tiles, then slabs, each ascending.  A chain of a weight gradient is at most 32 ceil(64 / 8) = 256 terms long.
#pragma once

#include "cnn_h512.hpp"
#include "mappo_loss.hpp"

namespace mrl {

constexpr uint32_t kH512Slab = 2048;    // samples per slab: a multiple of 64
constexpr uint32_t kH512Shares = 8;     // Q: shares of a slab's sample sum, hence partial vectors per net
constexpr uint32_t kH512ConvSlabs = 3;  // 32-column slabs of dW_conv's 9 F columns per wave: 9 F <= 4 * 3 * 32
constexpr uint32_t kH512ConvTail = kCnnTile * 2u * 4u;  // behind cnn_lds' image: the tile's sample numbers and row shifts

// The caller's scratch, in floats.  rows = min(kH512Slab, B rounded up to 64): one slab's rows, whatever B is beyond that.
//   row_norm, row_sums   (K, 2) each, padded to 4                       ValueNorm's recurrence, as in mappo_workspace
//   act                  (2, rows, 256 npos)   the post-ReLU conv image in torch's flatten order, then dL/d(conv pre-activation)
//   h1, h2, d_h1, d_h2   (2, rows, 512) each
//   out, d_out           (2, rows, 8) each
//   partial              (2, kH512Shares, stride)   the shares' gradient sums; stride = the actor's parameter count padded to 4
//   run, grad            (2, stride) each      the running gradient over the slabs; mrl_grad_reduce's output
//   sumsq                (2, blocks) padded to 4, blocks = ceil(stride / 256)
//   slab_stats           (2, rows / 32, 8) doubles;  run_stats (2, 8) doubles
struct H512Workspace {
    uint64_t row_norm, row_sums, act, h1, h2, d_h1, d_h2, out, d_out, partial, run, grad, sumsq, slab_stats, run_stats, total;
    uint64_t stride, blocks, rows, K2;
};

inline H512Workspace h512_workspace(uint64_t W, uint64_t H, uint64_t F, uint32_t minibatch_size, uint32_t num_minibatches)
{
    const auto pad = [](uint64_t n) { return (n + 3) & ~uint64_t(3); };
    const uint64_t whole = ((uint64_t)minibatch_size + 63) & ~uint64_t(63);
    H512Workspace w;
    w.rows = whole < kH512Slab ? whole : kH512Slab;
    w.K2 = kCnnH512Channels * (W - 2) * (H - 2);
    w.stride = pad(cnn_h512_net_params(W, H, F, kCnnActions));
    w.blocks = (w.stride + kAdamThreads - 1) / kAdamThreads;
    w.row_norm = 0;
    w.row_sums = w.row_norm + pad(2 * (uint64_t)num_minibatches);
    w.act = w.row_sums + pad(2 * (uint64_t)num_minibatches);
    w.h1 = w.act + 2 * w.rows * w.K2;
    w.h2 = w.h1 + 2 * w.rows * kCnnH512Hidden;
    w.d_h1 = w.h2 + 2 * w.rows * kCnnH512Hidden;
    w.d_h2 = w.d_h1 + 2 * w.rows * kCnnH512Hidden;
    w.out = w.d_h2 + 2 * w.rows * kCnnH512Hidden;
    w.d_out = w.out + 2 * w.rows * 8;
    w.partial = w.d_out + 2 * w.rows * 8;
    w.run = w.partial + 2 * kH512Shares * w.stride;
    w.grad = w.run + 2 * w.stride;
    w.sumsq = w.grad + 2 * w.stride;
    w.slab_stats = w.sumsq + pad(2 * w.blocks);
    w.run_stats = w.slab_stats + 2 * (w.rows / kCnnTile) * kMappoStats * 2;
    w.total = w.run_stats + 2 * kMappoStats * 2;
    return w;
}

// the larger of the forward pass's LDS image (the act's) and dW_conv's (cnn_lds' and the tile's tables)
inline uint32_t h512_update_lds(uint32_t W, uint32_t H, uint32_t F)
{
    const uint32_t forward = cnn_h512_lds(W, H, F).total, conv = cnn_lds(W, H, F).total + kH512ConvTail;
    return forward > conv ? forward : conv;
}

// A weight gradient C = A^T B of a linear layer with k = a slab's samples, and db as the same product against ones
// (mrl_h512_dw in cnn_h512_update.hip): the sum order above.  The hidden-512 MLPBase update (mlpbase_h512_update.hip) launches it
// for its own layers.
struct H512DwArgs {
    const float *a, *b;  // net 0's A (nrows x lda: dL/d(pre-activation)) and B (nrows x ldb: the layer's input)
    float *partial;      // (2, kH512Shares, stride)
    uint64_t a_net, b_net, stride, w_at, bias_at[2];  // floats from net 0's operand to net 1's; where dW and db start in a vector
    uint32_t lda, ldb, a_cols;  // a_cols: A's valid columns, a multiple of 4
    uint32_t m[2], n;           // C is m[net] x n; n a multiple of 128
    uint32_t nrows, share;      // the slab's samples in whole tiles; samples per share
};
// one launch for both nets and every share; the rows past the slab's samples up to nrows must be zero rows of A and finite in B
void launch_h512_dw(const H512DwArgs &args, hipStream_t stream);

// K rows enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_h512_update)
void launch_mappo_h512_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_batch &batch,
                              const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                              float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream);

}  // namespace mrl
