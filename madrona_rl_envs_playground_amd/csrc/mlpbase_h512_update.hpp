// MAPPO's update for the balance beam's MLPBase actor-critic at hidden_size 512 (C ABI: mrl_mappo_mlp_update with MRL_MLPBASE_H512 in
// mrl_mlpbase_policy.flags and hidden = 512, sized by mrl_mappo_mlp_workspace_bytes with 512 | MRL_MLPBASE_H512_HIDDEN; DESIGN.md
// section 33).  The kernels live in mlpbase_h512_update.hip; capi_mappo.hip validates the arguments.
//
// A net of this width has 0.53 to 0.80 million parameters, so the hidden-64 scheme of a gradient vector per workgroup
// (mlpbase_update.hip) is out of reach.  The update is LAYERED, as the hidden-512 CNN's (cnn_h512_update.hpp): a row's index list is
// cut into SLABS of at most kMlpH512Slab consecutive samples, a slab's activations of both nets are stored in the workspace, and the
// gradient goes back one layer per launch over the slab (mlpbase_h512_update.hip lists the launches).
//
// THE ORDER OF EVERY SUM.  The forward pass is the act's (mlpbase_h512.hpp; the same device functions, mlpbase_h512_forward.hpp).
//   dy of a hidden layer   dy[s][c] = sum over j of d_pre_{l+1}[s][j] W_{l+1}[j][c]: ONE chain of fused multiply-adds from 0 over
//                          j = 0 .. 511 ascending (a matrix instruction takes j = 2 kk, then 2 kk + 1).  Below the head: one fmaf per
//                          head output, ascending, from 0.
//   LayerNorm backward     a wavefront per row, lane l the columns l + 64 j; xhat = (z - mean) rstd, g = dy gamma; the two row sums
//                          (g and g xhat) are the lane's eight columns added in ascending order to 0, then wave_sum; dz = rstd ((g -
//                          sum_g / 512) - xhat (sum_gx / 512)), kept where z > 0.
//   dgamma, dbeta          of LayerNorm(512): per tile of 32 samples a lane per column adds dy xhat (dy) in ascending row order from 0;
//                          mrl_mlp512_fold adds the tiles' vectors in ascending tile order from 0.
//   dW, db of a layer      a slab's n samples, rounded up to whole tiles of 32 (rows past n are zero rows), are cut into kH512Shares
//                          contiguous shares of ceil(tiles / kH512Shares) tiles; each output adds share q's products as ONE chain
//                          from 0 in ascending sample order (Linear(512, 512) and the head on mrl_h512_dw, cnn_h512_update.hpp; fc1,
//                          its bias and feature_norm a thread per output); mrl_mlp512_fold adds the share sums in ascending q from 0.
//   d(feature_norm out)    d_in0[s][i] = sum over j of W_fc1[j][i] d_pre_0[s][j], one fmaf chain over j = 0 .. 511 from 0.
//   slabs                  the slab sum is added to the running gradient, which the first slab starts; slabs run in ascending order.
// The stats' terms are double sums: lanes, then tiles, then slabs, each ascending.  The fc_h block's gradient is written as zeros.
#pragma once

#include "cnn_h512_update.hpp"
#include "mlpbase_h512.hpp"

namespace mrl {

constexpr uint32_t kMlpH512Slab = 2048;  // samples per slab: a multiple of 64
constexpr uint32_t kMlpH512MaxLayers = 1 + kMlpBaseMaxLayerN;  // fc1 and fc2[0 .. layer_N - 1]
constexpr uint32_t kMlpH512Tile = 32;                          // the update runs 32-row tiles at every size (RB = 1)

// The caller's scratch, in floats.  rows = min(kMlpH512Slab, B rounded up to 64): one slab's rows, whatever B is beyond that;
// L = 1 + layer_N hidden layers.
//   row_norm, row_sums   (K, 2) each, padded to 4        ValueNorm's recurrence, as in mappo_workspace
//   in0, y0              (2, rows, 8) each               the observation rows as floats; LayerNorm(7)'s output (column 7 zero)
//   stat0, d_in0         (2, rows, 2), (2, rows, 8)      LayerNorm(7)'s (mean, rstd); dL/d(its output)
//   z, y, d_pre          (2, L, rows, 512) each          post-ReLU rows, LayerNorm(512)'s outputs, dL/d(Linear output)
//   stat                 (2, L, rows, 2)                 LayerNorm(512)'s (mean, rstd)
//   out, d_out           (2, rows, 8) each
//   ln                   (2, L, rows / 32, 1024)         the tiles' (dgamma, dbeta)
//   partial              (2, kH512Shares, stride)        the shares' gradient sums; stride = the actor's parameter count padded to 4
//   run, grad            (2, stride) each                the running gradient over the slabs; mrl_grad_reduce's output
//   sumsq                (2, blocks) padded to 4, blocks = ceil(stride / 256)
//   slab_stats           (2, rows / 32, 8) doubles;  run_stats (2, 8) doubles
struct MlpH512Workspace {
    uint64_t row_norm, row_sums, in0, y0, stat0, d_in0, z, y, d_pre, stat, out, d_out, ln, partial, run, grad, sumsq, slab_stats, run_stats, total;
    uint64_t stride, blocks, rows, layers;
};

inline MlpH512Workspace mlp_h512_workspace(uint32_t layer_N, uint32_t minibatch_size, uint32_t num_minibatches)
{
    const auto pad = [](uint64_t n) { return (n + 3) & ~uint64_t(3); };
    const uint64_t whole = ((uint64_t)minibatch_size + 63) & ~uint64_t(63);
    MlpH512Workspace w;
    w.rows = whole < kMlpH512Slab ? whole : kMlpH512Slab;
    w.layers = 1u + layer_N;
    w.stride = pad(mlpbase_h512_net_params(layer_N, kMlpBaseActions));
    w.blocks = (w.stride + kAdamThreads - 1) / kAdamThreads;
    const uint64_t wide = 2 * w.layers * w.rows * kMlpH512Hidden;
    w.row_norm = 0;
    w.row_sums = w.row_norm + pad(2 * (uint64_t)num_minibatches);
    w.in0 = w.row_sums + pad(2 * (uint64_t)num_minibatches);
    w.y0 = w.in0 + 2 * w.rows * 8;
    w.stat0 = w.y0 + 2 * w.rows * 8;
    w.d_in0 = w.stat0 + 2 * w.rows * 2;
    w.z = w.d_in0 + 2 * w.rows * 8;
    w.y = w.z + wide;
    w.d_pre = w.y + wide;
    w.stat = w.d_pre + wide;
    w.out = w.stat + 2 * w.layers * w.rows * 2;
    w.d_out = w.out + 2 * w.rows * 8;
    w.ln = w.d_out + 2 * w.rows * 8;
    w.partial = w.ln + 2 * w.layers * (w.rows / kMlpH512Tile) * 2 * kMlpH512Hidden;
    w.run = w.partial + 2 * kH512Shares * w.stride;
    w.grad = w.run + 2 * w.stride;
    w.sumsq = w.grad + 2 * w.stride;
    w.slab_stats = w.sumsq + pad(2 * w.blocks);
    w.run_stats = w.slab_stats + 2 * (w.rows / kMlpH512Tile) * kMappoStats * 2;
    w.total = w.run_stats + 2 * kMappoStats * 2;
    return w;
}

// The workgroup's LDS images, in floats.  The forward pass: the act's 32-row image (mlpbase_h512.hpp) and the tile's LayerNorm
// statistics behind it.  The backward pass of a layer: dy, 32 rows of 513; the rows' (mean, rstd); dL/d(head output), 32 rows of 8.
constexpr uint32_t kMlpH512FwdStatAt = mlpbase_h512_lds_floats(kMlpH512Tile), kMlpH512FwdFloats = kMlpH512FwdStatAt + 2u * kMlpH512Tile;
constexpr uint32_t kMlpH512BwdStatAt = kMlpH512Tile * kMlpH512Ld, kMlpH512BwdDoutAt = kMlpH512BwdStatAt + 2u * kMlpH512Tile,
                   kMlpH512BwdFloats = kMlpH512BwdDoutAt + 8u * kMlpH512Tile;

// K rows enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_mlp_update)
void launch_mappo_mlp_h512_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_batch &batch, const int32_t *indices,
                                  uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                                  float *workspace, float *stats, float *grads, hipStream_t stream);

}  // namespace mrl
