// MAPPO's MLP actor-critic for the balance beam at the reference trainer's default hidden_size 512 (train/config.py:200): the act
// and the rollout (C ABI: mrl_mlpbase_act and mrl_rollout_mlpbase with MRL_MLPBASE_H512 in mrl_mlpbase_policy.flags and hidden =
// 512).  The kernel lives in mlpbase_h512.hip; capi_mappo.hip validates the arguments.
//
// THE NETWORK, per net (train/MAPPO/utils/mlp.py as at 64, mlpbase_policy.hpp):
//     LayerNorm(7) -> Linear(7, 512) -> ReLU -> LayerNorm(512) -> layer_N x [Linear(512, 512) -> ReLU -> LayerNorm(512)] -> head
// head = Linear(512, 4) for the actor and Linear(512, 1) for the critic; eps 1e-5, the biased variance.
//
// THE FLAT TENSOR is mlpbase_policy.hpp's with 512 in place of 64: actor, then critic, each in parameters_to_vector order, the
// registered-but-unused fc_h block (263 680 floats per net) included; no kernel reads it.
//
// THE ORDER OF EVERY SUM.
//   Linear      an output starts from 0 and adds its products with one fused multiply-add each in ascending input index, ONE chain
//               over k = 0 .. 511 (fc1: k = 0 .. 6 and one zero product), and the bias is added to the finished sum.  A matrix
//               instruction takes k = 2 kk (lanes 0..31) and 2 kk + 1 (lanes 32..63), in that order.
//   LayerNorm   a wavefront per row; lane l owns columns l, l + 64, ..., l + 448 (LayerNorm(7): column l where l < 7, else nothing).
//               A sum over the row is the lane's own columns added in ascending order to 0.0f, then wave_sum (mlpbase_forward.hpp:
//               partners 32, 16, 8, 4, 2, 1 lanes apart).  mean = sum(x) / D; var = sum((x - mean)^2) / D; rstd = 1 / sqrtf(var +
//               1e-5); y = ((x - mean) * rstd) * weight + bias, a product, a product and a sum.  A row of variance 0 has x - mean = 0
//               in every column: y is the bias.
// A row's arithmetic reads its own LDS row and the net's weights only: neither its tile-mates, its place in the tile, the tile's
// width nor the number of worlds can change a bit of its outputs.
#pragma once

#include "act_record.hpp"
#include "common.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

constexpr uint32_t kMlpH512Hidden = 512, kMlpH512Threads = 256;
constexpr uint32_t kMlpH512Ld = kMlpH512Hidden + 1;  // a row of h in LDS: odd, lane r reads bank r + k
// a workgroup's tile is 32 rows, or 64 (two row blocks behind ONE read of the weights) once the call has this many samples
constexpr uint32_t kMlpH512WideFrom = 4096;

// offsets inside one net, in floats: mlpbase_policy.hpp's with the width replaced
constexpr uint32_t kMlpH512Block = kMlpH512Hidden * kMlpH512Hidden + 3 * kMlpH512Hidden;                 // 263 680
constexpr uint32_t kMlpH512Fc1At = 2 * kMlpBaseObs;                                                      // 14
constexpr uint32_t kMlpH512FcHAt = kMlpH512Fc1At + kMlpH512Hidden * kMlpBaseObs + 3 * kMlpH512Hidden;    // 5 134
// hidden layer h of the forward pass (0: fc1; h >= 1: fc2[h - 1]): its Linear weight; bias, LayerNorm weight and bias follow
__host__ __device__ constexpr uint32_t mlpbase_h512_layer_at(uint32_t h) { return h == 0 ? kMlpH512Fc1At : kMlpH512FcHAt + kMlpH512Block * h; }
__host__ __device__ constexpr uint32_t mlpbase_h512_head_at(uint32_t layer_N) { return kMlpH512FcHAt + kMlpH512Block * (1u + layer_N); }
__host__ __device__ constexpr uint32_t mlpbase_h512_net_params(uint32_t layer_N, uint32_t out)
{
    return mlpbase_h512_head_at(layer_N) + out * kMlpH512Hidden + out;
}
static_assert(mlpbase_h512_net_params(2, 4) == 798226u && mlpbase_h512_net_params(2, 1) == 796687u, "layer_N 2");
static_assert(mlpbase_h512_net_params(1, 4) == 534546u && mlpbase_h512_net_params(1, 1) == 533007u, "layer_N 1");

// The workgroup's LDS image, in floats, for a tile of R = 32 or 64 rows of one net:
//   h     R rows of 513: a hidden layer's relu(Linear), then in place its LayerNorm output, the next layer's input.  A layer's
//         sums wait in registers until every wave has read the previous h.
//   in0   R rows of 9: the observation rows as floats, then in place LayerNorm(7)'s output (column 7 is the zero the padded
//         product reads)
//   outs  the head's outputs, R rows of 8 (act_tail's stride)
// The weights never pass through LDS: a lane fetches the row of torch's weight it owns straight into the matrix instruction's
// operand registers (mlpbase_h512.hip).
__host__ __device__ constexpr uint32_t mlpbase_h512_in0_at(uint32_t rows) { return rows * kMlpH512Ld; }
__host__ __device__ constexpr uint32_t mlpbase_h512_out_at(uint32_t rows) { return mlpbase_h512_in0_at(rows) + rows * kMlpLd0; }
__host__ __device__ constexpr uint32_t mlpbase_h512_lds_floats(uint32_t rows) { return mlpbase_h512_out_at(rows) + rows * 8u; }
static_assert(mlpbase_h512_lds_floats(64) * 4u <= 160u * 1024u, "the 64-row image fits one workgroup's LDS");

// `args` as for launch_mlpbase_act, args.params a hidden-512 parameter array
void launch_mlpbase_act_h512(const MlpBaseActArgs &args, hipStream_t stream);

}  // namespace mrl
