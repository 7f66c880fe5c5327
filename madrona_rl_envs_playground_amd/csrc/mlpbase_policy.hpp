// MAPPO's MLP actor-critic for the balance beam on the device (C ABI: mrl_mlpbase_act, mrl_rollout_mlpbase in
// include/mrl_envs.h).  The kernel lives in mlpbase_policy.hip, the forward pass in mlpbase_forward.hpp;
// capi_mappo.hip validates the arguments and collects the simulator's tensors.
//
// THE NETWORK (train/MAPPO/utils/mlp.py with use_feature_normalization, use_ReLU, use_orthogonal; hidden_size 64), per net:
//     LayerNorm(7) -> Linear(7, 64) -> ReLU -> LayerNorm(64) -> layer_N x [Linear(64, 64) -> ReLU -> LayerNorm(64)] -> head
// head = Linear(64, 4) for the actor (Categorical) and Linear(64, 1) for the critic, whose input is the seat's own observation.
// LayerNorm is (x - mean) / sqrt(var + 1e-5) * weight + bias with the biased variance over the row.
// The balance beam's ACTION_MASK is all ones in every state (src/balance_beam_env/sim.cpp:197): the kernels do not read it.
//
// THE FLAT TENSOR: actor, then critic, each in parameters_to_vector order --
//     feature_norm weight, bias (7, 7); fc1: Linear weight (64, 7), bias, LayerNorm weight, bias; fc_h: the same four tensors with a
//     (64, 64) weight; fc2[i], i < layer_N: the same four; the head's weight (out, 64) and bias.
// fc_h is registered by the reference and never used by its forward (mlp.py:20-27: fc2 are deep copies of it): its 4 288 floats
// per net are part of the tensor, no kernel reads them, and their gradient is zero.
#pragma once

#include "act_record.hpp"
#include "common.hpp"

namespace mrl {

constexpr uint32_t kMlpBaseHidden = 64, kMlpBaseObs = 7, kMlpBaseActions = 4, kMlpBaseTile = 32, kMlpBaseThreads = 256;
constexpr uint32_t kMlpBaseMaxLayerN = 2;
constexpr float kMlpBaseLnEps = 1e-5f;

// offsets inside one net, in floats
constexpr uint32_t kMlpBaseBlock = kMlpBaseHidden * kMlpBaseHidden + 3 * kMlpBaseHidden;  // Linear(64, 64) + bias + LayerNorm: 4 288
constexpr uint32_t kMlpBaseFc1At = 2 * kMlpBaseObs;                                                  // 14
constexpr uint32_t kMlpBaseFcHAt = kMlpBaseFc1At + kMlpBaseHidden * kMlpBaseObs + 3 * kMlpBaseHidden;  // 654
// hidden layer h of the forward pass (0: fc1; h >= 1: fc2[h - 1]): where its Linear weight starts; bias, LayerNorm weight and
// LayerNorm bias follow
__host__ __device__ constexpr uint32_t mlpbase_layer_at(uint32_t h) { return h == 0 ? kMlpBaseFc1At : kMlpBaseFcHAt + kMlpBaseBlock * h; }
__host__ __device__ constexpr uint32_t mlpbase_head_at(uint32_t layer_N) { return kMlpBaseFcHAt + kMlpBaseBlock * (1u + layer_N); }
__host__ __device__ constexpr uint32_t mlpbase_net_params(uint32_t layer_N, uint32_t out)
{
    return mlpbase_head_at(layer_N) + out * kMlpBaseHidden + out;
}

// The workgroup's LDS image, in floats, for 32 samples of one net.  Rows of the 64-wide arrays are 65 floats apart (lane r reads
// bank r + k), rows of the 7-wide ones 9 (column 7 is the zero the padded product reads).
//   chunk        the 64 x 64 weight chunk of cnn_fc_layer
//   in0          LayerNorm(7)'s output, fc1's input
//   xhat0        the observation rows as floats, then in place their normalised rows
//   rstd         1 / sqrt(var + eps) per (LayerNorm 0..3, row)
//   mask         per (hidden layer, row): bit j set where the ReLU passed unit j (64 bits)
//   outs         the head's outputs (32 x 8)
//   xhat[h]      hidden layer h: relu(Linear) as cnn_fc_layer writes it, then in place its normalised rows
//   y[h]         LayerNorm's output of hidden layer h: the next layer's input
// The act needs none of xhat0, rstd, mask and xhat once a layer is done; the update's backward pass reads them all, and it is one
// forward function for both.
constexpr uint32_t kMlpLd = kMlpBaseHidden + 1, kMlpLd0 = 9, kMlpMaxLayers = 1 + kMlpBaseMaxLayerN;
constexpr uint32_t kMlpChunkAt = 0, kMlpIn0At = kMlpChunkAt + kMlpBaseHidden * kMlpLd, kMlpXhat0At = kMlpIn0At + kMlpBaseTile * kMlpLd0,
                   kMlpRstdAt = kMlpXhat0At + kMlpBaseTile * kMlpLd0, kMlpMaskAt = kMlpRstdAt + (kMlpMaxLayers + 1) * kMlpBaseTile,
                   kMlpOutAt = kMlpMaskAt + kMlpMaxLayers * kMlpBaseTile * 2, kMlpXhatAt = kMlpOutAt + kMlpBaseTile * 8,
                   kMlpYAt = kMlpXhatAt + kMlpMaxLayers * kMlpBaseTile * kMlpLd, kMlpFwdFloats = kMlpYAt + kMlpMaxLayers * kMlpBaseTile * kMlpLd;
static_assert((kMlpMaskAt & 1u) == 0, "the ReLU masks are 64-bit words");

struct MlpBaseActArgs : ActArgs {
    const float *params;       // actor's tensors, then the critic's
    const int32_t *obs;        // OBSERVATION (P, N, 7)
    const float *reward;       // REWARD (P, N)
    int32_t *obs_row;          // the record's (N, P, 7) row for this call (nullptr: not written)
    uint32_t layer_N;
};

void launch_mlpbase_act(const MlpBaseActArgs &args, hipStream_t stream);

}  // namespace mrl
