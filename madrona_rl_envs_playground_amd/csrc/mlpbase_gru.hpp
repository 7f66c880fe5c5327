// MAPPO's RECURRENT MLP actor-critic for the balance beam on the device (C ABI: mrl_mlpbase_act, mrl_rollout_mlpbase and
// mrl_mappo_mlp_update with an mrl_mlpbase_gru_policy, include/mrl_envs.h).  The act's kernel lives in
// mlpbase_gru.hip, the update's in mlpbase_gru_update.hip; capi_mappo.hip validates the arguments.
//
// THE NETWORK (r_actor_critic.py with use_recurrent_policy, utils/rnn.py with recurrent_N 1), per net: MLPBase as in
// mlpbase_policy.hpp, then between the base and the head, with x the base's output row, h the incoming state and m the mask
// (0 where the world's DONE flag is set at the time of the act, else 1):
//     h_in = h * m
//     gi = W_ih x + b_ih,  gh = W_hh h_in + b_hh                       (192 each; torch's gate order r, z, n)
//     r = sigmoid(gi_r + gh_r),  z = sigmoid(gi_z + gh_z),  n = tanh(gi_n + r * gh_n)
//     h' = (1 - z) * n + z * h_in
//     head input = LayerNorm64(h'),  new state = h' (before the LayerNorm)
// sigmoid(x) = 1 / (1 + expf(-x)) and tanh(x) = tanhf(x): gru_sigmoid and gru_tanh below, the only forms any kernel uses.
// Each of the six 64 x 64 products is a cnn_fc_layer (ascending input index, the bias added to the finished sum); gi_g + gh_g
// adds the two finished sums; (1 - z) * n + z * h_in is two products and one sum, unfused (the library is built without
// contraction).
//
// THE FLAT TENSOR: per net base.* exactly as in mlpbase_policy.hpp (fc_h included), then rnn.rnn.weight_ih_l0 (192, 64),
// weight_hh_l0 (192, 64), bias_ih_l0 (192), bias_hh_l0 (192), rnn.norm.weight (64), bias (64), then the head: 25 088 floats more
// per net.
#pragma once

#include "gru_step.hpp"
#include "mappo_loss.hpp"
#include "mlpbase_forward.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

static_assert(kMlpBaseHidden == kGruHidden && kMlpLd == kGruLd && kMlpBaseTile == kGruTile && kMlpBaseThreads == kGruThreads,
              "gru_step.hpp's functions are written for this net's width, LDS row stride, tile and workgroup");
// offsets inside one net, in floats: the GRU block (gru_step.hpp) starts where the plain net's head does
__host__ __device__ constexpr uint32_t gru_wih_at(uint32_t layer_N) { return mlpbase_head_at(layer_N); }
__host__ __device__ constexpr uint32_t gru_head_at(uint32_t layer_N) { return mlpbase_head_at(layer_N) + kGruParams; }
__host__ __device__ constexpr uint32_t gru_net_params(uint32_t layer_N, uint32_t out) { return mlpbase_net_params(layer_N, out) + kGruParams; }

// The workgroup's LDS image: the plain forward image (mlpbase_policy.hpp), then the GRU's image (gru_step.hpp), in floats
constexpr uint32_t kGruHinAt = kMlpFwdFloats, kGruGateAt = kGruHinAt + kGruImgGate, kGruHnAt = kGruHinAt + kGruImgHn, kGruYAt = kGruHinAt + kGruImgY,
                   kGruRstdAt = kGruHinAt + kGruImgRstd, kGruCellAt = kGruHinAt + kGruImgCell, kGruKeepAt = kGruHinAt + kGruImgKeep,
                   kGruFwdFloats = kGruHinAt + kGruImgFloats;
static_assert(kGruFwdFloats * 4u <= 160u * 1024u, "the recurrent forward image fits one workgroup's LDS");

// the GRU and its LayerNorm behind the base: gru_step_forward on this net's image, x = the base's output rows
__device__ __forceinline__ void mlpbase_gru_forward(const float *__restrict__ net, uint32_t layer_N, const float *__restrict__ x,
                                                    float *__restrict__ lds, uint32_t tid)
{
    gru_step_forward(net + gru_wih_at(layer_N), x, lds + kMlpChunkAt, lds + kGruHinAt, tid);
}

// the head of a recurrent net: from gy to outs (row stride 8)
__device__ __forceinline__ void mlpbase_gru_head(const float *__restrict__ net, uint32_t layer_N, uint32_t out_dim, float *__restrict__ lds,
                                                 uint32_t tid)
{
    gru_step_head(net + gru_head_at(layer_N), out_dim, lds + kMlpChunkAt, lds + kGruHinAt, lds + kMlpOutAt, tid);
}

struct MlpBaseGruActArgs {
    MlpBaseActArgs act;   // act.params: the recurrent flat tensor
    float *h[2];          // the running states of the actor and the critic, (N, P, 64)
    float *h0_row[2];     // the record's h0 rows this act fills with the incoming states (nullptr: not written)
    uint32_t write_state; // 0 for the closing value-only act: neither state tensor changes
};

void launch_mlpbase_gru_act(const MlpBaseGruActArgs &args, hipStream_t stream);

// ---- the update (mlpbase_gru_update.hip)

constexpr uint32_t kGruMaxChunk = MRL_MLPBASE_GRU_MAX_CHUNK;  // the longest chunk the update back-propagates through

// The caller's scratch, in floats: the plain update's (mappo_loss.hpp) for Bc chunks a row, then every gradient workgroup's slice
// for the incoming states of a tile's steps (2 nets, groups, kGruMaxChunk, 32, 64), then every row's Bc L sample numbers (int32,
// room for L = kGruMaxChunk), which ValueNorm's recurrence reads.
struct GruUpdateWorkspace {
    MappoWorkspace plain;
    uint64_t history, samples, total;
};
GruUpdateWorkspace gru_update_workspace(uint32_t layer_N, uint32_t minibatch_size, uint32_t num_minibatches);

// K rows of Bc chunk ids enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_mlp_update).
void launch_mappo_gru_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_gru_batch &batch, const int32_t *indices,
                             uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                             float *workspace, float *stats, float *grads, hipStream_t stream);

}  // namespace mrl
