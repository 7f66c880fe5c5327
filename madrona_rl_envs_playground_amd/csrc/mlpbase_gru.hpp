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

#include "mappo_loss.hpp"
#include "mlpbase_forward.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

constexpr uint32_t kGruGates = 3 * kMlpBaseHidden;  // 192
constexpr uint32_t kGruParams = 2 * kGruGates * kMlpBaseHidden + 2 * kGruGates + 2 * kMlpBaseHidden;  // 25 088
// offsets inside one net, in floats: the GRU block starts where the plain net's head does
__host__ __device__ constexpr uint32_t gru_wih_at(uint32_t layer_N) { return mlpbase_head_at(layer_N); }
__host__ __device__ constexpr uint32_t gru_whh_at(uint32_t layer_N) { return gru_wih_at(layer_N) + kGruGates * kMlpBaseHidden; }
__host__ __device__ constexpr uint32_t gru_bih_at(uint32_t layer_N) { return gru_whh_at(layer_N) + kGruGates * kMlpBaseHidden; }
__host__ __device__ constexpr uint32_t gru_bhh_at(uint32_t layer_N) { return gru_bih_at(layer_N) + kGruGates; }
__host__ __device__ constexpr uint32_t gru_norm_at(uint32_t layer_N) { return gru_bhh_at(layer_N) + kGruGates; }
__host__ __device__ constexpr uint32_t gru_head_at(uint32_t layer_N) { return mlpbase_head_at(layer_N) + kGruParams; }
__host__ __device__ constexpr uint32_t gru_net_params(uint32_t layer_N, uint32_t out) { return mlpbase_net_params(layer_N, out) + kGruParams; }

// The workgroup's LDS image behind the plain forward image (mlpbase_policy.hpp), in floats, rows 65 apart:
//   hin          the tile's masked incoming state rows h * m; mlpbase_gru_forward leaves h' there
//   gate[0..5]   gi_r, gi_z, gi_n, gh_r, gh_z, gh_n as the products leave them; then r, z and n in place of gi_*, gh_n stays
//   hn           h', then in place its normalised rows
//   gy           LayerNorm64(h'), the head's input
//   grstd        1 / sqrt(var + eps) of that LayerNorm per row
//   cell, keep   per row: the sample's state row (world * P + seat; kGruAbsent for a row the tile lacks) and its mask m
constexpr uint32_t kGruRows = kMlpBaseTile * kMlpLd;
constexpr uint32_t kGruHinAt = kMlpFwdFloats, kGruGateAt = kGruHinAt + kGruRows, kGruHnAt = kGruGateAt + 6 * kGruRows, kGruYAt = kGruHnAt + kGruRows,
                   kGruRstdAt = kGruYAt + kGruRows, kGruCellAt = kGruRstdAt + kMlpBaseTile, kGruKeepAt = kGruCellAt + kMlpBaseTile,
                   kGruFwdFloats = kGruKeepAt + kMlpBaseTile;
static_assert(kGruFwdFloats * 4u <= 160u * 1024u, "the recurrent forward image fits one workgroup's LDS");
constexpr uint32_t kGruAbsent = 0xFFFFFFFFu;

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) { return tanhf(x); }

// The GRU and its LayerNorm for the tile: x = the base's output rows (LDS, rows 65 apart), lds + kGruHinAt = h * m.  Leaves the
// image described above; thread tid owns elements tid, tid + 256, ... of the 32 x 64 tile in every element-wise pass, so after
// the call it may read back the h' it wrote to hin without a barrier (there is one anyway: the LayerNorm ends behind it).
__device__ __forceinline__ void mlpbase_gru_forward(const float *__restrict__ net, uint32_t layer_N, const float *__restrict__ x,
                                                    float *__restrict__ lds, uint32_t tid)
{
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    float *chunk = lds + kMlpChunkAt, *hin = lds + kGruHinAt, *gate = lds + kGruGateAt, *hn = lds + kGruHnAt;
    const float *__restrict__ w_ih = net + gru_wih_at(layer_N), *__restrict__ w_hh = net + gru_whh_at(layer_N);
    const float *__restrict__ b_ih = net + gru_bih_at(layer_N), *__restrict__ b_hh = net + gru_bhh_at(layer_N);
#pragma unroll 1
    for (uint32_t g = 0; g < 3u; g++) {
        cnn_fc_layer(x, kMlpLd, kMlpBaseHidden, w_ih + g * kMlpBaseHidden * kMlpBaseHidden, b_ih + g * kMlpBaseHidden, kMlpBaseHidden, false, chunk,
                     gate + g * kGruRows, kMlpLd, wave, lane);
        cnn_fc_layer(hin, kMlpLd, kMlpBaseHidden, w_hh + g * kMlpBaseHidden * kMlpBaseHidden, b_hh + g * kMlpBaseHidden, kMlpBaseHidden, false,
                     chunk, gate + (3u + g) * kGruRows, kMlpLd, wave, lane);
    }
    for (uint32_t idx = tid; idx < kMlpBaseTile * kMlpBaseHidden; idx += kMlpBaseThreads) {
        const uint32_t at = (idx >> 6) * kMlpLd + (idx & 63u);
        const float r = gru_sigmoid(gate[at] + gate[3u * kGruRows + at]);
        const float z = gru_sigmoid(gate[kGruRows + at] + gate[4u * kGruRows + at]);
        const float n = gru_tanh(gate[2u * kGruRows + at] + r * gate[5u * kGruRows + at]);
        const float h = hin[at], next = (1.0f - z) * n + z * h;
        gate[at] = r, gate[kGruRows + at] = z, gate[2u * kGruRows + at] = n;
        hin[at] = next, hn[at] = next;
    }
    __syncthreads();
    const float *__restrict__ norm = net + gru_norm_at(layer_N);
    mlpbase_layer_norm(hn, lds + kGruYAt, kMlpLd, kMlpBaseHidden, norm, norm + kMlpBaseHidden, lds + kGruRstdAt, nullptr, wave, lane);
}

// the head of a recurrent net: from gy to outs (row stride 8)
__device__ __forceinline__ void mlpbase_gru_head(const float *__restrict__ net, uint32_t layer_N, uint32_t out_dim, float *__restrict__ lds,
                                                 uint32_t tid)
{
    const float *__restrict__ head_w = net + gru_head_at(layer_N);
    cnn_fc_layer(lds + kGruYAt, kMlpLd, kMlpBaseHidden, head_w, head_w + out_dim * kMlpBaseHidden, out_dim, false, lds + kMlpChunkAt,
                 lds + kMlpOutAt, 8u, tid >> 6, tid & 63u);
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
