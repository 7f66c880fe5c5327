// MAPPO's RECURRENT CNN actor-critic for the kitchens on the device (C ABI: mrl_cnn_act, mrl_rollout_cnn and mrl_mappo_update with
// MRL_CNN_RECURRENT in the policy's flags, include/mrl_envs.h).  The act's kernel lives in cnn_gru.hip, the
// update's in cnn_gru_update.hip; capi_mappo.hip validates the arguments.
//
// THE NETWORK (r_actor_critic.py with use_recurrent_policy, utils/rnn.py with recurrent_N 1), per net: CNNBase as in
// cnn_policy.hpp (conv 3 x 3 to 32 channels, ReLU, flatten, Linear to 64, ReLU, Linear to 64, ReLU), then the GRU step of
// gru_step.hpp with x = the base's output row h2 (the arithmetic is stated at the head of mlpbase_gru.hpp and is the beam's, word
// for word), then the head on LayerNorm64(h').  The new state is h' before the LayerNorm.
//
// THE FLAT TENSOR: per net base.* exactly as in cnn_policy.hpp, then rnn.rnn.weight_ih_l0 (192, 64), weight_hh_l0 (192, 64),
// bias_ih_l0 (192), bias_hh_l0 (192), rnn.norm.weight (64), bias (64), then the head: 25 088 floats more per net.
//
// THE LDS IMAGE.  The GRU's arrays (gru_step.hpp: nine of 32 x 65 floats plus three of 32, 75 264 bytes) do not fit behind a large
// kitchen's forward image (72 to 154 KB).  When the GRU runs, the only live data of that image are h2 and the weight chunk buffer,
// both inside the first kCnnFcBytes of region A: the int8 rows, the conv weights, the patch offsets and the activation image
// (region B) are dead.  So the GRU image OVERLAYS them, starting right behind the linear layers' arrays:
//     act:     [0, kCnnFcBytes) chunk, h1, h2, outs | [kCnnFcBytes, +kCnnGruImgBytes) the GRU image
//     image  = max(cnn_lds(W, H, F).total, kCnnFcBytes + kCnnGruImgBytes)
// kCnnFcBytes + kCnnGruImgBytes is 109 568 bytes, below the limit, so the recurrent act refuses no kitchen the plain act admits.
// The per-row cell and mask words lie inside the overlay and are therefore written only after fc2.
// The update's image is in cnn_gru_update.hip's header comment and below (CnnGruUpdateLds).
#pragma once

#include "cnn_forward.hpp"
#include "cnn_update.hpp"
#include "gru_step.hpp"

namespace mrl {

static_assert(kCnnHidden == kGruHidden && kCnnFcLd == kGruLd && kCnnTile == kGruTile && kCnnThreads == kGruThreads,
              "gru_step.hpp's functions are written for this net's width, LDS row stride, tile and workgroup");
static_assert(MRL_CNN_GRU_MAX_CHUNK == MRL_MLPBASE_GRU_MAX_CHUNK, "one longest chunk for both recurrent networks");

constexpr uint32_t kCnnGruImgBytes = kGruImgFloats * 4u;
constexpr uint32_t kCnnGruActBytes = kCnnFcBytes + kCnnGruImgBytes;
static_assert(kCnnFcBytes % 16u == 0 && kCnnGruActBytes <= kCnnLdsLimit, "the overlaid GRU image fits whatever the kitchen");
constexpr uint32_t kCnnGruMaxChunk = MRL_CNN_GRU_MAX_CHUNK;

// one recurrent net's parameter count, and where its pieces lie (floats from the net's first)
constexpr uint64_t cnn_gru_net_params(uint64_t W, uint64_t H, uint64_t F, uint64_t out) { return cnn_net_params(W, H, F, out) + kGruParams; }
struct CnnGruNetAt {
    size_t conv_b, fc1_w, fc1_b, fc2_w, fc2_b, gru, head_w, head_b;
};
__host__ __device__ __forceinline__ CnnGruNetAt cnn_gru_net_at(uint32_t k1, uint32_t K2, uint32_t out_dim)
{
    CnnGruNetAt n;
    n.conv_b = (size_t)kCnnChannels * k1;
    n.fc1_w = n.conv_b + kCnnChannels;
    n.fc1_b = n.fc1_w + (size_t)kCnnHidden * K2;
    n.fc2_w = n.fc1_b + kCnnHidden;
    n.fc2_b = n.fc2_w + kCnnHidden * kCnnHidden;
    n.gru = n.fc2_b + kCnnHidden;
    n.head_w = n.gru + kGruParams;
    n.head_b = n.head_w + (size_t)out_dim * kCnnHidden;
    return n;
}

inline uint32_t cnn_gru_act_lds_bytes(const CnnLds &l) { return l.total > kCnnGruActBytes ? l.total : kCnnGruActBytes; }

// CNNBase for a tile, as mrl_cnn_act runs it (the same device functions in the same order, hence the same bits): the tile's int8
// rows and the conv operands into LDS, the convolution, fc1 and fc2.  `net`: the net's first parameter.  With `shifts` (LDS, 32
// words) the rows' shifts are kept there for a later reload.  Leaves h1, h2 and the activation image; ends behind a barrier.
template <class RowAddress>
__device__ __forceinline__ void cnn_gru_base(const CnnActArgs &a, unsigned char *lds, const RowAddress &row_address, uint32_t *shifts,
                                             const float *__restrict__ net, const CnnGruNetAt &at, uint32_t tid)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t K2 = kCnnChannels * a.lds.npos;
    cnn_load_tile(a, lds, row_address, shifts, net, true);
    __syncthreads();
    const uint32_t shift = shifts ? shifts[r] : (uint32_t)(reinterpret_cast<uintptr_t>(row_address(r)) & 3u);
    cnn_conv_tile(a, lds, shift, net + at.conv_b, wave, r, half);
    __syncthreads();  // the activation image is complete; the convolution's operands are dead
    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt);
    float *h1 = reinterpret_cast<float *>(lds + kCnnH1At), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    cnn_fc_layer(reinterpret_cast<float *>(lds + a.lds.act_at), a.lds.act_ld, K2, net + at.fc1_w, net + at.fc1_b, kCnnHidden, true, chunk, h1,
                 kCnnFcLd, wave, lane);
    cnn_fc_layer(h1, kCnnFcLd, kCnnHidden, net + at.fc2_w, net + at.fc2_b, kCnnHidden, true, chunk, h2, kCnnFcLd, wave, lane);
}

struct CnnGruActArgs {
    CnnActArgs act;        // act.params: the recurrent flat tensor
    float *h[2];           // the running states of the actor and the critic, (N, P, 64)
    float *h0_row[2];      // the record's h0 rows this act fills with the incoming states (nullptr: not written)
    uint32_t write_state;  // 0 for the closing value-only act: neither state tensor changes
};

void launch_cnn_gru_act(const CnnGruActArgs &args, hipStream_t stream);

// ---- the update (cnn_gru_update.hip)

// The gradient workgroup's LDS image.  A tile's backward pass is split in phases that never hold the GRU's arrays together with
// the activation image or the int8 rows:
//     convolutional phases (the forward sweep's CNNBase, and the backward pass from fc2 down to dW_conv): today's update image
//         (cnn_update_lds) without its tail -- region A with d_out, d_h2, d_h1, then the activation image;
//     recurrent phase: [0, kUpdFcBytes) chunk, h1 (unused), x_i in h2's place, outs, d_out (d_h2, d_h1 unused) |
//         [kUpdFcBytes, ..) the GRU image, dh carried from step i + 1 (32 x 65), the step's sample numbers (32 words).
//     image = max of the two, then the tile's chunk ids and row shifts (32 words each), which every phase reads.
// The recurrent phase ends at kCnnGruUpdBytes = 135 680 bytes whatever the kitchen; the plain update's image is its conv phases
// plus the same 256 bytes, so no kitchen the plain update admits is refused.
constexpr uint32_t kCnnGruUpdImgAt = kUpdFcBytes, kCnnGruCarryAt = kCnnGruUpdImgAt + kCnnGruImgBytes, kCnnGruSampleAt = kCnnGruCarryAt + kGruRows * 4u,
                   kCnnGruUpdBytes = kCnnGruSampleAt + kCnnTile * 4u;
static_assert(kCnnGruUpdImgAt % 16u == 0 && kCnnGruUpdBytes + kCnnTile * 2u * 4u <= kCnnLdsLimit, "the recurrent phase fits whatever the kitchen");
struct CnnGruUpdateLds {
    CnnLds fwd;        // cnn_update_lds's
    uint32_t tail_at;  // chunk ids (32 words), then row shifts (32 words)
    uint32_t total;
};
inline CnnGruUpdateLds cnn_gru_update_lds(uint32_t W, uint32_t H, uint32_t F)
{
    const CnnUpdateLds plain = cnn_update_lds(W, H, F);
    CnnGruUpdateLds u{};
    u.fwd = plain.fwd;
    u.tail_at = plain.tail_at > kCnnGruUpdBytes ? plain.tail_at : kCnnGruUpdBytes;
    u.total = u.tail_at + kCnnTile * 2u * 4u;
    return u;
}

// The caller's scratch, in floats: the plain update's (mappo_loss.hpp) for Bc chunks a row, then every gradient workgroup's slice
// (2 nets, groups, kCnnGruMaxChunk, 2, 32, 64: per step the base's output x_i -- later dL/dx_i -- and the incoming state), then
// every row's Bc L sample numbers (int32, room for L = kCnnGruMaxChunk), which ValueNorm's recurrence reads.
struct CnnGruUpdateWorkspace {
    MappoWorkspace plain;
    uint64_t slices, samples, total;
};
CnnGruUpdateWorkspace cnn_gru_update_workspace(uint32_t W, uint32_t H, uint32_t F, uint32_t minibatch_size, uint32_t num_minibatches);

// K rows of Bc chunk ids enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_update).
void launch_mappo_cnn_gru_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_gru_batch &batch,
                                 const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                                 float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream);

}  // namespace mrl
