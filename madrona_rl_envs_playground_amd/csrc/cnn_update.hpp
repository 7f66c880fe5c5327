// MAPPO's update for the Overcooked CNN actor-critic on the device (C ABI: mrl_mappo_update, mrl_mappo_workspace_bytes in
// include/mrl_envs.h).  The kernels live in cnn_update.hip; capi_mappo.hip validates the arguments.
#pragma once

#include "cnn_policy.hpp"
#include "mappo_loss.hpp"

namespace mrl {

// The gradient workgroup's LDS image: mrl_cnn_act's (cnn_lds) with region A at least large enough for what back-propagation
// keeps beside the forward pass's chunk, h1, h2 and head outputs -- dL/d(head output) (32 x 8), dL/d(pre-activation of fc2) and
// of fc1 (32 rows of 65 floats each) -- and, behind the activation image, the tile's sample numbers and row shifts (32 x 2
// words).  The activation image doubles as dL/d(pre-activation of the convolution): it is overwritten in place once dW_fc1 has
// been formed, and the observation rows are loaded a second time into region A for dW_conv.
constexpr uint32_t kUpdDoutAt = kCnnFcBytes, kUpdDh2At = kUpdDoutAt + kCnnTile * 8 * 4, kUpdDh1At = kUpdDh2At + kCnnTile * kCnnFcLd * 4,
                   kUpdFcBytes = kUpdDh1At + kCnnTile * kCnnFcLd * 4;
struct CnnUpdateLds {
    CnnLds fwd;        // act_at moved up where region A grew; every other field is cnn_lds's
    uint32_t tail_at;  // sample numbers (32 words), then row shifts (32 words)
    uint32_t total;
};
inline CnnUpdateLds cnn_update_lds(uint32_t W, uint32_t H, uint32_t F)
{
    CnnUpdateLds u{};
    u.fwd = cnn_lds(W, H, F);
    if (u.fwd.act_at < kUpdFcBytes) u.fwd.act_at = kUpdFcBytes;
    u.tail_at = u.fwd.act_at + kCnnTile * u.fwd.act_ld * 4u;
    u.fwd.total = u.tail_at;
    u.total = u.tail_at + kCnnTile * 2u * 4u;
    return u;
}

// K rows enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_update).  With `members`
// (mrl_mappo_bank_update) opt, indices, value_norm_state, workspace, stats and grads are the first member's.
void launch_mappo_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_batch &batch,
                         const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                         float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream,
                         const MappoMembers &members = kMappoOneMember);

}  // namespace mrl
