// MAPPO's update for the balance beam's MLPBase actor-critic on the device (C ABI: mrl_mappo_mlp_update,
// mrl_mappo_mlp_workspace_bytes in include/mrl_envs.h).  The kernel lives in mlpbase_update.hip; capi_mappo.hip
// validates the arguments.  The loss head, the ValueNorm recurrence, the workspace and the launch plan are mrl_mappo_update's
// (mappo_loss.hpp), the optimiser tail every update's (adam_step.hpp).
#pragma once

#include "mappo_loss.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

// The gradient workgroup's LDS image: the forward pass's (mlpbase_policy.hpp), then dL/d(head output) (32 x 8), two 32 x 64
// gradient arrays that take turns -- dL/d(LayerNorm output) and dL/d(Linear output) of the layer at hand -- and the tile's sample
// numbers.
constexpr uint32_t kMlpDoutAt = kMlpFwdFloats, kMlpDyAt = kMlpDoutAt + kMlpBaseTile * 8, kMlpDzAt = kMlpDyAt + kMlpBaseTile * kMlpLd,
                   kMlpSampleAt = kMlpDzAt + kMlpBaseTile * kMlpLd, kMlpUpdFloats = kMlpSampleAt + kMlpBaseTile;

// K rows enqueued on `stream`; every argument has been validated (capi_mappo.hip, mrl_mappo_mlp_update).  With `members`
// (mrl_mappo_mlp_bank_update) opt, indices, value_norm_state, workspace, stats and grads are the first member's.
void launch_mappo_mlp_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_batch &batch, const int32_t *indices,
                             uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                             float *workspace, float *stats, float *grads, hipStream_t stream, const MappoMembers &members = kMappoOneMember);

}  // namespace mrl
