// launch_ppo_update_members: mrl_ppo_update with opt->num_members = M > 0 -- K seeds of the small PPO agent trained in one call
// (include/mrl_envs.h).  The launches are the plain update's, 1 + 3 R of them whatever M is, with the member
// in blockIdx.z: the kernels of ppo_update_kernels.hpp with their member strides, then the optimiser tail's MEMBERS instances
// (adam_step.hpp).  Member m reads and writes row m of the three optimizer arrays, indices[m], slice m of the workspace, stats[m]
// and grads[m]; the batch arrays, the configuration and the step number are everyone's.  Per member the arithmetic, and its order,
// is the plain update's: the same bits.
#include "ppo_update_kernels.hpp"

namespace mrl {

void launch_ppo_update_members(const mrl_mlp_policy &shape, const mrl_ppo_optimizer &opt, const mrl_ppo_batch &batch,
                               const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config &cfg,
                               float *workspace, float *stats, float *grads, hipStream_t stream)
{
    const uint32_t members = opt.num_members;
    PpoLaunch l = ppo_launch(shape, opt, batch, num_minibatches, minibatch_size, cfg, workspace);
    const PpoMemberStrides strides{l.P, (uint64_t)num_minibatches * minibatch_size, l.ws.total};
    if (l.norm && num_minibatches) {
        hipLaunchKernelGGL(mrl_ppo_mean_std<PpoMemberStrides>, dim3(num_minibatches, 1, members), dim3(kMeanThreads), 0, stream,
                           batch.advantages, indices, minibatch_size, workspace + l.ws.mean_std, strides);
        MRL_HIP(hipGetLastError());
    }
    l.ad.member_scratch = l.ws.total;
    l.ad.member_params = l.P;
    l.ad.member_grads_row = (uint64_t)num_minibatches * l.P;
    const dim3 grid(l.share.groups, 2, members);
    for (uint32_t k = 0; k < num_minibatches; k++) {
        l.g.indices = indices + (size_t)k * minibatch_size;  // member 0's row k
        l.g.mean_std = l.norm ? workspace + l.ws.mean_std + 2 * (size_t)k : nullptr;
        launch_ppo_grad(l.D, l.A, grid, l.g, stream, strides);
        l.ad.grads_row = grads ? grads + (size_t)k * l.P : nullptr;
        adam_set_step(l.ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.lr});
        l.row.row = stats ? stats + (size_t)k * kPpoStats : nullptr;
        launch_adam_step_members(l.ad, PpoMemberStatsRow{l.row, l.ws.total / 2, (uint64_t)num_minibatches * kPpoStats}, members, stream);
    }
}

}  // namespace mrl
