// launch_ppo_update: the plain PPO update, one policy (ppo_update_kernels.hpp has the kernels).  The update of
// a bank's members is an object of its own, ppo_update_bank.hip, so that this one holds the kernels it always held.
#include "ppo_update_kernels.hpp"

namespace mrl {

void launch_ppo_update(const mrl_mlp_policy &shape, const mrl_ppo_optimizer &opt, const mrl_ppo_batch &batch,
                       const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config &cfg,
                       float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (opt.num_members) return launch_ppo_update_members(shape, opt, batch, indices, num_minibatches, minibatch_size, cfg, workspace, stats, grads, stream);
    PpoLaunch l = ppo_launch(shape, opt, batch, num_minibatches, minibatch_size, cfg, workspace);
    if (l.norm && num_minibatches) {
        hipLaunchKernelGGL(mrl_ppo_mean_std<>, dim3(num_minibatches), dim3(kMeanThreads), 0, stream, batch.advantages, indices,
                           minibatch_size, workspace + l.ws.mean_std);
        MRL_HIP(hipGetLastError());
    }
    const dim3 grid(l.share.groups, 2);
    for (uint32_t k = 0; k < num_minibatches; k++) {
        l.g.indices = indices + (size_t)k * minibatch_size;
        l.g.mean_std = l.norm ? workspace + l.ws.mean_std + 2 * (size_t)k : nullptr;
        launch_ppo_grad(l.D, l.A, grid, l.g, stream);
        l.ad.grads_row = grads ? grads + (size_t)k * l.P : nullptr;
        adam_set_step(l.ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.lr});
        l.row.row = stats ? stats + (size_t)k * kPpoStats : nullptr;
        launch_adam_step(l.ad, l.row, stream);
    }
}

}  // namespace mrl
