// mrl_mappo_mlp_update: MAPPO's update for the balance beam's MLPBase actor-critic without torch in the loop (include/mrl_envs.h,
// mrl_mappo_mlp_update).  The launch plan is mrl_mappo_update's (cnn_update.hip): the ValueNorm recurrence
// up front, then per row
//   mrl_mappo_mlp_grad  workgroup (g, net) of four wavefronts owns samples [g * share, (g + 1) * share) of the row for the actor
//                     (net 0) or the critic (net 1) and takes them 32 at a time.  Per tile: the forward pass of mrl_mlpbase_act
//                     into LDS (the same device function, hence the same bits), which leaves every layer's normalised rows,
//                     reciprocal standard deviations and ReLU signs there; the loss head (a lane per sample, mappo_loss.hpp); then
//                     back-propagation through the head and, per hidden layer from the last to the first, LayerNorm, ReLU and
//                     Linear, down to feature_norm.
//                       LayerNorm   with g = dy * weight over the row: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), a
//                                   wavefront per row and wave_sum's fixed order; dweight = sum over samples of dy * xhat and dbias
//                                   = sum of dy, a lane per column in ascending sample order
//                       Linear      dW = dz^T in on v_mfma_f32_32x32x2_f32 with k = the tile's samples, a 32 x 32 block per
//                                   wavefront; d(in) = dz W with k = the layer's units (fc1's seven columns: fmaf over the units
//                                   ascending); db in ascending sample order
//                     The accumulators live in the workgroup's own partial vector in global memory, as mrl_mappo_grad's do: a
//                     sum over the share is ONE chain in sample order and nothing but its owner touches the vector.  The fc_h
//                     segment of the vector (registered by the reference, used by no forward pass) is written as zeros.
//   mrl_grad_reduce, mrl_clip_adam  the optimiser tail (adam_step.hpp), a segment per net.
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run.
#include "mlpbase_update.hpp"
#include "mlpbase_forward.hpp"

namespace mrl {

namespace {

extern __shared__ __attribute__((aligned(16))) unsigned char mlp_upd_lds_image[];

struct MappoMlpGradArgs {
    const float *params;
    const int32_t *obs;  // (S, 7)
    const int32_t *actions;
    const float *logprobs, *value_preds, *returns, *advantages;
    const int32_t *indices;  // this row's B sample numbers
    const float *row_norm;   // this row's ValueNorm (mean, sqrt(var)); nullptr without MRL_MAPPO_VALUENORM
    float *partial_grads;    // (2, groups, stride)
    double *partial_stats;   // (2, groups, 8)
    uint64_t share, stride;
    uint32_t minibatch_size, batch_size, groups, layer_N;
    MappoLoss loss;
};

// sum over the tile's samples of v[s * ld + col] (* w[s * ld + col]) on top of what the previous tile left, a lane per column
__device__ __forceinline__ void column_sum(float *__restrict__ g, bool first, const float *__restrict__ v, const float *__restrict__ w,
                                           uint32_t ld, uint32_t w_ld, uint32_t col)
{
    float sum = first ? 0.0f : g[col];
    for (uint32_t s = 0; s < kMlpBaseTile; s++) sum += w ? v[s * ld + col] * w[s * w_ld + col] : v[s * ld + col];
    g[col] = sum;
}

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mappo_mlp_grad(MappoMlpGradArgs a)
{
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x, layer_N = a.layer_N, out_dim = net ? 1u : kMlpBaseActions;
    const uint32_t net_at = net ? mlpbase_net_params(layer_N, kMlpBaseActions) : 0u;
    const float *__restrict__ params = a.params + net_at;
    // this workgroup's partial vector, in the net's parameter order
    float *__restrict__ grads = a.partial_grads + ((size_t)net * a.groups + blockIdx.x) * a.stride;
    const float *__restrict__ head_w = params + mlpbase_head_at(layer_N);
    float *__restrict__ g_head_w = grads + mlpbase_head_at(layer_N), *__restrict__ g_head_b = g_head_w + out_dim * kMlpBaseHidden;

    float *lds = reinterpret_cast<float *>(mlp_upd_lds_image);
    float *in0 = lds + kMlpIn0At, *xhat0 = lds + kMlpXhat0At, *rstd = lds + kMlpRstdAt, *outs = lds + kMlpOutAt;
    const unsigned long long *mask = reinterpret_cast<const unsigned long long *>(lds + kMlpMaskAt);
    float *d_out = lds + kMlpDoutAt, *dy = lds + kMlpDyAt, *dz = lds + kMlpDzAt;
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + kMlpSampleAt);

    const uint64_t begin = blockIdx.x * a.share;
    const uint64_t end = begin + a.share < a.minibatch_size ? begin + a.share : a.minibatch_size;
    const float count = (float)a.minibatch_size;
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    // fc_h: no forward pass reads it, so its gradient is zero
    for (uint32_t e = tid0; e < kMlpBaseBlock; e += kMlpBaseThreads) grads[kMlpBaseFcHAt + e] = 0.0f;

    for (uint64_t base = begin; base < end; base += kMlpBaseTile) {
        const bool first = base == begin;
        const uint32_t tid = opaque(tid0), lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
        // ---- the tile's samples; a lane past the end runs on a zero observation with zero upstream gradient
        if (tid < kMlpBaseTile) {
            uint32_t s = 0xFFFFFFFFu;
            if (base + tid < end) {
                s = (uint32_t)a.indices[base + tid];
                s = s < a.batch_size ? s : a.batch_size - 1u;  // outside the contract, but memory-safe
            }
            sample[tid] = s;
        }
        __syncthreads();
        {
            const uint32_t rr = tid >> 3, k = tid & 7u, s = sample[rr];
            xhat0[rr * kMlpLd0 + k] = s != 0xFFFFFFFFu && k < kMlpBaseObs ? (float)a.obs[(size_t)s * kMlpBaseObs + k] : 0.0f;
        }
        __syncthreads();
        // ---- the forward pass of mrl_mlpbase_act
        mlpbase_forward(params, layer_N, out_dim, lds, wave, lane);

        // ---- the loss head, a lane per sample: d_out = dLoss / d(head output)
        if (tid < kMlpBaseTile) {
            float d[kMlpBaseActions] = {0.0f, 0.0f, 0.0f, 0.0f};
            const uint32_t at = sample[tid];
            if (at != 0xFFFFFFFFu && net == 0u) {
                const float lg[kMlpBaseActions] = {outs[tid * 8u], outs[tid * 8u + 1], outs[tid * 8u + 2], outs[tid * 8u + 3]};
                mappo_actor_sample<(int)kMlpBaseActions>(lg, a.actions[at], a.logprobs[at], a.advantages[at], a.loss, count, d, stat);
            } else if (at != 0xFFFFFFFFu) {
                d[0] = mappo_critic_sample(outs[tid * 8u], a.value_preds[at], a.returns[at], a.row_norm, a.loss, count, stat);
            }
#pragma unroll
            for (int i = 0; i < (int)kMlpBaseActions; i++) d_out[tid * 8u + i] = d[i];
#pragma unroll
            for (int i = (int)kMlpBaseActions; i < 8; i++) d_out[tid * 8u + i] = 0.0f;
        }
        __syncthreads();

        // ---- head: dW_head = d_out^T y (rows: outputs, k: samples) on waves 0 and 1, a 32-column slab each; db_head; dy
        {
            const float *__restrict__ y = lds + kMlpYAt + layer_N * kMlpBaseTile * kMlpLd;
            if (wave < 2u) {
                const uint32_t col = 32u * wave + r;
                mappo_f32x16 acc = acc_load(g_head_w, kMlpBaseHidden, out_dim, col, true, first, half);
#pragma unroll 4
                for (uint32_t kk = 0; kk < kMlpBaseTile / 2u; kk++) {
                    const uint32_t s = 2u * kk + half;
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(r < out_dim ? d_out[s * 8u + r] : 0.0f, y[s * kMlpLd + col], acc, 0, 0, 0);
                }
                acc_store(g_head_w, kMlpBaseHidden, out_dim, col, true, half, acc);
            } else if (wave == 2u && lane < out_dim) {
                column_sum(g_head_b, first, d_out, nullptr, 8u, 0u, lane);
            }
            for (uint32_t idx = tid; idx < kMlpBaseTile * kMlpBaseHidden; idx += kMlpBaseThreads) {
                const uint32_t s = idx >> 6, j = idx & 63u;
                float sum = 0.0f;
                for (uint32_t o = 0; o < out_dim; o++) sum = fmaf(head_w[o * kMlpBaseHidden + j], d_out[s * 8u + o], sum);
                dy[s * kMlpLd + j] = sum;
            }
        }
        __syncthreads();

        // ---- the hidden layers, last to first: h = 0 is fc1, h >= 1 is fc2[h - 1]
#pragma unroll 1
        for (uint32_t hh = 0; hh <= layer_N; hh++) {
            const uint32_t h = layer_N - hh, K = h ? kMlpBaseHidden : kMlpBaseObs;
            const float *__restrict__ w = params + mlpbase_layer_at(h), *__restrict__ ln_w = w + kMlpBaseHidden * K + kMlpBaseHidden;
            float *__restrict__ g_w = grads + mlpbase_layer_at(h), *__restrict__ g_b = g_w + kMlpBaseHidden * K;
            float *__restrict__ g_ln_w = g_b + kMlpBaseHidden, *__restrict__ g_ln_b = g_ln_w + kMlpBaseHidden;
            const float *__restrict__ xhat = lds + kMlpXhatAt + h * kMlpBaseTile * kMlpLd;
            // LayerNorm and ReLU: dz = (ReLU passed) rstd (g - mean(g) - xhat mean(g xhat)), g = dy weight; a wavefront per row
            {
                const float weight = ln_w[lane];
                for (uint32_t row = wave; row < kMlpBaseTile; row += 4u) {
                    const float xh = xhat[row * kMlpLd + lane], g = dy[row * kMlpLd + lane] * weight;
                    const float mean_g = wave_sum(g) / (float)kMlpBaseHidden, mean_gx = wave_sum(g * xh) / (float)kMlpBaseHidden;
                    const float dx = rstd[(h + 1u) * kMlpBaseTile + row] * ((g - mean_g) - xh * mean_gx);
                    dz[row * kMlpLd + lane] = (mask[h * kMlpBaseTile + row] >> lane) & 1ull ? dx : 0.0f;
                }
                if (wave == 0u)
                    column_sum(g_ln_w, first, dy, xhat, kMlpLd, kMlpLd, lane);
                else if (wave == 1u)
                    column_sum(g_ln_b, first, dy, nullptr, kMlpLd, 0u, lane);
            }
            __syncthreads();  // dz is complete, dy is dead
            if (h) {
                // dW = dz^T in (64 x 64), one 32 x 32 block per wave, k = samples
                const float *__restrict__ in = lds + kMlpYAt + (h - 1u) * kMlpBaseTile * kMlpLd;
                {
                    const uint32_t jt = wave >> 1, it = wave & 1u, col = 32u * it + r;
                    float *__restrict__ g = g_w + (size_t)32u * jt * kMlpBaseHidden;
                    mappo_f32x16 acc = acc_load(g, kMlpBaseHidden, 32u, col, true, first, half);
#pragma unroll 4
                    for (uint32_t kk = 0; kk < kMlpBaseTile / 2u; kk++) {
                        const uint32_t s = 2u * kk + half;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[s * kMlpLd + 32u * jt + r], in[s * kMlpLd + col], acc, 0, 0, 0);
                    }
                    acc_store(g, kMlpBaseHidden, 32u, col, true, half, acc);
                }
                // dy[sample][i] of the layer below = sum_j dz[sample][j] W[j][i]: rows samples, k = this layer's units; waves 0 and 1
                if (wave < 2u) {
                    const uint32_t col = 32u * wave + r;
                    mappo_f32x16 acc;
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 4
                    for (uint32_t kk = 0; kk < kMlpBaseHidden / 2u; kk++) {
                        const uint32_t j = 2u * kk + half;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[r * kMlpLd + j], w[j * kMlpBaseHidden + col], acc, 0, 0, 0);
                    }
#pragma unroll
                    for (int e = 0; e < 16; e++) dy[tile_row(e, half) * kMlpLd + col] = acc[e];
                } else if (wave == 2u) {
                    column_sum(g_b, first, dz, nullptr, kMlpLd, 0u, lane);
                }
            } else {
                // fc1: dW = dz^T in0 (64 x 7), waves 0 and 1 a 32-row block each, columns past 7 idle; db; dy of feature_norm
                if (wave < 2u) {
                    const bool ok = r < kMlpBaseObs;
                    float *__restrict__ g = g_w + (size_t)32u * wave * kMlpBaseObs;
                    mappo_f32x16 acc = acc_load(g, kMlpBaseObs, 32u, r, ok, first, half);
#pragma unroll 4
                    for (uint32_t kk = 0; kk < kMlpBaseTile / 2u; kk++) {
                        const uint32_t s = 2u * kk + half;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(dz[s * kMlpLd + 32u * wave + r], ok ? in0[s * kMlpLd0 + r] : 0.0f, acc, 0, 0, 0);
                    }
                    acc_store(g, kMlpBaseObs, 32u, r, ok, half, acc);
                } else if (wave == 2u) {
                    column_sum(g_b, first, dz, nullptr, kMlpLd, 0u, lane);
                }
                for (uint32_t idx = tid; idx < kMlpBaseTile * kMlpBaseObs; idx += kMlpBaseThreads) {
                    const uint32_t s = idx / kMlpBaseObs, i = idx - s * kMlpBaseObs;
                    float sum = 0.0f;
                    for (uint32_t j = 0; j < kMlpBaseHidden; j++) sum = fmaf(w[j * kMlpBaseObs + i], dz[s * kMlpLd + j], sum);
                    dy[s * kMlpLd + i] = sum;
                }
            }
            __syncthreads();  // dy of the layer below is complete, dz is dead
        }

        // ---- feature_norm: dweight = sum dy xhat0, dbias = sum dy (nothing lies below it)
        if (wave == 0u && lane < kMlpBaseObs)
            column_sum(grads, first, dy, xhat0, kMlpLd, kMlpLd0, lane);
        else if (wave == 1u && lane < kMlpBaseObs)
            column_sum(grads + kMlpBaseObs, first, dy, nullptr, kMlpLd, 0u, lane);
        __syncthreads();  // the next tile overwrites what the sums above read
    }

    // ---- the stats' sums: lanes in ascending order
    const uint32_t tid = tid0;
    double *sums = reinterpret_cast<double *>(lds);
    if (tid < kMlpBaseTile) {
#pragma unroll
        for (int c = 0; c < 4; c++) sums[c * kMlpBaseTile + tid] = stat[c];
    }
    __syncthreads();
    if (tid < kMappoStats) {
        double sum = 0.0;
        if (tid < 4u)
            for (uint32_t s = 0; s < kMlpBaseTile; s++) sum += sums[tid * kMlpBaseTile + s];
        a.partial_stats[((size_t)net * a.groups + blockIdx.x) * kMappoStats + tid] = sum;
    }
}

}  // namespace

void launch_mappo_mlp_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_batch &batch, const int32_t *indices,
                             uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                             float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    const uint32_t actor = mlpbase_net_params(layer_N, kMlpBaseActions), critic = mlpbase_net_params(layer_N, 1);
    const SampleShare share = share_samples(minibatch_size, kMlpBaseTile, kMappoMaxGroups);
    const MappoWorkspace ws = mappo_workspace(actor, minibatch_size, num_minibatches);
    const bool norm = cfg.flags & MRL_MAPPO_VALUENORM;
    if (norm)
        launch_mappo_value_norm(batch.returns, indices, num_minibatches, minibatch_size, batch.size, cfg, value_norm_state,
                                workspace + ws.row_sums, workspace + ws.row_norm, stream);
    constexpr uint32_t lds_bytes = kMlpUpdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mappo_mlp_grad>(lds_bytes);
    MappoMlpGradArgs g{};
    g.params = opt.params_dev;
    g.obs = batch.obs;
    g.actions = batch.actions;
    g.logprobs = batch.logprobs;
    g.value_preds = batch.value_preds;
    g.returns = batch.returns;
    g.advantages = batch.advantages;
    g.partial_grads = workspace + ws.partial_grads;
    g.partial_stats = reinterpret_cast<double *>(workspace + ws.partial_stats);
    g.share = share.share;
    g.stride = ws.stride;
    g.minibatch_size = minibatch_size;
    g.batch_size = batch.size;
    g.groups = share.groups;
    g.layer_N = layer_N;
    g.loss = MappoLoss{cfg.clip_param, cfg.entropy_coef, cfg.value_loss_coef, cfg.huber_delta, cfg.flags};
    // two clip_grad_norm_ and two Adam steps: the actor's segment, then the critic's
    AdamStepArgs ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.opti_eps, cfg.flags & MRL_MAPPO_MAX_GRAD_NORM, cfg.max_grad_norm);
    ad.partial_grads = g.partial_grads;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = ws.stride;
    ad.segments = 2;
    ad.groups = share.groups;
    ad.blocks = (uint32_t)ws.blocks;
    ad.num_params[0] = actor, ad.num_params[1] = critic;
    ad.at[0] = 0, ad.at[1] = actor;
    MappoStatsRow row{g.partial_stats, nullptr, share.groups, minibatch_size};
    for (uint32_t k = 0; k < num_minibatches; k++) {
        g.indices = indices + (size_t)k * minibatch_size;
        g.row_norm = norm ? workspace + ws.row_norm + 2 * (size_t)k : nullptr;
        hipLaunchKernelGGL(mrl_mappo_mlp_grad, dim3(share.groups, 2), dim3(kMlpBaseThreads), lds_bytes, stream, g);
        MRL_HIP(hipGetLastError());
        ad.grads_row = grads ? grads + (size_t)k * ((size_t)actor + critic) : nullptr;
        adam_set_step(ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.critic_lr});
        row.row = stats ? stats + (size_t)k * kMappoStats : nullptr;
        launch_adam_step(ad, row, stream);
    }
}

}  // namespace mrl
