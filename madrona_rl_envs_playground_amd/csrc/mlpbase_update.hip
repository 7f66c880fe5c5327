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
// mrl_mappo_mlp_bank_update is the same launches with a third grid dimension, the member of the bank: a
// member's workgroups read its own parameters, indices and ValueNorm rows and write its own partial vectors (the kernels'
// MEMBERS = true instances; the plain update runs the MEMBERS = false ones, which are the kernels as they were).
// The sample table, the loss head, the head's and a Linear(64, 64)'s backward pass, the column sums, the stats' tail and the host's
// row loop are mappo_grad.hpp's, shared with mrl_mappo_grad; what is left here is what a LayerNorm MLP has of its own.
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run.
#include "mlpbase_update.hpp"
#include "mlpbase_forward.hpp"
#include "mappo_grad.hpp"

namespace mrl {

namespace {

static_assert(kMlpBaseHidden == kMappoHidden && kMlpBaseThreads == kMappoThreads && kMlpBaseTile == kMappoTile && kMlpLd == kMappoLd,
              "mappo_grad.hpp's functions are written for this net's width, workgroup, tile and LDS row stride");

extern __shared__ __attribute__((aligned(16))) unsigned char mlp_upd_lds_image[];

struct MappoMlpGradArgs {
    MappoGradCommon common;  // obs: int32 (S, 7)
    const float *params;
    uint32_t layer_N;
    MappoMemberStrides members;  // MEMBERS only
};

// MEMBERS: member blockIdx.z of a bank update, on its own parameters, indices, ValueNorm rows and partial vectors
template <bool MEMBERS>
__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mappo_mlp_grad(MappoMlpGradArgs a)
{
    const MappoGradCommon own = MEMBERS ? mappo_member_view(a.common, a.members) : MappoGradCommon{};
    const MappoGradCommon &c = MEMBERS ? own : a.common;
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x, layer_N = a.layer_N, out_dim = net ? 1u : kMlpBaseActions;
    const uint32_t net_at = net ? mlpbase_net_params(layer_N, kMlpBaseActions) : 0u;
    const float *__restrict__ params = a.params + (MEMBERS ? (size_t)blockIdx.z * a.members.params : 0) + net_at;
    // this workgroup's partial vector, in the net's parameter order
    float *__restrict__ grads = c.partial_grads + ((size_t)net * c.groups + blockIdx.x) * c.stride;
    const float *__restrict__ head_w = params + mlpbase_head_at(layer_N);
    float *__restrict__ g_head_w = grads + mlpbase_head_at(layer_N), *__restrict__ g_head_b = g_head_w + out_dim * kMlpBaseHidden;

    float *lds = reinterpret_cast<float *>(mlp_upd_lds_image);
    float *in0 = lds + kMlpIn0At, *xhat0 = lds + kMlpXhat0At, *rstd = lds + kMlpRstdAt, *outs = lds + kMlpOutAt;
    const unsigned long long *mask = reinterpret_cast<const unsigned long long *>(lds + kMlpMaskAt);
    float *d_out = lds + kMlpDoutAt, *dy = lds + kMlpDyAt, *dz = lds + kMlpDzAt;
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + kMlpSampleAt);

    const int32_t *__restrict__ obs = static_cast<const int32_t *>(c.obs);
    const uint64_t begin = blockIdx.x * c.share;
    const uint64_t end = begin + c.share < c.minibatch_size ? begin + c.share : c.minibatch_size;
    const float count = (float)c.minibatch_size;
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    // fc_h: no forward pass reads it, so its gradient is zero
    for (uint32_t e = tid0; e < kMlpBaseBlock; e += kMlpBaseThreads) grads[kMlpBaseFcHAt + e] = 0.0f;

    for (uint64_t base = begin; base < end; base += kMlpBaseTile) {
        const bool first = base == begin;
        const uint32_t tid = opaque(tid0), lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
        mappo_tile_samples(c, sample, base, end, tid);
        __syncthreads();
        {
            const uint32_t rr = tid >> 3, k = tid & 7u, s = sample[rr];
            xhat0[rr * kMlpLd0 + k] = s != kMappoAbsent && k < kMlpBaseObs ? (float)obs[(size_t)s * kMlpBaseObs + k] : 0.0f;
        }
        __syncthreads();
        // ---- the forward pass of mrl_mlpbase_act
        mlpbase_forward(params, layer_N, out_dim, lds, wave, lane);

        mappo_loss_head<(int)kMlpBaseActions>(c, net, sample, outs, d_out, count, stat, tid);
        __syncthreads();
        // ---- head: dW_head, db_head and dy of the last hidden layer
        mappo_head_backward<false>(head_w, g_head_w, g_head_b, out_dim, d_out, lds + kMlpYAt + layer_N * kMlpBaseTile * kMlpLd, dy, nullptr,
                                   kMlpLd, first, tid);
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
                // dW = dz^T in (64 x 64); dy of the layer below on waves 0 and 1; db
                mappo_dw_block(g_w, dz, lds + kMlpYAt + (h - 1u) * kMlpBaseTile * kMlpLd, kMlpLd, first, wave, r, half);
                if (wave < 2u)
                    mappo_d_in<false>(dz, w, dy, nullptr, kMlpLd, wave, r, half);
                else if (wave == 2u)
                    column_sum(g_b, first, dz, nullptr, kMlpLd, 0u, lane);
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

    mappo_stats_tail(c, net, reinterpret_cast<double *>(lds), stat, tid0);
}

}  // namespace

void launch_mappo_mlp_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_batch &batch, const int32_t *indices,
                             uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                             float *workspace, float *stats, float *grads, hipStream_t stream, const MappoMembers &members)
{
    if (num_minibatches == 0) return;
    constexpr uint32_t lds_bytes = kMlpUpdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mappo_mlp_grad<false>>(lds_bytes);
    allow_large_dynamic_lds<&mrl_mappo_mlp_grad<true>>(lds_bytes);
    MappoMlpGradArgs g{};
    g.params = opt.params_dev;
    g.layer_N = layer_N;
    mappo_update_rows(mlpbase_net_params(layer_N, kMlpBaseActions), mlpbase_net_params(layer_N, 1), opt, batch, indices, num_minibatches,
                      minibatch_size, cfg, value_norm_state, workspace, stats, grads, stream, members,
                      [&](const MappoGradCommon &common, uint32_t groups, const MappoMemberStrides &strides, uint32_t count) {
                          g.common = common;
                          g.members = strides;
                          if (count == 1)
                              hipLaunchKernelGGL(mrl_mappo_mlp_grad<false>, dim3(groups, 2), dim3(kMlpBaseThreads), lds_bytes, stream, g);
                          else
                              hipLaunchKernelGGL(mrl_mappo_mlp_grad<true>, dim3(groups, 2, count), dim3(kMlpBaseThreads), lds_bytes, stream, g);
                      });
}

}  // namespace mrl
