// The backward pass of MLPBase's base (mlpbase_update.hip describes the arithmetic) as a device function: from dL/d(the last
// hidden layer's LayerNorm output) in `dy` through every hidden layer, last to first, down to feature_norm, on top of the image
// mlpbase_forward left in LDS.  The recurrent mrl_mappo_gru_grad (mlpbase_gru_update.hip) runs it once per step of a chunk.  It is
// the body of mrl_mappo_mlp_grad's tile loop, statement for statement; that kernel keeps its own copy in line, because calling
// this function from there changes its register allocation and the plain update must compile to the instructions it had.  The
// accumulators live in the workgroup's partial vector `grads`, in the net's parameter order (`first`: nothing has been
// accumulated yet).  dy and dz are two 32 x 64 LDS arrays (rows 65 apart) that take turns; both are dead afterwards.  Ends behind
// a barrier.
#pragma once

#include "mappo_grad.hpp"
#include "mlpbase_forward.hpp"

namespace mrl {

__device__ __forceinline__ void mlpbase_backward(const float *__restrict__ params, float *__restrict__ grads, uint32_t layer_N, float *lds,
                                                 float *dy, float *dz, bool first, uint32_t tid)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    float *in0 = lds + kMlpIn0At, *xhat0 = lds + kMlpXhat0At, *rstd = lds + kMlpRstdAt;
    const unsigned long long *mask = reinterpret_cast<const unsigned long long *>(lds + kMlpMaskAt);
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

}  // namespace mrl
