// The forward pass of MAPPO's MLPBase actor-critic as device functions: what mrl_mlpbase_act (mlpbase_policy.hip) runs, shared
// with the update's gradient kernel (mlpbase_update.hip), which must recompute the act's values and log-probabilities bit for bit
// and reads what the pass leaves in LDS (the index map and the LDS image are in mlpbase_policy.hpp).
#pragma once

#include "cnn_forward.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

// The sum of one value per lane over the wavefront, in ONE fixed order: six exchange steps, partners 32, 16, 8, 4, 2 and 1 lanes
// apart, each lane adding its partner's partial sum to its own.  Floating-point addition commutes, so after every step the two
// partners hold the same bits and at the end all 64 lanes hold the same sum: ((((((v[l] + v[l ^ 32]) + ..) for every lane l.
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int apart = 32; apart > 0; apart >>= 1) v += __shfl_xor(v, apart);
    return v;
}

// LayerNorm over the tile's 32 rows of D <= 64 columns, a wavefront per row (wave w takes rows w, w + 4, ...), lane j column j.
// Two passes over registers: mean = wave_sum(x) / D, then var = wave_sum((x - mean)^2) / D (the biased variance), rstd = 1 /
// sqrtf(var + 1e-5); lanes past D add 0.  `x` holds the rows and receives the normalised rows (x - mean) * rstd in place; `y`
// receives normalised * weight + bias, and a 0 in column D where D is odd (the next layer's padded product reads it).  rstd[row]
// and, with `mask`, the 64-bit word of the lanes whose x was positive (the ReLU in front passed them) are kept for the backward
// pass.  Ends behind a barrier.
__device__ __forceinline__ void mlpbase_layer_norm(float *__restrict__ x, float *__restrict__ y, uint32_t ld, uint32_t D,
                                                   const float *__restrict__ weight, const float *__restrict__ bias, float *__restrict__ rstd,
                                                   unsigned long long *__restrict__ mask, uint32_t wave, uint32_t lane)
{
    const bool live = lane < D;
    const float w = live ? weight[lane] : 0.0f, b = live ? bias[lane] : 0.0f, count = (float)D;
    for (uint32_t row = wave; row < kMlpBaseTile; row += 4u) {
        const float v = live ? x[row * ld + lane] : 0.0f;
        const float mean = wave_sum(v) / count;
        const float c = live ? v - mean : 0.0f;
        const float var = wave_sum(c * c) / count;
        const float r = 1.0f / sqrtf(var + kMlpBaseLnEps);
        const float xh = c * r;
        if (live) {
            x[row * ld + lane] = xh;
            y[row * ld + lane] = xh * w + b;
        } else if (lane == D && (D & 1u)) {
            y[row * ld + lane] = 0.0f;
        }
        const unsigned long long passed = __ballot(v > 0.0f);
        if (lane == 0) {
            rstd[row] = r;
            if (mask) mask[row] = passed;
        }
    }
    __syncthreads();
}

// Both the act and the update: from the tile's observation rows as floats in xhat0 (a row past the end: zeros) to the head's
// outputs in outs (row stride 8).  `net`: the net's first parameter; out_dim 4 (actor) or 1 (critic).  HEAD = false (the recurrent
// net, mlpbase_gru.hpp, whose GRU lies between the two): the base alone, which ends with y[layer_N] behind a barrier.
template <bool HEAD = true>
__device__ __forceinline__ void mlpbase_forward(const float *__restrict__ net, uint32_t layer_N, uint32_t out_dim, float *__restrict__ lds,
                                                uint32_t wave, uint32_t lane)
{
    float *chunk = lds + kMlpChunkAt, *in0 = lds + kMlpIn0At, *xhat0 = lds + kMlpXhat0At, *rstd = lds + kMlpRstdAt, *outs = lds + kMlpOutAt;
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(lds + kMlpMaskAt);
    mlpbase_layer_norm(xhat0, in0, kMlpLd0, kMlpBaseObs, net, net + kMlpBaseObs, rstd, nullptr, wave, lane);
    const float *in = in0;
    uint32_t in_ld = kMlpLd0, K = kMlpBaseObs;
    for (uint32_t h = 0; h <= layer_N; h++) {
        const float *__restrict__ w = net + mlpbase_layer_at(h), *__restrict__ b = w + kMlpBaseHidden * K;
        float *xhat = lds + kMlpXhatAt + h * kMlpBaseTile * kMlpLd, *y = lds + kMlpYAt + h * kMlpBaseTile * kMlpLd;
        cnn_fc_layer(in, in_ld, K, w, b, kMlpBaseHidden, true, chunk, xhat, kMlpLd, wave, lane);
        mlpbase_layer_norm(xhat, y, kMlpLd, kMlpBaseHidden, b + kMlpBaseHidden, b + 2 * kMlpBaseHidden, rstd + (h + 1u) * kMlpBaseTile,
                           mask + h * kMlpBaseTile, wave, lane);
        in = y, in_ld = kMlpLd, K = kMlpBaseHidden;
    }
    if constexpr (!HEAD) return;
    const float *__restrict__ head_w = net + mlpbase_head_at(layer_N);
    cnn_fc_layer(in, in_ld, kMlpBaseHidden, head_w, head_w + out_dim * kMlpBaseHidden, out_dim, false, chunk, outs, 8u, wave, lane);
}

}  // namespace mrl
