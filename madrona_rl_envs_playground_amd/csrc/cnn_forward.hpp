// The forward pass of MAPPO's CNN actor-critic as device functions: the convolution and the linear layers of mrl_cnn_act
// (cnn_policy.hip; the operand maps are described there), shared with the update's gradient kernel (cnn_update.hip), which must
// recompute the act's values and log-probabilities bit for bit.
#pragma once

#include "cnn_policy.hpp"

namespace mrl {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int NP>
__device__ __forceinline__ void cnn_conv_pass(const CnnActArgs &a, const int8_t *__restrict__ my_obs, const float *__restrict__ my_w,
                                              const uint16_t *__restrict__ koff, float *__restrict__ act, float bias, uint32_t p0,
                                              uint32_t r, uint32_t half)
{
    const uint32_t hh = a.H - 2u;
    uint32_t base[NP];
    f32x16 acc[NP];
#pragma unroll
    for (int q = 0; q < NP; q++) {
        const uint32_t pos = p0 + 4u * q, ow = pos / hh, oh = pos - ow * hh;
        base[q] = (oh * a.W + ow) * a.F;
#pragma unroll
        for (int e = 0; e < 16; e++) acc[q][e] = 0.0f;
    }
    const uint32_t steps = a.lds.k1_padded / 2u;
    for (uint32_t kk = 0; kk < steps; kk++) {
        const uint32_t k = 2u * kk + half, off = koff[k];
        const float b = my_w[k];
#pragma unroll
        for (int q = 0; q < NP; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32((float)my_obs[base[q] + off], b, acc[q], 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < NP; q++) {
        float *__restrict__ out = act + r * a.lds.npos + p0 + 4u * q;
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t row = (e & 3) + 8 * (e >> 2) + 4 * half;  // C/D map of the 32 x 32 tile
            const float v = acc[q][e] + bias;
            out[row * a.lds.act_ld] = v > 0.0f ? v : 0.0f;
        }
    }
}

__device__ __forceinline__ void cnn_fetch(const float *__restrict__ w, uint32_t K, uint32_t out_dim, uint32_t k, uint32_t wave,
                                          float (&pb)[16])
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t col = wave + 4u * i;
        pb[i] = col < out_dim && k < K ? w[(size_t)col * K + k] : 0.0f;
    }
}

// out[row][col] = act(bias[col] + sum_k in[row][k] w[col][k]) for the tile's 32 rows; ends behind a barrier.  K is the weight
// rows' stride and the number of products; an odd K (the balance beam's 7 inputs) takes one more product, a zero weight times
// in[row][K], which the caller keeps at 0.  An even K -- every layer of the kitchens -- runs the steps it always ran.
__device__ __forceinline__ void cnn_fc_layer(const float *__restrict__ in, uint32_t in_ld, uint32_t K, const float *__restrict__ w,
                                             const float *__restrict__ bias, uint32_t out_dim, bool relu, float *__restrict__ chunk,
                                             float *__restrict__ out, uint32_t out_ld, uint32_t wave, uint32_t lane)
{
    const uint32_t r = lane & 31u, half = lane >> 5;
    const bool compute = wave * 32u < out_dim;
    float pb[16];
    cnn_fetch(w, K, out_dim, lane, wave, pb);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
    for (uint32_t k0 = 0; k0 < K; k0 += kCnnChunk) {
#pragma unroll
        for (int i = 0; i < 16; i++) chunk[(wave + 4u * i) * kCnnFcLd + lane] = pb[i];
        __syncthreads();
        if (k0 + kCnnChunk < K) cnn_fetch(w, K, out_dim, k0 + kCnnChunk + lane, wave, pb);
        if (compute) {
            const uint32_t left = K - k0, steps = left >= kCnnChunk ? kCnnChunk / 2u : (left + 1u) / 2u;
            const float *__restrict__ pa_lds = in + r * in_ld + k0 + half;
            const float *__restrict__ pb_lds = chunk + (wave * 32u + r) * kCnnFcLd + half;
            for (uint32_t s = 0; s < steps; s++) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa_lds[2u * s], pb_lds[2u * s], acc, 0, 0, 0);
        }
        __syncthreads();  // the next chunk overwrites what the products read
    }
    const uint32_t col = wave * 32u + r;
    if (compute && col < out_dim) {
        const float b = bias[col];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t row = (e & 3) + 8 * (e >> 2) + 4 * half;
            const float v = acc[e] + b;
            out[row * out_ld + col] = relu ? (v > 0.0f ? v : 0.0f) : v;
        }
    }
    __syncthreads();
}

}  // namespace mrl
