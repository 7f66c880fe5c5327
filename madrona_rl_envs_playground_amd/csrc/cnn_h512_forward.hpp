// The products of the hidden-512 CNN actor-critic's linear layers as device functions: how mrl_cnn_act_h512 (cnn_h512.hip) fetches
// a weight row, multiplies and stores a layer.  The update's forward pass (cnn_h512_update.hip) runs the same functions, so that
// it recomputes the act's values and log-probabilities bit for bit.  The sums' order is stated in cnn_h512.hpp.
#pragma once

#include "cnn_h512.hpp"
#include "cnn_forward.hpp"

namespace mrl {

// four floats on a 4-byte boundary (the critic's tensors start 6 floats behind a multiple of 4)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// 8 consecutive k, from k on, of the weight row of each of the lane's NB columns
template <int NB>
__device__ __forceinline__ void h512_fetch(const float *const (&w_row)[NB], uint32_t k, f32x4u (&b)[NB][2])
{
#pragma unroll
    for (int j = 0; j < NB; j++) {
        b[j][0] = *reinterpret_cast<const f32x4u *>(w_row[j] + k);
        b[j][1] = *reinterpret_cast<const f32x4u *>(w_row[j] + k + 4u);
    }
}

// the products of those 8 k: four matrix instructions per column block, k ascending
template <int NB>
__device__ __forceinline__ void h512_multiply(const float *__restrict__ a_row, uint32_t k, const f32x4u (&b)[NB][2], bool odd,
                                              f32x16 (&acc)[NB])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const float av = a_row[k + 2u * s];
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const float bv = odd ? b[j][s >> 1][2 * (s & 1) + 1] : b[j][s >> 1][2 * (s & 1)];
            acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
        }
    }
}

// acc[j][row][column r of block j] += sum over k < kcount of a[row][k] * w_row[j][k], k ascending.  a_row: this lane's LDS row
// from its own first k (sample r, k = half); kcount is a multiple of 16 (32 npos, or 512).
template <int NB>
__device__ __forceinline__ void h512_products(const float *__restrict__ a_row, uint32_t kcount, const float *const (&w_row)[NB], bool odd,
                                              f32x16 (&acc)[NB])
{
    f32x4u b0[NB][2], b1[NB][2];
    h512_fetch<NB>(w_row, 0u, b0);
    for (uint32_t k = 0; k < kcount; k += 16u) {
        h512_fetch<NB>(w_row, k + 8u, b1);
        h512_multiply<NB>(a_row, k, b0, odd, acc);
        if (k + 16u < kcount) h512_fetch<NB>(w_row, k + 16u, b0);
        h512_multiply<NB>(a_row, k + 8u, b1, odd, acc);
    }
}

// act(acc + bias) of the lane's column of each block into h (rows kCnnH512HLd floats apart), by the C/D map of the 32 x 32 tile
__device__ __forceinline__ void h512_store(const f32x16 (&acc)[4], const float *__restrict__ bias, float *__restrict__ h, uint32_t wave,
                                           uint32_t r, uint32_t half)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t col = (wave * 4u + j) * 32u + r;
        const float b = bias[col];
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t row = (e & 3) + 8 * (e >> 2) + 4 * half;
            const float v = acc[j][e] + b;
            h[row * kCnnH512HLd + col] = v > 0.0f ? v : 0.0f;
        }
    }
}

}  // namespace mrl
