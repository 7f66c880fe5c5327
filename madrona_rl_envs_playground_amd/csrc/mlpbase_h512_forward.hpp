// The layers of the hidden-512 MLPBase actor-critic as device functions: how mrl_mlpbase_act_h512 (mlpbase_h512.hip) multiplies,
// stores and normalises a layer.  The update's forward pass (mlpbase_h512_update.hip) runs the same functions, so that it recomputes
// the act's values and log-probabilities bit for bit.  The sums' order is stated in mlpbase_h512.hpp.
#pragma once

#include "cnn_h512_forward.hpp"
#include "mlpbase_forward.hpp"
#include "mlpbase_h512.hpp"

namespace mrl {

// the products of 8 consecutive k, from k on: four matrix instructions per (column block, row block), k ascending.  a_row: this
// lane's LDS row of row block 0 from its own first k (row r, k = half); row block rb lies 32 rows of `ld` floats further.
template <int RB>
__device__ __forceinline__ void mlp512_multiply(const float *__restrict__ a_row, uint32_t ld, uint32_t k, const f32x4u (&b)[4][2], bool odd,
                                                f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        float av[RB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++) av[rb] = a_row[rb * 32u * ld + k + 2u * s];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float bv = odd ? b[j][s >> 1][2 * (s & 1) + 1] : b[j][s >> 1][2 * (s & 1)];
#pragma unroll
            for (int rb = 0; rb < RB; rb++) acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb], bv, acc[rb][j], 0, 0, 0);
        }
    }
}

// acc[rb][j][row][column r of block j] = sum over k < 512 of h[32 rb + row][k] * w_row[j][k], one chain from 0, k ascending
template <int RB>
__device__ __forceinline__ void mlp512_products(const float *__restrict__ a_row, const float *const (&w_row)[4], bool odd, f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[rb][j][e] = 0.0f;
    f32x4u b0[4][2], b1[4][2];
    h512_fetch<4>(w_row, 0u, b0);
    for (uint32_t k = 0; k < kMlpH512Hidden; k += 16u) {
        h512_fetch<4>(w_row, k + 8u, b1);
        mlp512_multiply<RB>(a_row, kMlpH512Ld, k, b0, odd, acc);
        if (k + 16u < kMlpH512Hidden) h512_fetch<4>(w_row, k + 16u, b0);
        mlp512_multiply<RB>(a_row, kMlpH512Ld, k + 8u, b1, odd, acc);
    }
}

// fc1: acc = in0 (rows of 9 floats, column 7 zero) times the (512, 7) weight, k = 0 .. 7 with w[.][7] = 0
template <int RB>
__device__ __forceinline__ void mlp512_fc1(const float *__restrict__ in0, const float *__restrict__ w, uint32_t wave, uint32_t r, uint32_t half,
                                           f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float *__restrict__ row = w + ((wave * 4u + j) * 32u + r) * kMlpBaseObs;
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[rb][j][e] = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t k = 2u * s + half;
            const float bv = k < kMlpBaseObs ? row[k] : 0.0f;
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
                acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(in0[(rb * 32u + r) * kMlpLd0 + k], bv, acc[rb][j], 0, 0, 0);
        }
    }
}

// relu(acc + bias) of the lane's column of each block into h, by the C/D map of the 32 x 32 tile
template <int RB>
__device__ __forceinline__ void mlp512_store(const f32x16 (&acc)[RB][4], const float *__restrict__ bias, float *__restrict__ h, uint32_t wave,
                                             uint32_t r, uint32_t half)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t col = (wave * 4u + j) * 32u + r;
        const float b = bias[col];
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const uint32_t row = rb * 32u + (e & 3) + 8 * (e >> 2) + 4 * half;
                const float v = acc[rb][j][e] + b;
                h[row * kMlpH512Ld + col] = v > 0.0f ? v : 0.0f;
            }
    }
}

// LayerNorm over `rows` rows of D = 7 (J = 1) or 512 (J = 8) columns in place, a wavefront per row (wave w takes rows w, w + 4,
// ...), lane l the columns l + 64 j, j < J.  The sums' order is mlpbase_h512.hpp's.  With D = 7 lane 7 writes the zero the padded
// product reads.  STATS (the update's forward pass): the row's (mean, rstd) go to stats[2 row], stats[2 row + 1]; the act's
// instance is the function without them.  Ends behind a barrier.
template <int J, bool STATS = false>
__device__ __forceinline__ void mlp512_layer_norm(float *__restrict__ x, uint32_t ld, uint32_t rows, uint32_t D, const float *__restrict__ weight,
                                                  const float *__restrict__ bias, uint32_t wave, uint32_t lane, float *stats = nullptr)
{
    float w[J], b[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint32_t col = lane + 64u * j;
        w[j] = col < D ? weight[col] : 0.0f, b[j] = col < D ? bias[col] : 0.0f;
    }
    const float count = (float)D;
    for (uint32_t row = wave; row < rows; row += 4u) {
        float v[J], sum = 0.0f;
#pragma unroll
        for (int j = 0; j < J; j++) {
            const uint32_t col = lane + 64u * j;
            v[j] = col < D ? x[row * ld + col] : 0.0f;
            sum += v[j];
        }
        const float mean = wave_sum(sum) / count;
        float squares = 0.0f;
#pragma unroll
        for (int j = 0; j < J; j++) {
            v[j] = lane + 64u * j < D ? v[j] - mean : 0.0f;
            squares += v[j] * v[j];
        }
        const float rstd = 1.0f / sqrtf(wave_sum(squares) / count + kMlpBaseLnEps);
        if constexpr (STATS) {
            if (lane == 0u) stats[2u * row] = mean, stats[2u * row + 1u] = rstd;
        }
#pragma unroll
        for (int j = 0; j < J; j++) {
            const uint32_t col = lane + 64u * j;
            if (col < D)
                x[row * ld + col] = (v[j] * rstd) * w[j] + b[j];
            else if (col == D && (D & 1u))
                x[row * ld + col] = 0.0f;
        }
    }
    __syncthreads();
}

}  // namespace mrl
