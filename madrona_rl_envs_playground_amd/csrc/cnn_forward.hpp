// The forward pass of MAPPO's CNN actor-critic as device functions: the convolution and the linear layers of mrl_cnn_act
// (cnn_policy.hip; the operand maps are described there), shared with the update's gradient kernel (cnn_update.hip), which must
// recompute the act's values and log-probabilities bit for bit.
#pragma once

#include "cnn_policy.hpp"

namespace mrl {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// A tile's 32 observation rows into LDS, whole dwords from the 4-byte boundary at or below each row's start: LDS row rr holds the
// row's bytes from byte `shift` on, and the first and the last dword are put together from the row's own bytes only.
// row_address(rr) is the row's first byte, or nullptr for a row the tile does not have (zeros).  With `shifts`, shifts[rr]
// receives the row's shift.  Then the patch offset of every k and, with_weights, the conv weights, rows conv_ld floats apart and
// a zero behind an odd K.  The caller puts a barrier behind it.
template <class RowAddress>
__device__ __forceinline__ void cnn_load_tile(const CnnActArgs &a, unsigned char *lds, const RowAddress &row_address, uint32_t *shifts,
                                              const float *__restrict__ conv_w, bool with_weights)
{
    const CnnLds &l = a.lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t S = a.W * a.H * a.F, k1 = l.k1;
    uint32_t *obs_words = reinterpret_cast<uint32_t *>(lds);
    for (uint32_t rr = wave; rr < kCnnTile; rr += 4u) {
        uint32_t *__restrict__ dst = obs_words + rr * (l.obs_ld / 4u);
        const uint8_t *__restrict__ row = row_address(rr);
        if (!row) {
            for (uint32_t d = lane; d < (S + 3u) / 4u; d += 64u) dst[d] = 0u;
            if (shifts && lane == 0) shifts[rr] = 0u;
            continue;
        }
        const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(row) & 3u), words = (shift + S + 3u) / 4u;
        if (shifts && lane == 0) shifts[rr] = shift;
        for (uint32_t d = lane; d < words; d += 64u) {
            const int32_t g = (int32_t)(4u * d) - (int32_t)shift;  // the dword's first byte, counted from the row's start
            uint32_t v = 0u;
            if (g >= 0 && (uint32_t)g + 4u <= S) {
                v = *reinterpret_cast<const uint32_t *>(row + g);
            } else {
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int32_t at = g + b;
                    if (at >= 0 && (uint32_t)at < S) v |= (uint32_t)row[at] << (8 * b);
                }
            }
            dst[d] = v;
        }
    }
    if (with_weights) {
        float *w_lds = reinterpret_cast<float *>(lds + l.conv_w_at);
        for (uint32_t e = tid; e < kCnnChannels * k1; e += kCnnThreads) {
            const uint32_t c = e / k1, k = e - c * k1;
            w_lds[c * l.conv_ld + k] = conv_w[e];
        }
        if (k1 != l.k1_padded && tid < kCnnChannels) w_lds[tid * l.conv_ld + k1] = 0.0f;
    }
    uint16_t *koff = reinterpret_cast<uint16_t *>(lds + l.koff_at);
    for (uint32_t k = tid; k < l.k1_padded; k += kCnnThreads) {
        const uint32_t f = k / 9u, ij = k - 9u * f, i = ij / 3u, j = ij - 3u * i;
        koff[k] = k < k1 ? (uint16_t)((j * a.W + i) * a.F + f) : (uint16_t)0;
    }
}

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

// The convolution of a tile cnn_load_tile left in LDS, into the activation image: wave w takes positions w, w + 4, ..., three at a
// time.  `shift`: where the row of this lane's sample r begins in its LDS row.  The caller puts a barrier behind it.
__device__ __forceinline__ void cnn_conv_tile(const CnnActArgs &a, unsigned char *lds, uint32_t shift, const float *__restrict__ conv_b,
                                              uint32_t wave, uint32_t r, uint32_t half)
{
    const int8_t *__restrict__ my_obs = reinterpret_cast<const int8_t *>(lds) + r * a.lds.obs_ld + shift;
    const float *__restrict__ my_w = reinterpret_cast<const float *>(lds + a.lds.conv_w_at) + r * a.lds.conv_ld;
    const uint16_t *koff = reinterpret_cast<const uint16_t *>(lds + a.lds.koff_at);
    float *act = reinterpret_cast<float *>(lds + a.lds.act_at);
    const float bias = conv_b[r];
    const uint32_t npos = a.lds.npos;
    for (uint32_t p0 = wave; p0 < npos; p0 += 12u) {
        const uint32_t count = (npos - p0 + 3u) / 4u;  // positions p0, p0 + 4, p0 + 8 that exist
        if (count >= 3u)
            cnn_conv_pass<3>(a, my_obs, my_w, koff, act, bias, p0, r, half);
        else if (count == 2u)
            cnn_conv_pass<2>(a, my_obs, my_w, koff, act, bias, p0, r, half);
        else
            cnn_conv_pass<1>(a, my_obs, my_w, koff, act, bias, p0, r, half);
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
