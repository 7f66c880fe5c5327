// One step of the reference's RNNLayer (train/MAPPO/utils/rnn.py with recurrent_N 1: a GRU of width 64 and a LayerNorm) for a tile
// of 32 samples, forward and backward, as device functions over an LDS image whose BASE the caller chooses: the balance beam's
// recurrent MLP (mlpbase_gru.hpp) keeps the image behind its forward image, the kitchens' recurrent CNN (cnn_gru.hpp) lays it
// over the convolution's dead operands.  The arithmetic is stated at the head of mlpbase_gru.hpp; both nets run these functions
// and no other, so a step has one set of bits.  DESIGN.md sections 27 and 28.
//
// The parameter block, in floats from its first: weight_ih_l0 (192, 64), weight_hh_l0 (192, 64), bias_ih_l0 (192), bias_hh_l0 (192),
// norm.weight (64), norm.bias (64); torch's gate order r, z, n.  A gradient block has the same order.
#pragma once

#include "mappo_grad.hpp"
#include "mlpbase_forward.hpp"

namespace mrl {

constexpr uint32_t kGruHidden = 64, kGruLd = kGruHidden + 1, kGruTile = 32, kGruThreads = 256;
constexpr uint32_t kGruGates = 3 * kGruHidden;                                                 // 192
constexpr uint32_t kGruParams = 2 * kGruGates * kGruHidden + 2 * kGruGates + 2 * kGruHidden;  // 25 088
constexpr uint32_t kGruWhhOff = kGruGates * kGruHidden, kGruBihOff = 2 * kGruWhhOff, kGruBhhOff = kGruBihOff + kGruGates,
                   kGruNormOff = kGruBhhOff + kGruGates;
static_assert(kGruHidden == kMappoHidden && kGruLd == kMappoLd && kGruTile == kMappoTile && kGruThreads == kMappoThreads,
              "mappo_grad.hpp's functions are written for this width, tile, workgroup and LDS row stride");

// The image, in floats from its base, rows 65 apart:
//   hin          the tile's masked incoming state rows h * m; gru_step_forward leaves h' there
//   gate[0..5]   gi_r, gi_z, gi_n, gh_r, gh_z, gh_n as the products leave them; then r, z and n in place of gi_*, gh_n stays
//   hn           h', then in place its normalised rows
//   gy           LayerNorm64(h'), the head's input
//   rstd         1 / sqrt(var + eps) of that LayerNorm per row
//   cell, keep   per row, the caller's: the sample's state row (kGruAbsent for a row the tile lacks) and its mask m
constexpr uint32_t kGruRows = kGruTile * kGruLd;
constexpr uint32_t kGruImgHin = 0, kGruImgGate = kGruImgHin + kGruRows, kGruImgHn = kGruImgGate + 6 * kGruRows, kGruImgY = kGruImgHn + kGruRows,
                   kGruImgRstd = kGruImgY + kGruRows, kGruImgCell = kGruImgRstd + kGruTile, kGruImgKeep = kGruImgCell + kGruTile,
                   kGruImgFloats = kGruImgKeep + kGruTile;
constexpr uint32_t kGruAbsent = 0xFFFFFFFFu;
constexpr uint32_t kGruTileFloats = kGruTile * kGruHidden;  // a tile's 32 rows of 64, dense, as the update keeps them in global memory

__device__ __forceinline__ float gru_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float gru_tanh(float x) { return tanhf(x); }

// The GRU and its LayerNorm for the tile: x = the base's output rows (LDS, rows 65 apart, outside the image), img + kGruImgHin =
// h * m, chunk = cnn_fc_layer's 64 x 65 weight buffer.  Leaves the image described above; thread tid owns elements tid, tid + 256,
// ... of the 32 x 64 tile in every element-wise pass, so after the call it may read back the h' it wrote to hin without a barrier
// (there is one anyway: the LayerNorm ends behind it).
__device__ __forceinline__ void gru_step_forward(const float *__restrict__ block, const float *__restrict__ x, float *__restrict__ chunk,
                                                 float *__restrict__ img, uint32_t tid)
{
    const uint32_t wave = tid >> 6, lane = tid & 63u;
    float *hin = img + kGruImgHin, *gate = img + kGruImgGate, *hn = img + kGruImgHn;
    const float *__restrict__ w_ih = block, *__restrict__ w_hh = block + kGruWhhOff;
    const float *__restrict__ b_ih = block + kGruBihOff, *__restrict__ b_hh = block + kGruBhhOff;
#pragma unroll 1
    for (uint32_t g = 0; g < 3u; g++) {
        cnn_fc_layer(x, kGruLd, kGruHidden, w_ih + g * kGruHidden * kGruHidden, b_ih + g * kGruHidden, kGruHidden, false, chunk,
                     gate + g * kGruRows, kGruLd, wave, lane);
        cnn_fc_layer(hin, kGruLd, kGruHidden, w_hh + g * kGruHidden * kGruHidden, b_hh + g * kGruHidden, kGruHidden, false, chunk,
                     gate + (3u + g) * kGruRows, kGruLd, wave, lane);
    }
    for (uint32_t idx = tid; idx < kGruTile * kGruHidden; idx += kGruThreads) {
        const uint32_t at = (idx >> 6) * kGruLd + (idx & 63u);
        const float r = gru_sigmoid(gate[at] + gate[3u * kGruRows + at]);
        const float z = gru_sigmoid(gate[kGruRows + at] + gate[4u * kGruRows + at]);
        const float n = gru_tanh(gate[2u * kGruRows + at] + r * gate[5u * kGruRows + at]);
        const float h = hin[at], next = (1.0f - z) * n + z * h;
        gate[at] = r, gate[kGruRows + at] = z, gate[2u * kGruRows + at] = n;
        hin[at] = next, hn[at] = next;
    }
    __syncthreads();
    const float *__restrict__ norm = block + kGruNormOff;
    mlpbase_layer_norm(hn, img + kGruImgY, kGruLd, kGruHidden, norm, norm + kGruHidden, img + kGruImgRstd, nullptr, wave, lane);
}

// the head of a recurrent net: from gy to outs (row stride 8); head_w (out_dim, 64), then the bias
__device__ __forceinline__ void gru_step_head(const float *__restrict__ head_w, uint32_t out_dim, float *__restrict__ chunk,
                                              const float *__restrict__ img, float *__restrict__ outs, uint32_t tid)
{
    cnn_fc_layer(img + kGruImgY, kGruLd, kGruHidden, head_w, head_w + out_dim * kGruHidden, out_dim, false, chunk, outs, 8u, tid >> 6, tid & 63u);
}

// out[sample][col] = sum over the three gates g of d_g[sample][:] W[g][:][col] (W: three 64 x 64 blocks), a 32-column slab per
// calling wave (`slab` 0 or 1); with `add`: (that + add[sample][col]) * keep[sample]
__device__ __forceinline__ void gru_d_in3(const float *d0, const float *d1, const float *d2, const float *__restrict__ w, float *out,
                                          const float *add, const float *keep, uint32_t slab, uint32_t r, uint32_t half)
{
    const uint32_t col = 32u * slab + r;
    mappo_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 1
    for (uint32_t g = 0; g < 3u; g++) {
        const float *d = g == 0u ? d0 : (g == 1u ? d1 : d2);
        const float *__restrict__ wg = w + g * kGruHidden * kGruHidden;
#pragma unroll 4
        for (uint32_t kk = 0; kk < kGruHidden / 2u; kk++) {
            const uint32_t j = 2u * kk + half;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[r * kGruLd + j], wg[j * kGruHidden + col], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t row = tile_row(e, half);
        out[row * kGruLd + col] = add ? (acc[e] + add[row * kGruLd + col]) * keep[row] : acc[e];
    }
}

// Back through the head, the LayerNorm and the GRU of one step, on the image gru_step_forward and gru_step_head left, with hin put
// back to h_in = h * m by the caller (the forward pass left h' there) and d_out (32 x 8) = dL/d(head output) complete behind a
// barrier.  With dh' = dL/dh' (from the LayerNorm and, where carry_in, from step i + 1 in `carry`):
//     dn = dh' (1 - z), dz = dh' (h_in - n); a_n = dn (1 - n^2), a_z = dz z (1 - z), a_r = a_n gh_n r (1 - r)
//     dgi = (a_r, a_z, a_n), dgh = (a_r, a_z, a_n r); dW_ih += dgi^T x, dW_hh += dgh^T h_in on the matrix instruction with the
//     sample pair as k (mappo_dw_block, three each); db_ih, db_hh column sums in ascending sample order;
//     dx = dgi W_ih, dh_in = dgh W_hh + dh' z; where carry_out, carry = dh_in m (what step i - 1 receives).
// The accumulators live in the workgroup's partial vector: g_block in the parameter block's order, g_head_w, g_head_b (`first`:
// nothing has been accumulated yet).  Leaves dx = dL/dx in gate[3] (img + kGruImgGate + 3 kGruRows); gate[4] is free for the
// caller; everything else in the image is dead.  Ends behind a barrier.
__device__ __forceinline__ void gru_step_backward(const float *__restrict__ block, float *__restrict__ g_block, const float *__restrict__ head_w,
                                                  float *__restrict__ g_head_w, float *__restrict__ g_head_b, uint32_t out_dim, const float *d_out,
                                                  const float *x, float *img, float *carry, bool carry_in, bool carry_out, bool first, uint32_t tid)
{
    const uint32_t lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    float *hin = img + kGruImgHin, *gate = img + kGruImgGate, *hn = img + kGruImgHn, *keep = img + kGruImgKeep;
    float *d_gy = gate + 3u * kGruRows, *d_h = gate + 4u * kGruRows;
    const float *__restrict__ norm_w = block + kGruNormOff;
    float *__restrict__ g_wih = g_block, *__restrict__ g_whh = g_block + kGruWhhOff, *__restrict__ g_bih = g_block + kGruBihOff;
    float *__restrict__ g_bhh = g_block + kGruBhhOff, *__restrict__ g_norm = g_block + kGruNormOff;
    // ---- head: dW_head, db_head and dL/d(gy)
    mappo_head_backward<false>(head_w, g_head_w, g_head_b, out_dim, d_out, img + kGruImgY, d_gy, nullptr, kGruLd, first, tid);
    __syncthreads();
    // ---- the GRU's LayerNorm: dh' = rstd (g - mean(g) - xhat mean(g xhat)) + what step i + 1 carried here
    {
        const float weight = norm_w[lane];
        for (uint32_t row = wave; row < kGruTile; row += 4u) {
            const float xh = hn[row * kGruLd + lane], g = d_gy[row * kGruLd + lane] * weight;
            const float mean_g = wave_sum(g) / (float)kGruHidden, mean_gx = wave_sum(g * xh) / (float)kGruHidden;
            const float dx = img[kGruImgRstd + row] * ((g - mean_g) - xh * mean_gx);
            d_h[row * kGruLd + lane] = carry_in ? dx + carry[row * kGruLd + lane] : dx;
        }
        if (wave == 0u)
            column_sum(g_norm, first, d_gy, hn, kGruLd, kGruLd, lane);
        else if (wave == 1u)
            column_sum(g_norm + kGruHidden, first, d_gy, nullptr, kGruLd, 0u, lane);
    }
    __syncthreads();  // dh' is complete; d_gy and the normalised rows are dead
    // ---- the gates, element-wise: gate[0], [1], [2], [5] become a_r, a_z, a_n, a_n r; hn becomes dh' z
    for (uint32_t idx = tid; idx < kGruTileFloats; idx += kGruThreads) {
        const uint32_t at = (idx >> 6) * kGruLd + (idx & 63u);
        const float dh = d_h[at], rg = gate[at], zg = gate[kGruRows + at], ng = gate[2u * kGruRows + at], ghn = gate[5u * kGruRows + at];
        const float a_n = (dh * (1.0f - zg)) * (1.0f - ng * ng);
        const float a_z = (dh * (hin[at] - ng)) * (zg * (1.0f - zg));
        const float a_r = (a_n * ghn) * (rg * (1.0f - rg));
        gate[at] = a_r, gate[kGruRows + at] = a_z, gate[2u * kGruRows + at] = a_n, gate[5u * kGruRows + at] = a_n * rg;
        hn[at] = dh * zg;
    }
    __syncthreads();  // the gate gradients are complete; dh' is dead
    // ---- dW_ih = dgi^T x, dW_hh = dgh^T h_in, a 32 x 32 block per wave each; the bias sums
#pragma unroll 1
    for (uint32_t g = 0; g < 3u; g++) {
        const float *dgi = gate + g * kGruRows, *dgh = gate + (g == 2u ? 5u : g) * kGruRows;
        mappo_dw_block(g_wih + g * kGruHidden * kGruHidden, dgi, x, kGruLd, first, wave, r, half);
        mappo_dw_block(g_whh + g * kGruHidden * kGruHidden, dgh, hin, kGruLd, first, wave, r, half);
        if (wave == g)
            column_sum(g_bih + g * kGruHidden, first, dgi, nullptr, kGruLd, 0u, lane);
        else if (wave == ((g + 1u) & 3u))
            column_sum(g_bhh + g * kGruHidden, first, dgh, nullptr, kGruLd, 0u, lane);
    }
    // ---- dx on waves 0 and 1; on waves 2 and 3 what step i - 1 receives: (dgh W_hh + dh' z) m_i
    if (wave < 2u)
        gru_d_in3(gate, gate + kGruRows, gate + 2u * kGruRows, block, d_gy, nullptr, nullptr, wave, r, half);
    else if (carry_out)
        gru_d_in3(gate, gate + kGruRows, gate + 5u * kGruRows, block + kGruWhhOff, carry, hn, keep, wave - 2u, r, half);
    __syncthreads();  // dx and the carry are complete; the gate gradients are dead
}

}  // namespace mrl
