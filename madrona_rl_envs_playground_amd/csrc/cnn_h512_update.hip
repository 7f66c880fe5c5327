// mrl_mappo_h512_update: MAPPO's update for the CNN actor-critic at hidden_size 512 without torch in the loop (include/mrl_envs.h;
// DESIGN.md section 31; the slabs, the workspace and the order of every sum are in cnn_h512_update.hpp).
//
// A row is cut into slabs of at most kH512Slab samples.  Per slab, for both nets at once (the net is a grid dimension):
//   mrl_h512_forward  the act's computation (cnn_h512_forward.hpp: the same chains, hence the same bits) on the samples the
//                     index list names, a workgroup per tile of 32; it stores the post-ReLU conv image, h1, h2 and the head's
//                     outputs.  A row past the slab's end is a zero observation.
//   mrl_h512_loss     a lane per sample (mappo_loss.hpp): dL/d(head output), the gated d_h2 and the stats' double sums per tile.
//   mrl_h512_dw       a weight gradient C = A^T B with k = the slab's samples: dW_head = d_out^T h2, dW_fc2 = d_h2^T h1,
//                     dW_fc1 = d_h1^T act, and each bias gradient as the same product against ones.  A workgroup of four waves
//                     owns a 128 x 128 tile of C and share q of the samples; a wave keeps its 64 x 64 sub-tile in 64 accumulator
//                     registers across the whole share.  BOTH operands are staged through LDS in chunks of 32 samples -- one
//                     global load serves four waves -- with the next chunk's loads issued before the current products; an LDS row
//                     is 160 floats, so the lanes 32..63 (sample 2 kk + 1) read the banks the lanes 0..31 leave free.
//   mrl_h512_dx       an activation gradient D = gate (A W) with k = the layer's 512 outputs: d_h1 = (h1 > 0) (d_h2 W_fc2) and
//                     d_act = (act > 0) (d_h1 W_fc1), the latter in place over the conv image once dW_fc1 has read it.  A
//                     workgroup owns 64 rows x 128 columns; A (rows of 33 floats) and W (rows of 160) are staged in chunks of 32 k.
//   mrl_h512_dconv    dW_conv and db_conv: workgroup (channel block of 32, share q) loads a tile's int8 rows (cnn_load_tile) and
//                     its 32 x 32 npos slice of d_act into LDS and keeps the 32 x 9 F accumulator, split over the waves by
//                     32-column slab, in registers across the share.
//   mrl_h512_fold     the shares' sums in ascending q onto the running gradient, the tiles' stats onto the running stats.
// Per row the optimiser tail (adam_step.hpp) then runs on the one running vector per net.  Every product is
// v_mfma_f32_32x32x2_f32.  No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits.
#include "cnn_h512_update.hpp"
#include "cnn_h512_forward.hpp"
#include "mappo_grad.hpp"

namespace mrl {

namespace {

constexpr uint32_t kGemmLd = 160;  // an LDS row of 128 columns: 160 = 32 mod 64, the two halves of a wave on different banks
constexpr uint32_t kDxLda = 33;    // an LDS row of 32 k of the dx kernel's A operand: odd, lane r reads bank 33 r + k
constexpr uint32_t kChunk = 32;    // samples (dw) or k (dx) per staged chunk
static_assert(kCnnH512Hidden % 128u == 0 && kCnnH512Channels % 128u == 0, "every product's column count is a multiple of a 128-column tile");
static_assert(kH512Slab % 64u == 0, "a slab is whole tiles of the dx kernel's 64 rows");

extern __shared__ __attribute__((aligned(16))) unsigned char h512_upd_lds_image[];

// where a net's tensors start in its parameter (and gradient) vector
struct H512Offsets {
    uint64_t conv_b, fc1_w, fc1_b, fc2_w, fc2_b, head_w, head_b[2], net[2];
};
H512Offsets h512_offsets(uint64_t W, uint64_t H, uint64_t F)
{
    H512Offsets o;
    const uint64_t K2 = kCnnH512Channels * (W - 2) * (H - 2);
    o.conv_b = kCnnH512Channels * F * 9;
    o.fc1_w = o.conv_b + kCnnH512Channels;
    o.fc1_b = o.fc1_w + kCnnH512Hidden * K2;
    o.fc2_w = o.fc1_b + kCnnH512Hidden;
    o.fc2_b = o.fc2_w + (uint64_t)kCnnH512Hidden * kCnnH512Hidden;
    o.head_w = o.fc2_b + kCnnH512Hidden;
    o.head_b[0] = o.head_w + kCnnActions * kCnnH512Hidden;
    o.head_b[1] = o.head_w + kCnnH512Hidden;
    o.net[0] = 0;
    o.net[1] = cnn_h512_net_params(W, H, F, kCnnActions);
    return o;
}

// ---------------------------------------------------------------- the forward pass, storing activations

struct H512ForwardArgs {
    CnnActArgs fwd;          // W, H, F, the act's LDS image, params
    const int8_t *obs;       // the batch's rows (S, H, W, F)
    const int32_t *indices;  // the slab's sample numbers
    float *act, *h1, *h2, *out;  // net 0's; net 1's lie `rows` rows behind
    uint32_t count, batch_size, rows;  // the slab's samples, S, the workspace's rows per net
};

// mrl_cnn_act_h512's body (cnn_h512.hip) on gathered samples, every layer's output stored
__global__ void __launch_bounds__(kCnnThreads) mrl_h512_forward(H512ForwardArgs g)
{
    const CnnActArgs &a = g.fwd;
    const uint32_t net = blockIdx.y;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const bool odd = half != 0u;
    const CnnLds &l = a.lds;
    const uint32_t S = a.W * a.H * a.F, k1 = l.k1, kb = kCnnChannels * l.npos, K2 = kCnnH512Channels * l.npos;
    const uint32_t out_dim = net ? 1u : kCnnActions;
    const float *__restrict__ conv_w = a.params + (net ? cnn_h512_net_params(a.W, a.H, a.F, kCnnActions) : 0);
    const float *__restrict__ conv_b = conv_w + (size_t)kCnnH512Channels * k1;
    const float *__restrict__ fc1_w = conv_b + kCnnH512Channels, *__restrict__ fc1_b = fc1_w + (size_t)kCnnH512Hidden * K2;
    const float *__restrict__ fc2_w = fc1_b + kCnnH512Hidden, *__restrict__ fc2_b = fc2_w + kCnnH512Hidden * kCnnH512Hidden;
    const float *__restrict__ head_w = fc2_b + kCnnH512Hidden, *__restrict__ head_b = head_w + out_dim * kCnnH512Hidden;

    unsigned char *lds = h512_upd_lds_image;
    const uint32_t tile0 = blockIdx.x * kCnnTile;
    const size_t row0 = (size_t)net * g.rows + tile0;  // the tile's first row of the net's stored arrays
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        if (tile0 + rr >= g.count) return nullptr;
        uint32_t s = (uint32_t)g.indices[tile0 + rr];
        s = s < g.batch_size ? s : g.batch_size - 1u;  // outside the contract, but memory-safe
        return reinterpret_cast<const uint8_t *>(g.obs) + (size_t)s * S;
    };
    cnn_load_tile(a, lds, row_address, nullptr, conv_w, true);
    __syncthreads();
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(row_address(r)) & 3u);

    f32x16 acc[4];
    const float *w_row[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        w_row[j] = fc1_w + (size_t)((wave * 4u + j) * 32u + r) * K2;
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.0f;
    }
    const float *act_lds = reinterpret_cast<const float *>(lds + l.act_at);
    const float *a_row = act_lds + r * l.act_ld + half;
    float *conv_lds = reinterpret_cast<float *>(lds + l.conv_w_at);
    for (uint32_t b = 0; b < kCnnH512Blocks; b++) {
        cnn_conv_tile(a, lds, shift, conv_b + b * kCnnChannels, wave, r, half);
        __syncthreads();
        if (b + 1u < kCnnH512Blocks) {
            const float *__restrict__ next = conv_w + (size_t)(b + 1u) * kCnnChannels * k1;
            for (uint32_t e = tid; e < kCnnChannels * k1; e += kCnnThreads) {
                const uint32_t c = e / k1, k = e - c * k1;
                conv_lds[c * l.conv_ld + k] = next[e];
            }
        }
        // the block's activations: columns [b kb, (b + 1) kb) of the stored image
        for (uint32_t e = tid; e < kCnnTile * kb; e += kCnnThreads) {
            const uint32_t row = e / kb, j = e - row * kb;
            g.act[(row0 + row) * K2 + b * kb + j] = act_lds[row * l.act_ld + j];
        }
        f32x16 part[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) part[j][e] = 0.0f;
        h512_products<4>(a_row, kb, w_row, odd, part);
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int e = 0; e < 16; e++) acc[j][e] += part[j][e];
            w_row[j] += kb;
        }
        __syncthreads();
    }

    float *h = reinterpret_cast<float *>(lds), *outs = reinterpret_cast<float *>(lds + kCnnTile * kCnnH512HLd * 4u);
    h512_store(acc, fc1_b, h, wave, r, half);
    __syncthreads();
    for (uint32_t e = tid; e < kCnnTile * kCnnH512Hidden; e += kCnnThreads)
        g.h1[(row0 + (e >> 9)) * kCnnH512Hidden + (e & 511u)] = h[(e >> 9) * kCnnH512HLd + (e & 511u)];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        w_row[j] = fc2_w + (size_t)((wave * 4u + j) * 32u + r) * kCnnH512Hidden;
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.0f;
    }
    const float *h_row = h + r * kCnnH512HLd + half;
    h512_products<4>(h_row, kCnnH512Hidden, w_row, odd, acc);
    __syncthreads();
    h512_store(acc, fc2_b, h, wave, r, half);
    __syncthreads();
    for (uint32_t e = tid; e < kCnnTile * kCnnH512Hidden; e += kCnnThreads)
        g.h2[(row0 + (e >> 9)) * kCnnH512Hidden + (e & 511u)] = h[(e >> 9) * kCnnH512HLd + (e & 511u)];
    if (wave == 0) {
        f32x16 out[1];
        const float *head_row[1] = {head_w + (size_t)(r < out_dim ? r : 0u) * kCnnH512Hidden};
#pragma unroll
        for (int e = 0; e < 16; e++) out[0][e] = 0.0f;
        h512_products<1>(h_row, kCnnH512Hidden, head_row, odd, out);
        if (r < 8u) {
            const float bias = r < out_dim ? head_b[r] : 0.0f;
#pragma unroll
            for (int e = 0; e < 16; e++) outs[((e & 3) + 8 * (e >> 2) + 4 * half) * 8u + r] = r < out_dim ? out[0][e] + bias : 0.0f;
        }
    }
    __syncthreads();
    if (tid < kCnnTile * 8u) g.out[row0 * 8u + tid] = outs[tid];
}

// ---------------------------------------------------------------- the loss head

struct H512LossArgs {
    MappoGradCommon common;  // indices: the slab's; groups: the slab's tiles; partial_stats: (2, tiles, 8)
    const float *params, *out, *h2;
    float *d_out, *d_h2;
    uint64_t head_w[2];  // where each net's head weights start in params
    uint32_t count, rows;
};

__global__ void __launch_bounds__(kMappoThreads) mrl_h512_loss(H512LossArgs g)
{
    __shared__ uint32_t sample[kMappoTile];
    __shared__ float d_out[kMappoTile * 8u];
    __shared__ double sums[4 * kMappoTile];
    const MappoGradCommon &c = g.common;
    const uint32_t net = blockIdx.y, tid = threadIdx.x, out_dim = net ? 1u : kCnnActions;
    const uint64_t base = (uint64_t)blockIdx.x * kMappoTile;
    const size_t row0 = (size_t)net * g.rows + base;
    mappo_tile_samples(c, sample, base, g.count, tid);
    __syncthreads();
    double stat[4] = {0.0, 0.0, 0.0, 0.0};
    mappo_loss_head<(int)kCnnActions>(c, net, sample, g.out + row0 * 8u, d_out, (float)c.minibatch_size, stat, tid);
    __syncthreads();
    g.d_out[row0 * 8u + tid] = d_out[tid];
    // d_h2 behind fc2's ReLU: a plain ordered loop over the head's outputs
    const float *__restrict__ head_w = g.params + g.head_w[net];
    for (uint32_t idx = tid; idx < kMappoTile * kCnnH512Hidden; idx += kMappoThreads) {
        const uint32_t s = idx >> 9, j = idx & 511u;
        float sum = 0.0f;
        for (uint32_t o = 0; o < out_dim; o++) sum = fmaf(head_w[o * kCnnH512Hidden + j], d_out[s * 8u + o], sum);
        const size_t at = (row0 + s) * kCnnH512Hidden + j;
        g.d_h2[at] = g.h2[at] > 0.0f ? sum : 0.0f;
    }
    mappo_stats_tail(c, net, sums, stat, tid);
}

// ---------------------------------------------------------------- the weight gradients of the linear layers

// 32 samples x 128 columns from `src` (rows ld floats apart, `cols` valid columns from col0 on) into registers
__device__ __forceinline__ void dw_fetch(const float *__restrict__ src, uint32_t ld, uint32_t col0, uint32_t cols, uint32_t tid, f32x4u (&p)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t idx = tid + 256u * i, srow = idx >> 5, col = col0 + 4u * (idx & 31u);
        if (col < cols)
            p[i] = *reinterpret_cast<const f32x4u *>(src + (size_t)srow * ld + col);
        else
            p[i] = f32x4u{0.0f, 0.0f, 0.0f, 0.0f};
    }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void dw_stage(float *__restrict__ dst, uint32_t tid, const f32x4u (&p)[4])
{
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t idx = tid + 256u * i;
        *reinterpret_cast<f32x4 *>(dst + (idx >> 5) * kGemmLd + 4u * (idx & 31u)) = f32x4{p[i][0], p[i][1], p[i][2], p[i][3]};
    }
}

__global__ void __launch_bounds__(kCnnThreads) mrl_h512_dw(H512DwArgs g)
{
    __shared__ __attribute__((aligned(16))) float a_lds[kChunk * kGemmLd];
    __shared__ __attribute__((aligned(16))) float b_lds[kChunk * kGemmLd];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t wm = wave >> 1, wn = wave & 1u;
    const uint32_t q = blockIdx.z % kH512Shares, net = blockIdx.z / kH512Shares;
    const uint32_t m0 = blockIdx.y * 128u, n0 = blockIdx.x * 128u;
    const bool bias = blockIdx.x == 0 && wn == 0;  // these waves also sum A's columns: the product against ones
    const uint32_t begin = q * g.share, end = begin + g.share < g.nrows ? begin + g.share : g.nrows;
    const float *__restrict__ A = g.a + net * g.a_net, *__restrict__ B = g.b + net * g.b_net;

    f32x16 acc[2][2], ones[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int e = 0; e < 16; e++) acc[i][0][e] = acc[i][1][e] = ones[i][e] = 0.0f;
    }
    f32x4u pa[4], pb[4];
    if (begin < end) {
        dw_fetch(A + (size_t)begin * g.lda, g.lda, m0, g.a_cols, tid, pa);
        dw_fetch(B + (size_t)begin * g.ldb, g.ldb, n0, g.n, tid, pb);
    }
    for (uint32_t s0 = begin; s0 < end; s0 += kChunk) {
        dw_stage(a_lds, tid, pa);
        dw_stage(b_lds, tid, pb);
        __syncthreads();
        if (s0 + kChunk < end) {
            dw_fetch(A + (size_t)(s0 + kChunk) * g.lda, g.lda, m0, g.a_cols, tid, pa);
            dw_fetch(B + (size_t)(s0 + kChunk) * g.ldb, g.ldb, n0, g.n, tid, pb);
        }
        const float *__restrict__ pa_lds = a_lds + half * kGemmLd + 64u * wm + r, *__restrict__ pb_lds = b_lds + half * kGemmLd + 64u * wn + r;
#pragma unroll 4
        for (uint32_t kk = 0; kk < kChunk / 2u; kk++) {
            const float a0 = pa_lds[2u * kk * kGemmLd], a1 = pa_lds[2u * kk * kGemmLd + 32u];
            const float b0 = pb_lds[2u * kk * kGemmLd], b1 = pb_lds[2u * kk * kGemmLd + 32u];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            if (bias) {
                ones[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, 1.0f, ones[0], 0, 0, 0);
                ones[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, 1.0f, ones[1], 0, 0, 0);
            }
        }
        __syncthreads();  // the next chunk overwrites what the products read
    }

    float *__restrict__ out = g.partial + ((size_t)net * kH512Shares + q) * g.stride;
    const uint32_t rows = g.m[net];
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t row = m0 + 64u * wm + 32u * i + tile_row(e, half);
            if (row < rows) {
                float *__restrict__ c_row = out + g.w_at + (size_t)row * g.n + n0 + 64u * wn + r;
                c_row[0] = acc[i][0][e];
                c_row[32] = acc[i][1][e];
                if (bias && r == 0u) out[g.bias_at[net] + row] = ones[i][e];
            }
        }
    }
}

// ---------------------------------------------------------------- the activation gradients of the linear layers

struct H512DxArgs {
    const float *d;     // net 0's A (nrows x 512): dL/d(the layer's pre-activation)
    const float *gate;  // net 0's gate (nrows x cols): the layer's post-ReLU input
    float *out;         // net 0's D (nrows x cols); may be `gate`
    uint64_t w[2];      // where each net's weight (512 x cols, row-major) starts in params
    const float *params;
    uint64_t d_net, out_net;
    uint32_t nrows, cols;  // cols a multiple of 128
};

__global__ void __launch_bounds__(kCnnThreads) mrl_h512_dx(H512DxArgs g)
{
    __shared__ float a_lds[64u * kDxLda];
    __shared__ __attribute__((aligned(16))) float b_lds[kChunk * kGemmLd];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t net = blockIdx.z, col0 = blockIdx.x * 128u, row0 = blockIdx.y * 64u;
    const float *__restrict__ A = g.d + net * g.d_net + (size_t)row0 * kCnnH512Hidden;
    const float *__restrict__ W = g.params + g.w[net];

    f32x16 acc[2];
#pragma unroll
    for (int e = 0; e < 16; e++) acc[0][e] = acc[1][e] = 0.0f;
    f32x4u pa[2], pb[4];
    // 64 rows x 32 k of A: thread t takes rows t / 8 and 32 + t / 8, four k each; 32 k x 128 columns of W as dw_fetch
    const uint32_t a_row = tid >> 3, a_k = 4u * (tid & 7u);
    const auto fetch = [&](uint32_t k0) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const uint32_t row = a_row + 32u * i;
            if (row0 + row < g.nrows)
                pa[i] = *reinterpret_cast<const f32x4u *>(A + (size_t)row * kCnnH512Hidden + k0 + a_k);
            else
                pa[i] = f32x4u{0.0f, 0.0f, 0.0f, 0.0f};
        }
        dw_fetch(W + (size_t)k0 * g.cols, g.cols, col0, g.cols, tid, pb);
    };
    fetch(0u);
    for (uint32_t k0 = 0; k0 < kCnnH512Hidden; k0 += kChunk) {
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) a_lds[(a_row + 32u * i) * kDxLda + a_k + j] = pa[i][j];
        dw_stage(b_lds, tid, pb);
        __syncthreads();
        if (k0 + kChunk < kCnnH512Hidden) fetch(k0 + kChunk);
        const float *__restrict__ pa_lds = a_lds + r * kDxLda + half, *__restrict__ pb_lds = b_lds + half * kGemmLd + 32u * wave + r;
#pragma unroll 4
        for (uint32_t kk = 0; kk < kChunk / 2u; kk++) {
            const float b = pb_lds[2u * kk * kGemmLd];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa_lds[2u * kk], b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(pa_lds[32u * kDxLda + 2u * kk], b, acc[1], 0, 0, 0);
        }
        __syncthreads();
    }
    const size_t at = net * g.out_net + col0 + 32u * wave + r;
#pragma unroll
    for (int i = 0; i < 2; i++) {
#pragma unroll
        for (int e = 0; e < 16; e++) {
            const uint32_t row = row0 + 32u * i + tile_row(e, half);
            if (row < g.nrows) {
                const size_t p = at + (size_t)row * g.cols;
                g.out[p] = g.gate[p] > 0.0f ? acc[i][e] : 0.0f;
            }
        }
    }
}

// ---------------------------------------------------------------- the convolution's weight gradient

struct H512ConvArgs {
    CnnActArgs fwd;  // W, H, F and cnn_lds' image
    const int8_t *obs;
    const int32_t *indices;  // the slab's sample numbers
    const float *d_act;      // net 0's (nrows x 256 npos)
    float *partial;
    uint64_t act_net, stride;
    uint32_t count, batch_size, nrows, share, tail_at;
};

__global__ void __launch_bounds__(kCnnThreads) mrl_h512_dconv(H512ConvArgs g)
{
    const CnnActArgs &f = g.fwd;
    const CnnLds &l = f.lds;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t b = blockIdx.x, q = blockIdx.y, net = blockIdx.z;
    const uint32_t k1 = l.k1, npos = l.npos, kb = kCnnChannels * npos, K2 = kCnnH512Channels * npos, act_ld = l.act_ld;
    const uint32_t slabs = (k1 + 31u) / 32u, hh = f.H - 2u;
    unsigned char *lds = h512_upd_lds_image;
    const uint16_t *koff = reinterpret_cast<const uint16_t *>(lds + l.koff_at);
    float *act = reinterpret_cast<float *>(lds + l.act_at);
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + g.tail_at), *shifts = sample + kCnnTile;
    const float *__restrict__ d_act = g.d_act + net * g.act_net + (size_t)b * kb;
    const uint32_t begin = q * g.share, end = begin + g.share < g.nrows ? begin + g.share : g.nrows;
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        const uint32_t s = sample[rr];
        return s == kMappoAbsent ? nullptr : reinterpret_cast<const uint8_t *>(g.obs) + (size_t)s * (f.W * f.H * f.F);
    };

    f32x16 acc[kH512ConvSlabs];
#pragma unroll
    for (uint32_t i = 0; i < kH512ConvSlabs; i++)
#pragma unroll
        for (int e = 0; e < 16; e++) acc[i][e] = 0.0f;
    float bias_sum = 0.0f;  // lanes 0..31 of the wave with the fewest slabs: db_conv of channel 32 b + lane
    for (uint32_t base = begin; base < end; base += kCnnTile) {
        if (tid < kCnnTile) {
            uint32_t s = kMappoAbsent;
            if (base + tid < g.count) {
                s = (uint32_t)g.indices[base + tid];
                s = s < g.batch_size ? s : g.batch_size - 1u;
            }
            sample[tid] = s;
        }
        __syncthreads();
        cnn_load_tile(f, lds, row_address, shifts, nullptr, false);
        for (uint32_t e = tid; e < kCnnTile * kb; e += kCnnThreads) {
            const uint32_t row = e / kb, j = e - row * kb;
            act[row * act_ld + j] = d_act[(size_t)(base + row) * K2 + j];
        }
        __syncthreads();
        uint32_t off[kH512ConvSlabs];
        bool ok[kH512ConvSlabs];
#pragma unroll
        for (uint32_t i = 0; i < kH512ConvSlabs; i++) {
            const uint32_t k = 32u * (wave + 4u * i) + r;
            ok[i] = k < k1;
            off[i] = ok[i] ? koff[k] : 0u;
        }
#pragma unroll 1
        for (uint32_t pos = 0; pos < npos; pos++) {
            const uint32_t ow = pos / hh, oh = pos - ow * hh, at = (oh * f.W + ow) * f.F;
#pragma unroll 2
            for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                const uint32_t s = 2u * kk + half;
                const float a = act[s * act_ld + r * npos + pos];
                const int8_t *__restrict__ row = reinterpret_cast<const int8_t *>(lds) + s * l.obs_ld + shifts[s] + at;
#pragma unroll
                for (uint32_t i = 0; i < kH512ConvSlabs; i++)
                    if (wave + 4u * i < slabs) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ok[i] ? (float)row[off[i]] : 0.0f, acc[i], 0, 0, 0);
            }
        }
        if (slabs % 4u == wave && lane < kCnnChannels)
            for (uint32_t s = 0; s < kCnnTile; s++)
                for (uint32_t pos = 0; pos < npos; pos++) bias_sum += act[s * act_ld + lane * npos + pos];
        __syncthreads();  // the next tile overwrites what the loops above read
    }
    float *__restrict__ out = g.partial + ((size_t)net * kH512Shares + q) * g.stride;
#pragma unroll
    for (uint32_t i = 0; i < kH512ConvSlabs; i++) {
        const uint32_t k = 32u * (wave + 4u * i) + r;
        if (wave + 4u * i < slabs) acc_store(out + (size_t)b * kCnnChannels * k1, k1, kCnnChannels, k, k < k1, half, acc[i]);
    }
    if (slabs % 4u == wave && lane < kCnnChannels) out[(size_t)kCnnH512Channels * k1 + b * kCnnChannels + lane] = bias_sum;
}

// ---------------------------------------------------------------- the shares' sums onto the running gradient

struct H512FoldArgs {
    const float *partial;  // (2, kH512Shares, stride)
    float *run;            // (2, stride)
    const double *slab_stats;  // (2, tiles, 8)
    double *run_stats;         // (2, 8)
    uint64_t stride;
    uint32_t num_params[2], tiles, first;
};

__global__ void __launch_bounds__(kAdamThreads) mrl_h512_fold(H512FoldArgs g)
{
    const uint32_t net = blockIdx.y, p = blockIdx.x * kAdamThreads + threadIdx.x;
    if (p < g.num_params[net]) {
        float sum = 0.0f;
        for (uint32_t q = 0; q < kH512Shares; q++) sum += g.partial[((size_t)net * kH512Shares + q) * g.stride + p];
        float *run = g.run + (size_t)net * g.stride + p;
        *run = g.first ? sum : *run + sum;
    }
    if (blockIdx.x == 0 && threadIdx.x < kMappoStats) {
        double sum = 0.0;
        for (uint32_t t = 0; t < g.tiles; t++) sum += g.slab_stats[((size_t)net * g.tiles + t) * kMappoStats + threadIdx.x];
        double *run = g.run_stats + net * kMappoStats + threadIdx.x;
        *run = g.first ? sum : *run + sum;
    }
}

}  // namespace

void launch_h512_dw(const H512DwArgs &args, hipStream_t stream)
{
    const uint32_t rows = args.m[0] > args.m[1] ? args.m[0] : args.m[1];
    hipLaunchKernelGGL(mrl_h512_dw, dim3(args.n / 128u, (rows + 127u) / 128u, 2u * kH512Shares), dim3(kCnnThreads), 0, stream, args);
    MRL_HIP(hipGetLastError());
}

void launch_mappo_h512_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_batch &batch,
                              const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                              float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    const uint32_t W = policy.width, H = policy.height, F = policy.channels;
    const H512Workspace ws = h512_workspace(W, H, F, minibatch_size, num_minibatches);
    const H512Offsets at = h512_offsets(W, H, F);
    const uint32_t actor = (uint32_t)cnn_h512_net_params(W, H, F, kCnnActions), critic = (uint32_t)cnn_h512_net_params(W, H, F, 1);
    const uint32_t rows = (uint32_t)ws.rows, K2 = (uint32_t)ws.K2;
    const CnnLds lds = cnn_lds(W, H, F);
    const uint32_t forward_lds = cnn_h512_lds(W, H, F).total, conv_lds = lds.total + kH512ConvTail;
    allow_large_dynamic_lds<&mrl_h512_forward>(forward_lds);
    allow_large_dynamic_lds<&mrl_h512_dconv>(conv_lds);
    const bool norm = cfg.flags & MRL_MAPPO_VALUENORM;
    if (norm)
        launch_mappo_value_norm(batch.returns, indices, num_minibatches, minibatch_size, batch.size, cfg, value_norm_state,
                                workspace + ws.row_sums, workspace + ws.row_norm, stream);
    float *act = workspace + ws.act, *h1 = workspace + ws.h1, *h2 = workspace + ws.h2, *d_h1 = workspace + ws.d_h1, *d_h2 = workspace + ws.d_h2;
    float *out = workspace + ws.out, *d_out = workspace + ws.d_out, *partial = workspace + ws.partial, *run = workspace + ws.run;
    double *slab_stats = reinterpret_cast<double *>(workspace + ws.slab_stats), *run_stats = reinterpret_cast<double *>(workspace + ws.run_stats);

    H512ForwardArgs fw{};
    fw.fwd.params = opt.params_dev;
    fw.fwd.W = W, fw.fwd.H = H, fw.fwd.F = F;
    fw.fwd.lds = lds;
    fw.obs = static_cast<const int8_t *>(batch.obs);
    fw.act = act, fw.h1 = h1, fw.h2 = h2, fw.out = out;
    fw.batch_size = batch.size, fw.rows = rows;

    H512LossArgs ls{};
    MappoGradCommon &c = ls.common;
    c.actions = batch.actions, c.logprobs = batch.logprobs, c.value_preds = batch.value_preds;
    c.returns = batch.returns, c.advantages = batch.advantages;
    c.partial_stats = slab_stats;
    c.minibatch_size = minibatch_size, c.batch_size = batch.size;
    c.loss = MappoLoss{cfg.clip_param, cfg.entropy_coef, cfg.value_loss_coef, cfg.huber_delta, cfg.flags};
    ls.params = opt.params_dev, ls.out = out, ls.h2 = h2, ls.d_out = d_out, ls.d_h2 = d_h2;
    ls.head_w[0] = at.net[0] + at.head_w, ls.head_w[1] = at.net[1] + at.head_w;
    ls.rows = rows;

    // the three weight-gradient products and the two activation-gradient products; the operands of a slab are set below
    H512DwArgs head{}, fc2{}, fc1{};
    for (H512DwArgs *dw : {&head, &fc2, &fc1}) dw->partial = partial, dw->stride = ws.stride;
    head.a = d_out, head.b = h2, head.a_net = (uint64_t)rows * 8, head.b_net = (uint64_t)rows * kCnnH512Hidden;
    head.lda = 8, head.ldb = kCnnH512Hidden, head.a_cols = 8, head.m[0] = kCnnActions, head.m[1] = 1, head.n = kCnnH512Hidden;
    head.w_at = at.head_w, head.bias_at[0] = at.head_b[0], head.bias_at[1] = at.head_b[1];
    fc2.a = d_h2, fc2.b = h1, fc2.a_net = fc2.b_net = (uint64_t)rows * kCnnH512Hidden;
    fc2.lda = fc2.ldb = fc2.a_cols = fc2.m[0] = fc2.m[1] = fc2.n = kCnnH512Hidden;
    fc2.w_at = at.fc2_w, fc2.bias_at[0] = fc2.bias_at[1] = at.fc2_b;
    fc1.a = d_h1, fc1.b = act, fc1.a_net = (uint64_t)rows * kCnnH512Hidden, fc1.b_net = (uint64_t)rows * K2;
    fc1.lda = fc1.a_cols = fc1.m[0] = fc1.m[1] = kCnnH512Hidden, fc1.ldb = fc1.n = K2;
    fc1.w_at = at.fc1_w, fc1.bias_at[0] = fc1.bias_at[1] = at.fc1_b;
    H512DxArgs to_h1{}, to_act{};
    to_h1.params = to_act.params = opt.params_dev;
    to_h1.d = d_h2, to_h1.gate = h1, to_h1.out = d_h1, to_h1.cols = kCnnH512Hidden;
    to_h1.d_net = to_h1.out_net = (uint64_t)rows * kCnnH512Hidden;
    to_h1.w[0] = at.net[0] + at.fc2_w, to_h1.w[1] = at.net[1] + at.fc2_w;
    to_act.d = d_h1, to_act.gate = act, to_act.out = act, to_act.cols = K2;
    to_act.d_net = (uint64_t)rows * kCnnH512Hidden, to_act.out_net = (uint64_t)rows * K2;
    to_act.w[0] = at.net[0] + at.fc1_w, to_act.w[1] = at.net[1] + at.fc1_w;

    H512ConvArgs cv{};
    cv.fwd = fw.fwd;
    cv.obs = fw.obs;
    cv.d_act = act, cv.partial = partial;
    cv.act_net = (uint64_t)rows * K2, cv.stride = ws.stride;
    cv.batch_size = batch.size, cv.tail_at = lds.total;

    H512FoldArgs fold{partial, run, slab_stats, run_stats, ws.stride, {actor, critic}, 0, 0};

    AdamStepArgs ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.opti_eps, cfg.flags & MRL_MAPPO_MAX_GRAD_NORM, cfg.max_grad_norm);
    ad.partial_grads = run;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = ws.stride;
    ad.segments = 2;
    ad.groups = 1;
    ad.blocks = (uint32_t)ws.blocks;
    ad.num_params[0] = actor, ad.num_params[1] = critic;
    ad.at[0] = 0, ad.at[1] = actor;
    MappoStatsRow row{run_stats, nullptr, 1, minibatch_size};

    const dim3 threads(kCnnThreads);
    for (uint32_t k = 0; k < num_minibatches; k++) {
        const int32_t *row_indices = indices + (size_t)k * minibatch_size;
        c.row_norm = norm ? workspace + ws.row_norm + 2 * (size_t)k : nullptr;
        for (uint64_t s0 = 0; s0 < minibatch_size; s0 += kH512Slab) {
            const uint32_t count = (uint32_t)(minibatch_size - s0 < kH512Slab ? minibatch_size - s0 : kH512Slab);
            const uint32_t tiles = (count + kCnnTile - 1) / kCnnTile, nrows = tiles * kCnnTile;
            const uint32_t share = (tiles + kH512Shares - 1) / kH512Shares * kCnnTile;
            fw.indices = c.indices = cv.indices = row_indices + s0;
            fw.count = ls.count = cv.count = count;
            c.groups = fold.tiles = tiles;
            hipLaunchKernelGGL(mrl_h512_forward, dim3(tiles, 2), threads, forward_lds, stream, fw);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_loss, dim3(tiles, 2), threads, 0, stream, ls);
            MRL_HIP(hipGetLastError());
            for (H512DwArgs *dw : {&head, &fc2, &fc1}) dw->nrows = nrows, dw->share = share;
            to_h1.nrows = to_act.nrows = cv.nrows = nrows;
            cv.share = share;
            const dim3 shares(1, 1, 2 * kH512Shares);
            hipLaunchKernelGGL(mrl_h512_dw, dim3(kCnnH512Hidden / 128, 1, shares.z), threads, 0, stream, head);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_dx, dim3(kCnnH512Hidden / 128, (nrows + 63) / 64, 2), threads, 0, stream, to_h1);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_dw, dim3(kCnnH512Hidden / 128, kCnnH512Hidden / 128, shares.z), threads, 0, stream, fc2);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_dw, dim3(K2 / 128, kCnnH512Hidden / 128, shares.z), threads, 0, stream, fc1);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_dx, dim3(K2 / 128, (nrows + 63) / 64, 2), threads, 0, stream, to_act);
            MRL_HIP(hipGetLastError());
            hipLaunchKernelGGL(mrl_h512_dconv, dim3(kCnnH512Blocks, kH512Shares, 2), threads, conv_lds, stream, cv);
            MRL_HIP(hipGetLastError());
            fold.first = s0 == 0 ? 1u : 0u;
            hipLaunchKernelGGL(mrl_h512_fold, dim3((uint32_t)ws.blocks, 2), dim3(kAdamThreads), 0, stream, fold);
            MRL_HIP(hipGetLastError());
        }
        ad.grads_row = grads ? grads + (size_t)k * ((size_t)actor + critic) : nullptr;
        adam_set_step(ad, (double)opt.step + 1.0 + (double)k, {cfg.lr, cfg.critic_lr});
        row.row = stats ? stats + (size_t)k * kMappoStats : nullptr;
        launch_adam_step(ad, row, stream);
    }
}

}  // namespace mrl
