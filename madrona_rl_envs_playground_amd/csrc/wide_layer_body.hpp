// mrl_wide_layer and the body of mrl_agent_head (wide_policy.hip describes the workgroup and the arithmetic).  The layer kernel is a
// template on the map from a workgroup to its tile, with two instances: under WidePlainTiles (wide_policy.hip) tile blockIdx.x holds
// list positions [32 x, 32 x + 32) below *count under ONE parameter array; under WideBankTiles (wide_bank.hip) a tile is an entry
// of a bank plan's table: up to 32 list positions of ONE policy of a bank, under that policy's row.  A map is a kernel argument and
// offers
//     uint32_t end(const WideLayerArgs &a) const, uint32_t first() const    the tile's list positions [first, end); none: no tile
//     size_t shift() const                                                  floats from the arguments' weights to the tile's
// (The kernel is the template, and not a function it calls: a body inlined into two kernels reaches the arguments through a
// pointer, and the plain kernel then compiles to other instructions than it had before there was a map.  As it stands the plain
// instance's instructions are those of the kernel it replaces.)
// An output row's arithmetic reads its own input row and the tile's common weights only -- MFMA rows are independent --, so which
// other rows share its tile, and where in the tile it sits, cannot change a bit of it.
#pragma once

#include "wide_policy.hpp"
#include "random_policy.hpp"

namespace mrl {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTileRows = 32, kTileCols = 128, kChunk = 64, kLd = 66, kLayerThreads = 256;
constexpr int kStageA = kTileRows * kChunk / kLayerThreads;  // 8 elements of the input tile per thread and chunk
constexpr int kStageB = kTileCols * kChunk / kLayerThreads;  // 32 of the weight tile

__device__ __forceinline__ bool wide_nonzero(const WideInput &in, int64_t at)
{
    switch (in.type) {
    case MRL_INT8:
    case MRL_UINT8: return static_cast<const uint8_t *>(in.data)[at] != 0;
    case MRL_FLOAT32: return static_cast<const float *>(in.data)[at] != 0.0f;
    default: return static_cast<const uint32_t *>(in.data)[at] != 0u;
    }
}

// ---------------------------------------------------------------- one matrix layer

struct WideLayerNet {
    const void *in;       // (rows, K) at in_row_stride; layer 1: the simulator's tensor, indexed by world
    const float *weight;  // (out_dim, K) row-major
    const float *bias;
    float *out;           // (rows, out_stride), indexed by position in the world list
    int64_t in_row_stride;
    uint32_t in_type, K, out_dim, out_stride;
};
struct WideLayerArgs {
    WideLayerNet net[2];
    const uint32_t *rows, *count;
    uint32_t gather;  // the input rows are worlds (rows[j]) and not list positions (j)
    uint32_t relu;
};

// the plain map: tile blockIdx.x of the one list rows[0 .. *count), the arguments' own weights
struct WidePlainTiles {
    __device__ __forceinline__ uint32_t end(const WideLayerArgs &a) const { return *a.count; }
    __device__ __forceinline__ uint32_t first() const { return blockIdx.x * kTileRows; }
    __device__ __forceinline__ size_t shift() const { return 0; }
};

__device__ __forceinline__ void wide_fetch(const WideLayerNet &n, size_t shift, const int64_t (&arow)[kStageA],
                                           uint32_t col_first, uint32_t k, float (&pa)[kStageA], float (&pb)[kStageB])
{
    const bool in_k = k < n.K;
#pragma unroll
    for (int i = 0; i < kStageA; i++) pa[i] = in_k && arow[i] >= 0 ? wide_load(n.in, n.in_type, arow[i] + k) : 0.0f;
#pragma unroll
    for (int i = 0; i < kStageB; i++) {
        const uint32_t col = col_first + 4u * i;
        pb[i] = in_k && col < n.out_dim ? n.weight[shift + (size_t)col * n.K + k] : 0.0f;
    }
}

template <class Map>
__global__ void __launch_bounds__(kLayerThreads) mrl_wide_layer(WideLayerArgs a, Map map)
{
    const WideLayerNet &n = a.net[blockIdx.z];
    const uint32_t count = map.end(a);  // the tile's list positions are [row0, count), at most kTileRows of them
    const uint32_t row0 = map.first(), col0 = blockIdx.y * kTileCols;
    if (row0 >= count || col0 >= n.out_dim) return;  // (uniform over the workgroup)
    const size_t shift = map.shift();
    __shared__ float tile_a[kTileRows * kLd];
    __shared__ float tile_b[kTileCols * kLd];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;

    // staging: this thread moves k = lane of every chunk for the input rows wave + 4 i and the weight rows wave + 4 i
    int64_t arow[kStageA];
#pragma unroll
    for (int i = 0; i < kStageA; i++) {
        const uint32_t j = row0 + wave + 4u * i;
        arow[i] = j < count ? (int64_t)(a.gather ? a.rows[j] : j) * n.in_row_stride : -1;
    }
    float pa[kStageA], pb[kStageB];
    wide_fetch(n, shift, arow, col0 + wave, lane, pa, pb);

    const uint32_t col = col0 + wave * 32u + r;
    const bool live = col0 + wave * 32u < n.out_dim;  // this wavefront's 32 columns hold at least one output
    const float bias = col < n.out_dim ? n.bias[shift + col] : 0.0f;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    for (uint32_t k0 = 0; k0 < n.K; k0 += kChunk) {
#pragma unroll
        for (int i = 0; i < kStageA; i++) tile_a[(wave + 4u * i) * kLd + lane] = pa[i];
#pragma unroll
        for (int i = 0; i < kStageB; i++) tile_b[(wave + 4u * i) * kLd + lane] = pb[i];
        __syncthreads();
        if (k0 + kChunk < n.K) wide_fetch(n, shift, arow, col0 + wave, k0 + kChunk + lane, pa, pb);
        if (live) {
            const uint32_t left = n.K - k0, steps = left >= (uint32_t)kChunk ? kChunk / 2 : (left + 1u) / 2u;  // an odd tail is padded with a zero
            const float *__restrict__ pa_lds = tile_a + r * kLd + half;
            const float *__restrict__ pb_lds = tile_b + (wave * 32u + r) * kLd + half;
            for (uint32_t kk = 0; kk < steps; kk++)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa_lds[2 * kk], pb_lds[2 * kk], acc, 0, 0, 0);
        }
        __syncthreads();  // the next chunk overwrites what the products read
    }
    if (!live || col >= n.out_dim) return;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t j = row0 + (e & 3) + 8 * (e >> 2) + 4 * half;  // C/D map of the 32 x 32 tile
        if (j >= count) continue;
        const float v = acc[e] + bias;
        n.out[(size_t)j * n.out_stride + col] = a.relu ? (v > 0.0f ? v : 0.0f) : v;
    }
}

// The arguments of layer `layer` (0-3) of a forward pass; weights and biases are those of the array g.params, which a bank's map
// shifts to its policy's row.
inline WideLayerArgs wide_layer_args(const WideForwardArgs &g, uint32_t layer)
{
    // critic: parameters from 0; actor: behind them
    const uint64_t H = kWideHidden;
    const float *net_params[2] = {g.params, g.params + wide_net_params(g.S, 1)};
    const WideInput first_in[2] = {g.state, g.obs};
    const uint32_t first_k[2] = {g.S, g.D}, last_out[2] = {1u, g.A};
    WideLayerArgs la{};
    la.rows = g.rows, la.count = g.count;
    la.gather = layer == 0, la.relu = layer < 3;
    for (uint32_t net = 0; net < g.nets; net++) {
        WideLayerNet &n = la.net[net];
        const float *p = net_params[net];
        if (layer >= 1) p += (uint64_t)first_k[net] * H + H;
        if (layer >= 2) p += H * H + H;
        if (layer >= 3) p += H * H + H;
        n.K = layer == 0 ? first_k[net] : kWideHidden;
        n.out_dim = layer == 3 ? last_out[net] : kWideHidden;
        n.weight = p;
        n.bias = p + (uint64_t)n.out_dim * n.K;
        if (layer == 0) {
            n.in = first_in[net].data, n.in_row_stride = first_in[net].row_stride, n.in_type = first_in[net].type;
        } else {
            n.in = g.hidden[net][layer - 1], n.in_row_stride = (int64_t)H, n.in_type = MRL_FLOAT32;
        }
        if (layer < 3) {
            n.out = g.hidden[net][layer], n.out_stride = kWideHidden;
        } else if (net == 0) {
            n.out = g.value, n.out_stride = 1;
        } else {
            n.out = g.logits, n.out_stride = kWideMaxActions;
        }
    }
    return la;
}
// the column slabs of layer `layer`: the grid's y extent
constexpr uint32_t wide_layer_slabs(uint32_t layer) { return layer == 3 ? 1u : kWideHidden / kTileCols; }

// ---------------------------------------------------------------- the head

struct HeadArgs {
    const uint32_t *rows, *count;
    const float *logits, *value;  // (count, 64), (count)
    WideInput mask;
    int32_t *action;
    int64_t action_stride;
    mrl_agent_record rec;
    uint32_t has_record, row, flags, A, num_worlds, player, step;
    uint64_t seed;
};

// list position j, which is world w: mask, soft-max, draw, log-prob; ACTION and, with a record, its row
__device__ __forceinline__ void wide_head_body(const HeadArgs &a, uint32_t j, uint32_t w)
{
    const uint64_t N = a.num_worlds, at = (uint64_t)a.row * N + w;
    const mrl_agent_record &r = a.rec;
    if (a.flags & MRL_AGENT_VALUE_ONLY) {
        r.next_value[w] = a.value[j];
        return;
    }
    const float *__restrict__ l = a.logits + (size_t)j * kWideMaxActions;
    const int64_t mask_at = (int64_t)w * a.mask.row_stride;
    const int A = (int)a.A;
    // categorical_sample's rule (random_policy.hpp) over the legal actions only, A at run time, the logits read from memory
    float top = -INFINITY;
    int first = -1, last_legal = -1;  // the first legal arg-max, the last legal action
    for (int i = 0; i < A; i++) {
        if (!wide_nonzero(a.mask, mask_at + i)) continue;
        const float v = l[i];
        if (first < 0 || v > top) {
            top = v;
            first = i;
        }
        last_legal = i;
    }
    int action = 0;
    float logprob = -INFINITY;
    if (first >= 0) {
        float sum = 0.0f;
        for (int i = 0; i < A; i++) sum += wide_nonzero(a.mask, mask_at + i) ? expf(l[i] - top) : 0.0f;
        action = first;
        if (!(a.flags & MRL_POLICY_GREEDY)) {
            const float u = (float)(policy_hash(a.seed, a.step, w, a.player) >> 8) * 0x1p-24f;
            float cdf = 0.0f;
            action = 0;
            for (int i = 0; i < A - 1; i++) {
                cdf += (wide_nonzero(a.mask, mask_at + i) ? expf(l[i] - top) : 0.0f) / sum;
                action += u >= cdf ? 1 : 0;
            }
            if (!wide_nonzero(a.mask, mask_at + action)) action = last_legal;
        }
        logprob = (l[action] - top) - logf(sum);
    }
    a.action[(int64_t)w * a.action_stride] = action;
    if (!a.has_record) return;
    r.actions[at] = action;
    r.logprobs[at] = logprob;
    r.values[at] = a.value[j];
    if (r.logits)
        for (int i = 0; i < A; i++) r.logits[(size_t)w * kWideMaxActions + i] = l[i];
}

}  // namespace mrl
