// mrl_mappo_mlp_update for the RECURRENT actor-critic (include/mrl_envs.h, MRL_MLPBASE_RECURRENT): MAPPO's
// update over CHUNKS of L steps with back-propagation through time.  The launch plan is mrl_mappo_mlp_update's with one launch in
// front: mrl_gru_expand_chunks writes every row's Bc L sample numbers behind the workspace, which is what the ValueNorm
// recurrence up front reads; then per row
//   mrl_mappo_gru_grad  workgroup (g, net) of four wavefronts owns chunks [g * share, (g + 1) * share) of the row for the actor
//                     (net 0) or the critic (net 1) and takes them 32 at a time.  Per tile
//                       a forward sweep, i = 0 .. L - 1: the act's forward pass (mlpbase_forward<false>, mlpbase_gru_forward: the
//                         same device functions, hence the same bits) from h0 of the chunk, with m_i = 1 - dones[j L + i]; the
//                         incoming state of every step goes to the workgroup's own slice of the workspace;
//                       a backward sweep, i = L - 1 .. 0: the step's forward pass again from its stored incoming state, the head,
//                         the loss head for the step's 32 samples (mappo_loss.hpp; every mean is over the row's Bc L samples),
//                         then back through the head, the LayerNorm, the GRU -- dh is carried to step i - 1 through z, W_hh and
//                         the mask -- and the base (mlpbase_backward.hpp).
//                       GRU, with dh' = dL/dh' (from the LayerNorm and from step i + 1):
//                         dn = dh' (1 - z), dz = dh' (h_in - n); a_n = dn (1 - n^2), a_z = dz z (1 - z), a_r = a_n gh_n r (1 - r)
//                         dgi = (a_r, a_z, a_n), dgh = (a_r, a_z, a_n r); dW_ih += dgi^T x, dW_hh += dgh^T h_in on the matrix
//                         instruction with the sample pair as k (mappo_dw_block, three each); db_ih, db_hh column sums in ascending
//                         sample order; dx = dgi W_ih, dh_in = dgh W_hh + dh' z; dh'(i - 1) += dh_in m_i.
//                     The accumulators live in the workgroup's own partial vector in global memory: a sum over the share is ONE
//                     chain -- tiles ascending, within a tile the steps DESCENDING, within a step the samples ascending -- and
//                     nothing but its owner touches the vector.  The fc_h segment is written as zeros.
//   mrl_grad_reduce, mrl_clip_adam  the optimiser tail (adam_step.hpp), a segment per net, unchanged.
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run, and a call of K
// rows gives the bits of K calls of one row.
#include "mlpbase_backward.hpp"
#include "mlpbase_gru.hpp"
#include "mappo_grad.hpp"

namespace mrl {

namespace {

static_assert(kMlpBaseHidden == kMappoHidden && kMlpBaseThreads == kMappoThreads && kMlpBaseTile == kMappoTile && kMlpLd == kMappoLd,
              "mappo_grad.hpp's functions are written for this net's width, workgroup, tile and LDS row stride");

// The gradient workgroup's LDS image: the recurrent forward image (mlpbase_gru.hpp), then dh carried from step i + 1, dL/d(head
// output) (32 x 8), the step's sample numbers and the tile's chunk ids.  The backward sweep reuses the gate arrays once the
// element-wise pass has read them: gate[3] holds dL/d(gy), then dx (the base's dy); gate[4] dL/dh', then the base's dz.
constexpr uint32_t kGruCarryAt = kGruFwdFloats, kGruDoutAt = kGruCarryAt + kGruRows, kGruSampleAt = kGruDoutAt + kMlpBaseTile * 8,
                   kGruChunkAt = kGruSampleAt + kMlpBaseTile, kGruUpdFloats = kGruChunkAt + kMlpBaseTile;
static_assert(kGruUpdFloats * 4u <= 160u * 1024u, "the recurrent gradient image fits one workgroup's LDS");
constexpr uint32_t kGruTileFloats = kMlpBaseTile * kMlpBaseHidden;  // a step's incoming states of a tile in the workspace

extern __shared__ __attribute__((aligned(16))) unsigned char gru_upd_lds_image[];

struct MappoGruGradArgs {
    MappoGradCommon common;  // obs: int32 (S, 7); indices: this row's Bc chunk ids; minibatch_size: Bc
    const float *params;
    const float *h0[2];      // (T / L, N, P, 64): chunk c starts from row c
    const float *dones;      // (S)
    float *history;          // (2, groups, L, 32, 64): every workgroup's own slice
    uint32_t layer_N, L, cells /* N P */, chunks /* (T / L) N P */, row_samples /* Bc L */;
};

// the step's sample numbers, masks and observation rows of the tile; the caller's barrier follows
__device__ __forceinline__ void gru_load_step(const MappoGruGradArgs &a, float *lds, uint32_t i, uint32_t tid)
{
    const uint32_t *chunk = reinterpret_cast<const uint32_t *>(lds + kGruChunkAt);
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + kGruSampleAt);
    const int32_t *__restrict__ obs = static_cast<const int32_t *>(a.common.obs);
    const uint32_t rr = tid >> 3, k = tid & 7u, c = chunk[rr];
    float v = 0.0f;
    if (c != kMappoAbsent) {
        const uint32_t j = c / a.cells, s = (j * a.L + i) * a.cells + (c - j * a.cells);
        if (k < kMlpBaseObs) {
            v = (float)obs[(size_t)s * kMlpBaseObs + k];
        } else {
            sample[rr] = s;
            lds[kGruKeepAt + rr] = a.dones[s] != 0.0f ? 0.0f : 1.0f;
        }
    } else if (k == kMlpBaseObs) {
        sample[rr] = kMappoAbsent;
        lds[kGruKeepAt + rr] = 0.0f;
    }
    lds[kMlpXhat0At + rr * kMlpLd0 + k] = v;
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
        const float *__restrict__ wg = w + g * kMlpBaseHidden * kMlpBaseHidden;
#pragma unroll 4
        for (uint32_t kk = 0; kk < kMappoHidden / 2u; kk++) {
            const uint32_t j = 2u * kk + half;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d[r * kMlpLd + j], wg[j * kMappoHidden + col], acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t row = tile_row(e, half);
        out[row * kMlpLd + col] = add ? (acc[e] + add[row * kMlpLd + col]) * keep[row] : acc[e];
    }
}

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mappo_gru_grad(MappoGruGradArgs a)
{
    const MappoGradCommon &c = a.common;
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x, layer_N = a.layer_N, L = a.L, out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = a.params + (net ? gru_net_params(layer_N, kMlpBaseActions) : 0u);
    float *__restrict__ grads = c.partial_grads + ((size_t)net * c.groups + blockIdx.x) * c.stride;
    float *__restrict__ history = a.history + ((size_t)net * c.groups + blockIdx.x) * L * kGruTileFloats;
    const float *__restrict__ h0 = a.h0[net];
    const float *__restrict__ head_w = params + gru_head_at(layer_N), *__restrict__ norm_w = params + gru_norm_at(layer_N);
    float *__restrict__ g_head_w = grads + gru_head_at(layer_N), *__restrict__ g_head_b = g_head_w + out_dim * kMlpBaseHidden;
    float *__restrict__ g_wih = grads + gru_wih_at(layer_N), *__restrict__ g_whh = grads + gru_whh_at(layer_N);
    float *__restrict__ g_bih = grads + gru_bih_at(layer_N), *__restrict__ g_bhh = grads + gru_bhh_at(layer_N);
    float *__restrict__ g_norm = grads + gru_norm_at(layer_N);

    float *lds = reinterpret_cast<float *>(gru_upd_lds_image);
    float *hin = lds + kGruHinAt, *gate = lds + kGruGateAt, *hn = lds + kGruHnAt, *keep = lds + kGruKeepAt, *carry = lds + kGruCarryAt;
    float *d_out = lds + kGruDoutAt, *d_gy = gate + 3u * kGruRows, *d_h = gate + 4u * kGruRows;
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + kGruSampleAt), *chunk = reinterpret_cast<uint32_t *>(lds + kGruChunkAt);
    const float *x = lds + kMlpYAt + layer_N * kMlpBaseTile * kMlpLd;

    const uint64_t begin = blockIdx.x * c.share;
    const uint64_t end = begin + c.share < c.minibatch_size ? begin + c.share : c.minibatch_size;
    const float count = (float)a.row_samples;
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    // fc_h: no forward pass reads it, so its gradient is zero
    for (uint32_t e = tid0; e < kMlpBaseBlock; e += kMlpBaseThreads) grads[kMlpBaseFcHAt + e] = 0.0f;

    for (uint64_t base = begin; base < end; base += kMlpBaseTile) {
        const uint32_t tid = opaque(tid0), lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
        if (tid < kMlpBaseTile) {
            uint32_t id = kMappoAbsent;
            if (base + tid < end) {
                id = (uint32_t)c.indices[base + tid];
                id = id < a.chunks ? id : a.chunks - 1u;  // outside the contract, but memory-safe
            }
            chunk[tid] = id;
        }
        __syncthreads();

        // ---- the forward sweep: the incoming state of every step into the workgroup's slice
#pragma unroll 1
        for (uint32_t i = 0; i < L; i++) {
            gru_load_step(a, lds, i, tid);
            __syncthreads();
            mlpbase_forward<false>(params, layer_N, out_dim, lds, wave, lane);
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kMlpBaseThreads) {
                const uint32_t rr = idx >> 6, col = idx & 63u, id = chunk[rr];
                float v = hin[rr * kMlpLd + col];  // h' of step i - 1
                if (i == 0u) v = id != kMappoAbsent ? h0[(size_t)id * kMlpBaseHidden + col] : 0.0f;
                history[(size_t)i * kGruTileFloats + idx] = v;
                hin[rr * kMlpLd + col] = v * keep[rr];
            }
            __syncthreads();
            if (i + 1u < L) mlpbase_gru_forward(params, layer_N, x, lds, tid);
        }

        // ---- the backward sweep
#pragma unroll 1
        for (uint32_t back = 0; back < L; back++) {
            const uint32_t i = L - 1u - back;
            const bool first = base == begin && back == 0u;
            if (back) {  // (step L - 1 is where the forward sweep stopped)
                gru_load_step(a, lds, i, tid);
                __syncthreads();
                mlpbase_forward<false>(params, layer_N, out_dim, lds, wave, lane);
                for (uint32_t idx = tid; idx < kGruTileFloats; idx += kMlpBaseThreads) {
                    const uint32_t rr = idx >> 6, col = idx & 63u;
                    hin[rr * kMlpLd + col] = history[(size_t)i * kGruTileFloats + idx] * keep[rr];
                }
                __syncthreads();
            }
            mlpbase_gru_forward(params, layer_N, x, lds, tid);
            // the element-wise pass left h' in hin; the backward pass needs h_in
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kMlpBaseThreads) {
                const uint32_t rr = idx >> 6, col = idx & 63u;
                hin[rr * kMlpLd + col] = history[(size_t)i * kGruTileFloats + idx] * keep[rr];
            }
            mlpbase_gru_head(params, layer_N, out_dim, lds, tid);

            mappo_loss_head<(int)kMlpBaseActions>(c, net, sample, lds + kMlpOutAt, d_out, count, stat, tid);
            __syncthreads();
            // ---- head: dW_head, db_head and dL/d(gy)
            mappo_head_backward<false>(head_w, g_head_w, g_head_b, out_dim, d_out, lds + kGruYAt, d_gy, nullptr, kMlpLd, first, tid);
            __syncthreads();
            // ---- the GRU's LayerNorm: dh' = rstd (g - mean(g) - xhat mean(g xhat)) + what step i + 1 carried here
            {
                const float weight = norm_w[lane];
                for (uint32_t row = wave; row < kMlpBaseTile; row += 4u) {
                    const float xh = hn[row * kMlpLd + lane], g = d_gy[row * kMlpLd + lane] * weight;
                    const float mean_g = wave_sum(g) / (float)kMlpBaseHidden, mean_gx = wave_sum(g * xh) / (float)kMlpBaseHidden;
                    const float dx = lds[kGruRstdAt + row] * ((g - mean_g) - xh * mean_gx);
                    d_h[row * kMlpLd + lane] = back ? dx + carry[row * kMlpLd + lane] : dx;
                }
                if (wave == 0u)
                    column_sum(g_norm, first, d_gy, hn, kMlpLd, kMlpLd, lane);
                else if (wave == 1u)
                    column_sum(g_norm + kMlpBaseHidden, first, d_gy, nullptr, kMlpLd, 0u, lane);
            }
            __syncthreads();  // dh' is complete; d_gy and the normalised rows are dead
            // ---- the gates, element-wise: gate[0], [1], [2], [5] become a_r, a_z, a_n, a_n r; hn becomes dh' z
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kMlpBaseThreads) {
                const uint32_t at = (idx >> 6) * kMlpLd + (idx & 63u);
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
                mappo_dw_block(g_wih + g * kMlpBaseHidden * kMlpBaseHidden, dgi, x, kMlpLd, first, wave, r, half);
                mappo_dw_block(g_whh + g * kMlpBaseHidden * kMlpBaseHidden, dgh, hin, kMlpLd, first, wave, r, half);
                if (wave == g)
                    column_sum(g_bih + g * kMlpBaseHidden, first, dgi, nullptr, kMlpLd, 0u, lane);
                else if (wave == ((g + 1u) & 3u))
                    column_sum(g_bhh + g * kMlpBaseHidden, first, dgh, nullptr, kMlpLd, 0u, lane);
            }
            // ---- dx on waves 0 and 1 (the base's dy); on waves 2 and 3 what step i - 1 receives: (dgh W_hh + dh' z) m_i
            if (wave < 2u)
                gru_d_in3(gate, gate + kGruRows, gate + 2u * kGruRows, params + gru_wih_at(layer_N), d_gy, nullptr, nullptr, wave, r, half);
            else if (i)
                gru_d_in3(gate, gate + kGruRows, gate + 5u * kGruRows, params + gru_whh_at(layer_N), carry, hn, keep, wave - 2u, r, half);
            __syncthreads();  // dx and the carry are complete; the gate gradients are dead
            mlpbase_backward(params, grads, layer_N, lds, d_gy, d_h, first, tid);
        }
    }

    mappo_stats_tail(c, net, reinterpret_cast<double *>(lds), stat, tid0);
}

// every row's sample numbers, (K, Bc L): chunk c = (j N + n) P + p covers samples ((j L + i) N + n) P + p, i < L
__global__ void mrl_gru_expand_chunks(const int32_t *__restrict__ chunk_ids, int32_t *__restrict__ samples, uint64_t total, uint32_t L,
                                      uint32_t cells, uint32_t chunks)
{
    const uint64_t at = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= total) return;
    const uint64_t which = at / L;
    const uint32_t i = (uint32_t)(at - which * L);
    uint32_t id = (uint32_t)chunk_ids[which];
    id = id < chunks ? id : chunks - 1u;
    const uint32_t j = id / cells;
    samples[at] = (int32_t)((j * L + i) * cells + (id - j * cells));
}

}  // namespace

GruUpdateWorkspace gru_update_workspace(uint32_t layer_N, uint32_t minibatch_size, uint32_t num_minibatches)
{
    GruUpdateWorkspace w;
    w.plain = mappo_workspace(gru_net_params(layer_N, kMlpBaseActions), minibatch_size, num_minibatches);
    w.history = w.plain.total;
    w.samples = w.history + 2 * w.plain.groups * (uint64_t)kGruMaxChunk * kGruTileFloats;
    w.total = w.samples + (((uint64_t)num_minibatches * minibatch_size * kGruMaxChunk + 3) & ~uint64_t(3));
    return w;
}

void launch_mappo_gru_update(uint32_t layer_N, const mrl_mappo_optimizer &opt, const mrl_mappo_mlp_gru_batch &batch, const int32_t *indices,
                             uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg, float *value_norm_state,
                             float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    constexpr uint32_t lds_bytes = kGruUpdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mappo_gru_grad>(lds_bytes);
    const uint32_t L = batch.chunk_length, cells = batch.num_worlds * batch.num_seats, chunks = batch.base.size / L;
    const uint32_t row_samples = minibatch_size * L;  // (Bc <= chunks, so this is at most the batch's size)
    const GruUpdateWorkspace gw = gru_update_workspace(layer_N, minibatch_size, num_minibatches);
    int32_t *samples = nullptr;
    if (cfg.flags & MRL_MAPPO_VALUENORM) {
        // ValueNorm's recurrence reads samples: every row's chunks as their Bc L sample numbers
        samples = reinterpret_cast<int32_t *>(workspace + gw.samples);
        const uint64_t total = (uint64_t)num_minibatches * row_samples;
        hipLaunchKernelGGL(mrl_gru_expand_chunks, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, indices, samples, total, L, cells,
                           chunks);
        MRL_HIP(hipGetLastError());
    }
    MappoGruGradArgs g{};
    g.params = opt.params_dev;
    g.h0[0] = batch.h0_actor, g.h0[1] = batch.h0_critic;
    g.dones = batch.dones;
    g.history = workspace + gw.history;
    g.layer_N = layer_N, g.L = L, g.cells = cells, g.chunks = chunks, g.row_samples = row_samples;
    // the row loop and the optimiser tail are the plain update's (gw.plain is its workspace for Bc a row), over chunks: ValueNorm
    // reads the expanded sample numbers and every mean runs over Bc L samples
    mappo_update_rows(gru_net_params(layer_N, kMlpBaseActions), gru_net_params(layer_N, 1), opt, batch.base, indices, num_minibatches,
                      minibatch_size, cfg, value_norm_state, workspace, stats, grads, stream, kMappoOneMember,
                      [&](const MappoGradCommon &common, uint32_t groups, const MappoMemberStrides &, uint32_t) {
                          g.common = common;
                          hipLaunchKernelGGL(mrl_mappo_gru_grad, dim3(groups, 2), dim3(kMlpBaseThreads), lds_bytes, stream, g);
                      },
                      MappoRowSamples{samples, row_samples});
}

}  // namespace mrl
