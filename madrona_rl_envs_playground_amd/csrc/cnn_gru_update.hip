// mrl_mappo_update for the RECURRENT CNN actor-critic (include/mrl_envs.h, MRL_CNN_RECURRENT; cnn_gru.hpp):
// MAPPO's update over CHUNKS of L steps with back-propagation through time.  The launch plan is mrl_mappo_update's with one launch
// in front: mrl_cnn_gru_expand_chunks writes every row's Bc L sample numbers behind the workspace, which is what the ValueNorm
// recurrence up front reads; then per row
//   mrl_mappo_cnn_gru_grad  workgroup (g, net) of four wavefronts owns chunks [g * share, (g + 1) * share) of the row for the actor
//                     (net 0) or the critic (net 1) and takes them 32 at a time.  dW_fc1 needs the activation image, dW_conv
//                     the int8 rows, and neither fits one workgroup's LDS together with the GRU's arrays in a large kitchen,
//                     so a tile goes through three phases that never hold both (the images are in cnn_gru.hpp):
//                       the forward sweep, i = 0 .. L - 1: CNNBase (cnn_gru_base: the act's device functions, hence its bits) for
//                         x_i, then the GRU from the step's incoming state with m_i = 1 - dones[j L + i].  x_i and the incoming
//                         state go to the workgroup's own slice of the workspace (2 L tiles of 32 x 64 floats; nobody else
//                         touches it, and every element is read back by the thread that wrote it);
//                       the recurrent phase, i = L - 1 .. 0, with only the GRU image, the head and the loss head in LDS: x_i and
//                         the incoming state from the slice, the GRU, its LayerNorm and the head again, the loss head for the
//                         step's 32 samples (mappo_loss.hpp; every mean is over the row's Bc L samples), then back through the
//                         head, the LayerNorm and the GRU (gru_step_backward, the beam's own) -- dh is carried to step i - 1
//                         through z, W_hh and the mask --; dL/dx_i is written over x_i in the slice;
//                       the convolutional phase, i = 0 .. L - 1, with only the plain update's image in LDS: CNNBase again for the
//                         ReLU signs, h1 and the activation image, then the plain update's backward path from fc2 down to dW_conv
//                         (cnn_gru_base_backward: mrl_mappo_grad's statements), which starts from dL/dx_i behind fc2's ReLU.
//                     The accumulators live in the workgroup's own partial vector in global memory: a sum over the share is ONE
//                     chain -- tiles ascending; within a tile the GRU's and the head's terms by steps DESCENDING and CNNBase's by
//                     steps ASCENDING; within a step the samples ascending -- and nothing but its owner touches the vector.
//   mrl_grad_reduce, mrl_clip_adam  the optimiser tail (adam_step.hpp), a segment per net, unchanged.
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run, and a call of K
// rows gives the bits of K calls of one row.
#include "cnn_gru.hpp"
#include "mappo_grad.hpp"

namespace mrl {

namespace {

struct MappoCnnGruGradArgs {
    MappoGradCommon common;  // obs: int8 (S, H, W, F); indices: this row's Bc chunk ids; minibatch_size: Bc
    CnnActArgs fwd;          // W, H, F and the LDS image of CNNBase (cnn_update_lds's); params
    const float *h0[2];      // (T / L, N, P, 64): chunk c starts from row c
    const float *dones;      // (S)
    float *slices;           // (2, groups, L, 2, 32, 64): every workgroup's own
    uint32_t tail_at, L, cells /* N P */, chunks /* (T / L) N P */, row_samples /* Bc L */;
};

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_gru_upd_lds_image[];

// The plain update's backward path from fc2 down to dW_conv for one tile, on the image cnn_gru_base left and d_h2 = dL/d(fc2's
// pre-activation) complete behind a barrier: mrl_mappo_grad's statements (cnn_update.hip), which keeps its own copy in line so
// that the plain update compiles to the instructions it had.  `first`: nothing has been accumulated yet.  Ends behind a barrier.
template <class RowAddress>
__device__ __forceinline__ void cnn_gru_base_backward(const CnnActArgs &f, unsigned char *lds, const RowAddress &row_address, uint32_t *shifts,
                                                      const float *__restrict__ net, float *__restrict__ g_net, const CnnGruNetAt &at,
                                                      bool first, uint32_t tid)
{
    const CnnLds &l = f.lds;
    const uint32_t lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t k1 = l.k1, npos = l.npos, K2 = kCnnChannels * npos, act_ld = l.act_ld;
    const float *__restrict__ fc1_w = net + at.fc1_w, *__restrict__ fc2_w = net + at.fc2_w;
    float *__restrict__ g_conv_w = g_net, *__restrict__ g_conv_b = g_net + at.conv_b, *__restrict__ g_fc1_w = g_net + at.fc1_w;
    float *__restrict__ g_fc1_b = g_net + at.fc1_b, *__restrict__ g_fc2_w = g_net + at.fc2_w, *__restrict__ g_fc2_b = g_net + at.fc2_b;
    const uint16_t *koff = reinterpret_cast<const uint16_t *>(lds + l.koff_at);
    float *act = reinterpret_cast<float *>(lds + l.act_at), *h1 = reinterpret_cast<float *>(lds + kCnnH1At);
    float *d_h2 = reinterpret_cast<float *>(lds + kUpdDh2At), *d_h1 = reinterpret_cast<float *>(lds + kUpdDh1At);

    // ---- fc2: dW_fc2 = d_h2^T h1; d_h1 behind fc1's ReLU on waves 0 and 1; db_fc2
    mappo_dw_block(g_fc2_w, d_h2, h1, kCnnFcLd, first, wave, r, half);
    if (wave < 2u)
        mappo_d_in<true>(d_h2, fc2_w, d_h1, h1, kCnnFcLd, wave, r, half);
    else if (wave == 2u)
        column_sum(g_fc2_b, first, d_h2, nullptr, kCnnFcLd, 0u, lane);
    __syncthreads();

    // ---- fc1: dW_fc1 = d_h1^T act (64 x 32 npos) while act is intact: wave w takes the column slabs w, w + 4, ..., both row
    // blocks of a slab on one read of act
#pragma unroll 1
    for (uint32_t ct = wave; ct < npos; ct += 4u) {
        const uint32_t col = 32u * ct + r;
        float *__restrict__ g0 = g_fc1_w, *__restrict__ g1 = g_fc1_w + (size_t)32u * K2;
        f32x16 acc0 = acc_load(g0, K2, 32u, col, true, first, half), acc1 = acc_load(g1, K2, 32u, col, true, first, half);
#pragma unroll 4
        for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
            const uint32_t s = 2u * kk + half;
            const float b = act[s * act_ld + col];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[s * kCnnFcLd + r], b, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[s * kCnnFcLd + 32u + r], b, acc1, 0, 0, 0);
        }
        acc_store(g0, K2, 32u, col, true, half, acc0);
        acc_store(g1, K2, 32u, col, true, half, acc1);
    }
    if (wave == 3u) column_sum(g_fc1_b, first, d_h1, nullptr, kCnnFcLd, 0u, lane);
    __syncthreads();
    // act in place becomes dL/d(conv pre-activation) = (act > 0) sum_j d_h1[sample][j] W_fc1[j][.]: rows samples, k = units
#pragma unroll 1
    for (uint32_t ct = wave; ct < npos; ct += 4u) {
        const uint32_t col = 32u * ct + r;
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; e++) acc[e] = 0.0f;
#pragma unroll 4
        for (uint32_t kk = 0; kk < kCnnHidden / 2u; kk++) {
            const uint32_t j = 2u * kk + half;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(d_h1[r * kCnnFcLd + j], fc1_w[(size_t)j * K2 + col], acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 16; e++) {
            float *p = act + tile_row(e, half) * act_ld + col;
            *p = *p > 0.0f ? acc[e] : 0.0f;
        }
    }
    __syncthreads();  // d_h1 and everything else in region A is dead

    // ---- convolution: the observation rows again (out of L2), then dW_conv[c][k] = sum over (position, sample) of
    // d_conv[sample][c][position] * patch[sample][position][k]: rows channels, columns k in slabs of 32, wave w takes slabs w, w + 4
    cnn_load_tile(f, lds, row_address, shifts, net, false);
    __syncthreads();
    {
        const uint32_t hh = f.H - 2u, slabs = (k1 + 31u) / 32u;
#pragma unroll 1
        for (uint32_t kt = wave; kt < slabs; kt += 4u) {
            const uint32_t k = 32u * kt + r;
            const bool ok = k < k1;
            const uint32_t off = ok ? koff[k] : 0u;
            f32x16 acc = acc_load(g_conv_w, k1, kCnnChannels, k, ok, first, half);
#pragma unroll 1
            for (uint32_t pos = 0; pos < npos; pos++) {
                const uint32_t ow = pos / hh, oh = pos - ow * hh, where = (oh * f.W + ow) * f.F + off;
#pragma unroll 4
                for (uint32_t kk = 0; kk < kCnnTile / 2u; kk++) {
                    const uint32_t s = 2u * kk + half;
                    const int8_t byte = reinterpret_cast<const int8_t *>(lds)[s * l.obs_ld + shifts[s] + where];
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(act[s * act_ld + r * npos + pos], ok ? (float)byte : 0.0f, acc, 0, 0, 0);
                }
            }
            acc_store(g_conv_w, k1, kCnnChannels, k, ok, half, acc);
        }
        if (slabs % 4u == wave && lane < kCnnChannels) {  // the wave with the fewest slabs: db_conv
            float sum = first ? 0.0f : g_conv_b[lane];
            for (uint32_t s = 0; s < kCnnTile; s++)
                for (uint32_t pos = 0; pos < npos; pos++) sum += act[s * act_ld + lane * npos + pos];
            g_conv_b[lane] = sum;
        }
    }
    __syncthreads();  // the next step overwrites what the loops above read
}

__global__ void __launch_bounds__(kCnnThreads) mrl_mappo_cnn_gru_grad(MappoCnnGruGradArgs a)
{
    const MappoGradCommon &c = a.common;
    const CnnActArgs &f = a.fwd;
    const uint32_t net = blockIdx.y;  // 0 the actor, 1 the critic
    const uint32_t tid0 = threadIdx.x, L = a.L, out_dim = net ? 1u : kCnnActions;
    const uint32_t S = f.W * f.H * f.F;
    const CnnGruNetAt at = cnn_gru_net_at(f.lds.k1, kCnnChannels * f.lds.npos, out_dim);
    const float *__restrict__ params = f.params + (net ? cnn_gru_net_params(f.W, f.H, f.F, kCnnActions) : 0);
    float *__restrict__ grads = c.partial_grads + ((size_t)net * c.groups + blockIdx.x) * c.stride;
    // step i of the tile: x_i (later dL/dx_i) at slice + 2 i tiles, the incoming state one tile behind it
    float *__restrict__ slice = a.slices + ((size_t)net * c.groups + blockIdx.x) * L * 2u * kGruTileFloats;
    const float *__restrict__ h0 = a.h0[net];

    unsigned char *lds = cnn_gru_upd_lds_image;
    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt), *d_out = reinterpret_cast<float *>(lds + kUpdDoutAt);
    float *d_h2 = reinterpret_cast<float *>(lds + kUpdDh2At);
    float *img = reinterpret_cast<float *>(lds + kCnnGruUpdImgAt), *carry = reinterpret_cast<float *>(lds + kCnnGruCarryAt);
    float *hin = img + kGruImgHin, *keep = img + kGruImgKeep, *d_x = img + kGruImgGate + 3u * kGruRows;
    uint32_t *sample = reinterpret_cast<uint32_t *>(lds + kCnnGruSampleAt);
    uint32_t *chunk_id = reinterpret_cast<uint32_t *>(lds + a.tail_at), *shifts = chunk_id + kCnnTile;

    const uint64_t begin = blockIdx.x * c.share;
    const uint64_t end = begin + c.share < c.minibatch_size ? begin + c.share : c.minibatch_size;
    const float count = (float)a.row_samples;
    double stat[4] = {0.0, 0.0, 0.0, 0.0};  // lanes 0..31 of wave 0: this lane's samples

    // chunk id -> the sample number of its step i
    const auto step_sample = [&](uint32_t id, uint32_t i) -> uint32_t {
        const uint32_t j = id / a.cells;
        return (j * L + i) * a.cells + (id - j * a.cells);
    };

    for (uint64_t base = begin; base < end; base += kCnnTile) {
        const uint32_t tid = opaque(tid0);
        if (tid < kCnnTile) {
            uint32_t id = kMappoAbsent;
            if (base + tid < end) {
                id = (uint32_t)c.indices[base + tid];
                id = id < a.chunks ? id : a.chunks - 1u;  // outside the contract, but memory-safe
            }
            chunk_id[tid] = id;
        }
        __syncthreads();

        // ---- the forward sweep: x_i and the incoming state of every step into the workgroup's slice
#pragma unroll 1
        for (uint32_t i = 0; i < L; i++) {
            const auto row_address = [&](uint32_t rr) -> const uint8_t * {
                const uint32_t id = chunk_id[rr];
                return id == kMappoAbsent ? nullptr : static_cast<const uint8_t *>(c.obs) + (size_t)step_sample(id, i) * S;
            };
            cnn_gru_base(f, lds, row_address, shifts, params, at, tid);
            float *__restrict__ xs = slice + (size_t)i * 2u * kGruTileFloats, *__restrict__ hs = xs + kGruTileFloats;
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
                const uint32_t rr = idx >> 6, col = idx & 63u, id = chunk_id[rr];
                xs[idx] = h2[rr * kGruLd + col];
                float v, m = 0.0f;
                if (i == 0u) {
                    v = id != kMappoAbsent ? h0[(size_t)id * kCnnHidden + col] : 0.0f;
                    hs[idx] = v;
                } else {
                    v = hs[idx];  // h' of step i - 1: this thread stored it
                }
                if (id != kMappoAbsent) m = a.dones[step_sample(id, i)] != 0.0f ? 0.0f : 1.0f;
                hin[rr * kGruLd + col] = v * m;
            }
            __syncthreads();
            if (i + 1u < L) {
                gru_step_forward(params + at.gru, h2, chunk, img, tid);
                for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads)
                    hs[2u * kGruTileFloats + idx] = hin[(idx >> 6) * kGruLd + (idx & 63u)];
                __syncthreads();  // the next step's rows overwrite the GRU image
            }
        }

        // ---- the recurrent phase: only the GRU image, the head and the loss head are in LDS
#pragma unroll 1
        for (uint32_t back = 0; back < L; back++) {
            const uint32_t i = L - 1u - back;
            const bool first = base == begin && back == 0u;
            float *__restrict__ xs = slice + (size_t)i * 2u * kGruTileFloats;
            const float *__restrict__ hs = xs + kGruTileFloats;
            if (tid < kCnnTile) {
                const uint32_t id = chunk_id[tid];
                uint32_t s = kMappoAbsent;
                float m = 0.0f;
                if (id != kMappoAbsent) {
                    s = step_sample(id, i);
                    m = a.dones[s] != 0.0f ? 0.0f : 1.0f;
                }
                sample[tid] = s;
                keep[tid] = m;
            }
            __syncthreads();
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
                const uint32_t rr = idx >> 6, col = idx & 63u;
                h2[rr * kGruLd + col] = xs[idx];
                hin[rr * kGruLd + col] = hs[idx] * keep[rr];
            }
            __syncthreads();
            gru_step_forward(params + at.gru, h2, chunk, img, tid);
            // the element-wise pass left h' in hin; the backward pass needs h_in
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
                const uint32_t rr = idx >> 6, col = idx & 63u;
                hin[rr * kGruLd + col] = hs[idx] * keep[rr];
            }
            gru_step_head(params + at.head_w, out_dim, chunk, img, outs, tid);
            mappo_loss_head<(int)kCnnActions>(c, net, sample, outs, d_out, count, stat, tid);
            __syncthreads();
            gru_step_backward(params + at.gru, grads + at.gru, params + at.head_w, grads + at.head_w, grads + at.head_b, out_dim, d_out, h2, img,
                              carry, back != 0u, i != 0u, first, tid);
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) xs[idx] = d_x[(idx >> 6) * kGruLd + (idx & 63u)];
            __syncthreads();  // the next step overwrites x and the image
        }

        // ---- the convolutional phase: only the plain update's image is in LDS
#pragma unroll 1
        for (uint32_t i = 0; i < L; i++) {
            const bool first = base == begin && i == 0u;
            const auto row_address = [&](uint32_t rr) -> const uint8_t * {
                const uint32_t id = chunk_id[rr];
                return id == kMappoAbsent ? nullptr : static_cast<const uint8_t *>(c.obs) + (size_t)step_sample(id, i) * S;
            };
            cnn_gru_base(f, lds, row_address, shifts, params, at, tid);
            const float *__restrict__ dxs = slice + (size_t)i * 2u * kGruTileFloats;
            for (uint32_t idx = tid; idx < kGruTileFloats; idx += kCnnThreads) {
                const uint32_t where = (idx >> 6) * kGruLd + (idx & 63u);
                d_h2[where] = h2[where] > 0.0f ? dxs[idx] : 0.0f;  // behind fc2's ReLU
            }
            __syncthreads();
            cnn_gru_base_backward(f, lds, row_address, shifts, params, grads, at, first, tid);
        }
    }

    mappo_stats_tail(c, net, reinterpret_cast<double *>(lds), stat, tid0);
}

// every row's sample numbers, (K, Bc L): chunk c = j (N P) + cell covers samples (j L + i) N P + cell, i < L
__global__ void mrl_cnn_gru_expand_chunks(const int32_t *__restrict__ chunk_ids, int32_t *__restrict__ samples, uint64_t total, uint32_t L,
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

CnnGruUpdateWorkspace cnn_gru_update_workspace(uint32_t W, uint32_t H, uint32_t F, uint32_t minibatch_size, uint32_t num_minibatches)
{
    CnnGruUpdateWorkspace w;
    w.plain = mappo_workspace(cnn_gru_net_params(W, H, F, kCnnActions), minibatch_size, num_minibatches);
    w.slices = w.plain.total;
    w.samples = w.slices + 2 * w.plain.groups * (uint64_t)kCnnGruMaxChunk * 2u * kGruTileFloats;
    w.total = w.samples + (((uint64_t)num_minibatches * minibatch_size * kCnnGruMaxChunk + 3) & ~uint64_t(3));
    return w;
}

void launch_mappo_cnn_gru_update(const mrl_mappo_policy &policy, const mrl_mappo_optimizer &opt, const mrl_mappo_gru_batch &batch,
                                 const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config &cfg,
                                 float *value_norm_state, float *workspace, float *stats, float *grads, hipStream_t stream)
{
    if (num_minibatches == 0) return;
    const uint32_t W = policy.width, H = policy.height, F = policy.channels;
    const CnnGruUpdateLds lds = cnn_gru_update_lds(W, H, F);
    allow_large_dynamic_lds<&mrl_mappo_cnn_gru_grad>(lds.total);
    const uint32_t L = batch.chunk_length, cells = batch.num_worlds * batch.num_players, chunks = batch.base.size / L;
    const uint32_t row_samples = minibatch_size * L;  // (Bc <= chunks, so this is at most the batch's size)
    const CnnGruUpdateWorkspace gw = cnn_gru_update_workspace(W, H, F, minibatch_size, num_minibatches);
    int32_t *samples = nullptr;
    if (cfg.flags & MRL_MAPPO_VALUENORM) {
        // ValueNorm's recurrence reads samples: every row's chunks as their Bc L sample numbers
        samples = reinterpret_cast<int32_t *>(workspace + gw.samples);
        const uint64_t total = (uint64_t)num_minibatches * row_samples;
        hipLaunchKernelGGL(mrl_cnn_gru_expand_chunks, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, stream, indices, samples, total, L,
                           cells, chunks);
        MRL_HIP(hipGetLastError());
    }
    MappoCnnGruGradArgs g{};
    g.fwd.params = opt.params_dev;
    g.fwd.W = W, g.fwd.H = H, g.fwd.F = F;
    g.fwd.lds = lds.fwd;
    g.h0[0] = batch.h0_actor, g.h0[1] = batch.h0_critic;
    g.dones = batch.dones;
    g.slices = workspace + gw.slices;
    g.tail_at = lds.tail_at, g.L = L, g.cells = cells, g.chunks = chunks, g.row_samples = row_samples;
    // the row loop and the optimiser tail are the plain update's (gw.plain is its workspace for Bc a row), over chunks: ValueNorm
    // reads the expanded sample numbers and every mean runs over Bc L samples
    mappo_update_rows((uint32_t)cnn_gru_net_params(W, H, F, kCnnActions), (uint32_t)cnn_gru_net_params(W, H, F, 1), opt, batch.base, indices,
                      num_minibatches, minibatch_size, cfg, value_norm_state, workspace, stats, grads, stream, kMappoOneMember,
                      [&](const MappoGradCommon &common, uint32_t groups, const MappoMemberStrides &, uint32_t) {
                          g.common = common;
                          hipLaunchKernelGGL(mrl_mappo_cnn_gru_grad, dim3(groups, 2), dim3(kCnnThreads), lds.total, stream, g);
                      },
                      MappoRowSamples{samples, row_samples});
}

}  // namespace mrl
