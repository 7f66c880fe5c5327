// mrl_agent_update: the learning phase of the reference's CleanPPOAgent (pantheonrl_extension/vectoragent.py:268-330) for the
// wide policy, without torch in the loop (include/mrl_envs.h).
//
// One call is two launches up front and eleven per epoch, all on one stream:
//   mrl_update_rows    one workgroup turns record->active (T N flags) into the ascending list of active cells, as mrl_wide_rows
//                      does, but writes no entry past `capacity` -- the workspace is sized for capacity samples -- and
//                      leaves three words: B, the samples to compute (B, or 0 where the status is not 0) and the status.
//                      Every later kernel reads its sample count from the second word, so a refused batch enqueues work
//                      that leaves at once.
//   mrl_update_moments one workgroup: (mean, std + 1e-8) of the B advantages, sums in double (MRL_PPO_NORM_ADV only).
//   mrl_wide_layer x4  wide_policy.hip's forward pass over the record's own int8 / int32 rows through the list; every hidden
//                      activation is kept.
//   mrl_update_head    a lane per sample: masked soft-max with the act's expressions, log-prob, entropy, ratio, both losses,
//                      d_logits (B, 64) and d_value (B) with 1 / B folded in, and the workgroup's partial stats in double.
//   mrl_update_dx x3   dX[j][k] = (X[j][k] > 0) sum_c dY[j][c] W[c][k] for layers 4, 3, 2: mrl_wide_layer's tiling (32 rows x
//                      128 columns per workgroup, v_mfma_f32_32x32x2_f32, c ascending from 0), W read row-major.
//   mrl_update_dw      dW[c][k] = sum_j dY[j][c] X[j][k] and db[c] = sum_j dY[j][c] for all eight layers of both nets in
//                      ONE launch: a wavefront owns a 32 x 32 tile of dW (or 32 entries of db: the same product against a
//                      column of ones), the instruction's k is the sample pair, so an entry is 0, then fmaf over the samples in
//                      list order.  Every entry is written once to its place in the flat gradient vector.
//   mrl_grad_reduce, mrl_clip_adam   adam_step.hpp with one segment and groups = 1; a status other than 0 skips both.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "wide_update.hpp"

#include "adam_step.hpp"

namespace mrl {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr uint32_t kH = kWideHidden;

// ---------------------------------------------------------------- the sample list

__global__ void __launch_bounds__(1024) mrl_update_rows(const uint8_t *__restrict__ active, uint32_t cells, uint32_t capacity,
                                                        uint32_t *__restrict__ rows, uint32_t *__restrict__ words)
{
    __shared__ uint32_t wave_total[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t base = 0;
    for (uint32_t start = 0; start < cells; start += 1024u) {
        const uint32_t w = start + tid;
        const bool take = w < cells && active[w] != 0;
        const unsigned long long votes = __ballot(take);
        const uint32_t before = __popcll(votes & ((1ull << lane) - 1ull));
        if (lane == 0) wave_total[wave] = __popcll(votes);
        __syncthreads();
        uint32_t lower = 0, total = 0;
#pragma unroll
        for (uint32_t v = 0; v < 16; v++) {
            const uint32_t c = wave_total[v];
            lower += v < wave ? c : 0u;
            total += c;
        }
        const uint32_t at = base + lower + before;
        if (take && at < capacity) rows[at] = w;
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t status = base < 2u ? 1u : (base > capacity ? 2u : 0u);
        words[0] = base;
        words[1] = status ? 0u : base;
        words[2] = status;
    }
}

// ---------------------------------------------------------------- mean and std of the advantages

__global__ void __launch_bounds__(1024) mrl_update_moments(const float *__restrict__ advantages, const uint32_t *__restrict__ rows,
                                                           const uint32_t *__restrict__ words, float *__restrict__ mean_std)
{
    __shared__ double scratch[1024];
    const uint32_t count = words[1];
    if (count == 0) return;
    double sum = 0.0, squares = 0.0;
    for (uint32_t j = threadIdx.x; j < count; j += 1024u) {
        const double a = (double)advantages[rows[j]];
        sum += a;
        squares += a * a;
    }
    sum = block_sum<1024>(sum, scratch);
    squares = block_sum<1024>(squares, scratch);
    if (threadIdx.x == 0) {
        const double n = (double)count, mean = sum / n;
        const double var = (squares - sum * mean) / (n - 1.0);  // torch.std: unbiased
        mean_std[0] = (float)mean;
        mean_std[1] = (float)sqrt(var > 0.0 ? var : 0.0) + 1e-8f;
    }
}

// ---------------------------------------------------------------- the loss head

struct UpdateHeadArgs {
    const uint32_t *rows, *words;
    const float *logits, *value;  // (B, 64), (B)
    const uint8_t *masks;         // the record's (T N, A)
    const int32_t *actions;
    const float *logprobs, *values, *advantages, *returns;  // (T N)
    const float *mean_std;                                  // nullptr without MRL_PPO_NORM_ADV
    float *d_logits, *d_value;
    double *partial_stats;  // (workgroups, 8)
    uint32_t A, flags;
    float clip_coef, ent_coef, vf_coef;
};

__global__ void __launch_bounds__(kUpdateHeadThreads) mrl_update_head(UpdateHeadArgs a)
{
    __shared__ double scratch[kUpdateHeadThreads];
    const uint32_t count = a.words[1];
    if (blockIdx.x * kUpdateHeadThreads >= count) return;  // (uniform over the workgroup)
    const uint32_t j = blockIdx.x * kUpdateHeadThreads + threadIdx.x;
    double stat[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // ppo_update.hip's six sums: pg, v, entropy, -logratio, (ratio - 1) - logratio, clipped
    if (j < count) {
        const uint32_t at = a.rows[j];
        const float samples = (float)count;
        const float *__restrict__ l = a.logits + (size_t)j * kWideMaxActions;
        const uint8_t *__restrict__ legal = a.masks + (size_t)at * a.A;
        float *__restrict__ d = a.d_logits + (size_t)j * kWideMaxActions;
        const int A = (int)a.A;
        // mrl_agent_head's soft-max over the legal actions, the logits read from memory in every pass
        float top = -INFINITY;
        bool any = false;
        for (int i = 0; i < A; i++) {
            if (!legal[i]) continue;
            const float v = l[i];
            if (!any || v > top) top = v;
            any = true;
        }
        float sum = 0.0f;
        for (int i = 0; i < A; i++) sum += legal[i] ? expf(l[i] - top) : 0.0f;
        const float logsum = logf(sum);
        const int action = a.actions[at];
        // (a row with no legal action: sum = 0, log-prob NaN, as in the reference)
        const float newlogprob = (l[action] - top) - logsum;
        float entropy = 0.0f;
        for (int i = 0; i < A; i++) {
            if (!legal[i]) continue;
            const float p = expf(l[i] - top) / sum;
            entropy = fmaf(-p, (l[i] - top) - logsum, entropy);
        }
        const float logratio = newlogprob - a.logprobs[at];
        const float ratio = expf(logratio);
        float adv = a.advantages[at];
        if (a.mean_std) adv = (adv - a.mean_std[0]) / a.mean_std[1];
        const float lo = 1.0f - a.clip_coef, hi = 1.0f + a.clip_coef;
        const float pg1 = -adv * ratio, pg2 = -adv * fminf(fmaxf(ratio, lo), hi);
        // torch.max hands the gradient to the larger argument and halves it on a tie; clamp passes it inside [lo, hi]
        const float first = pg1 > pg2 ? 1.0f : (pg1 == pg2 ? 0.5f : 0.0f);
        const float through = first + (ratio >= lo && ratio <= hi ? 1.0f - first : 0.0f);
        const float g_logprob = (-adv * through) * ratio / samples;
        const float g_entropy = a.ent_coef / samples;  // of -ent_coef * mean(H): dH/dl_i = -p_i (logp_i + H)
        for (int i = 0; i < (int)kWideMaxActions; i++) {
            float g = 0.0f;
            if (i < A && legal[i]) {
                const float p = expf(l[i] - top) / sum, logp = (l[i] - top) - logsum;
                g = fmaf(g_logprob, (action == i ? 1.0f : 0.0f) - p, g_entropy * (p * (logp + entropy)));
            }
            d[i] = g;
        }
        stat[0] = (double)fmaxf(pg1, pg2);
        stat[2] = (double)entropy;
        stat[3] = (double)-logratio;
        stat[4] = (double)((ratio - 1.0f) - logratio);
        stat[5] = fabsf(ratio - 1.0f) > a.clip_coef ? 1.0 : 0.0;

        const float v = a.value[j], ret = a.returns[at];
        const float err = v - ret, plain = err * err;
        float worst = plain, g = 2.0f * err;
        if (a.flags & MRL_PPO_CLIP_VLOSS) {
            const float old = a.values[at], moved = v - old;
            const float err_c = (old + fminf(fmaxf(moved, -a.clip_coef), a.clip_coef)) - ret, clipped = err_c * err_c;
            const float lead = plain > clipped ? 1.0f : (plain == clipped ? 0.5f : 0.0f);
            const bool inside = moved >= -a.clip_coef && moved <= a.clip_coef;
            worst = fmaxf(plain, clipped);
            g = lead * (2.0f * err) + (inside ? (1.0f - lead) * (2.0f * err_c) : 0.0f);
        }
        a.d_value[j] = (a.vf_coef * 0.5f) * g / samples;
        stat[1] = (double)worst;
    }
    // the workgroup's sums: a fixed tree over its 256 terms
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double total = block_sum<(int)kUpdateHeadThreads>(stat[c], scratch);
        if (threadIdx.x == 0) a.partial_stats[(size_t)blockIdx.x * 8 + c] = total;
    }
}

// ---------------------------------------------------------------- input gradients

constexpr int kDxRows = 32, kDxCols = 128, kDxChunk = 64, kDxLdA = 66, kDxLdB = 160, kDxThreads = 256;
constexpr int kDxStageA = kDxRows * kDxChunk / kDxThreads;  // 8 elements of dY per thread and chunk
constexpr int kDxStageB = kDxCols * kDxChunk / kDxThreads;  // 32 of W

struct DxNet {
    const float *dy;      // (B, dy_stride), C columns used
    const float *weight;  // (C, 512) row-major
    const float *x;       // (B, 512): the layer's input activation, whose sign is the ReLU mask
    float *dx;            // (B, 512)
    uint32_t dy_stride, C;
};
struct DxArgs {
    DxNet net[2];
    const uint32_t *words;
};

__device__ __forceinline__ void dx_fetch(const DxNet &n, const int64_t (&arow)[kDxStageA], uint32_t c_lane, uint32_t c_first,
                                         uint32_t col, float (&pa)[kDxStageA], float (&pb)[kDxStageB])
{
#pragma unroll
    for (int i = 0; i < kDxStageA; i++) pa[i] = c_lane < n.C && arow[i] >= 0 ? n.dy[arow[i] + c_lane] : 0.0f;
#pragma unroll
    for (int i = 0; i < kDxStageB; i++) {
        const uint32_t c = c_first + 2u * i;
        pb[i] = c < n.C ? n.weight[(size_t)c * kH + col] : 0.0f;
    }
}

__global__ void __launch_bounds__(kDxThreads) mrl_update_dx(DxArgs a)
{
    const DxNet &n = a.net[blockIdx.z];
    const uint32_t count = a.words[1];
    const uint32_t row0 = blockIdx.x * kDxRows, col0 = blockIdx.y * kDxCols;
    if (row0 >= count) return;  // (uniform over the workgroup)
    __shared__ float tile_a[kDxRows * kDxLdA];   // dY: [row][c], rows 66 floats apart: lane r reads bank 2 r + half
    __shared__ float tile_b[kDxChunk * kDxLdB];  // W: [c][column], rows 160 floats apart: the two halves read banks 32 apart
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;

    // staging: this thread moves c = lane of every chunk for the dY rows wave + 4 i, and column tid & 127 of the W rows
    // (tid >> 7) + 2 i, a coalesced read of 128 consecutive floats
    int64_t arow[kDxStageA];
#pragma unroll
    for (int i = 0; i < kDxStageA; i++) {
        const uint32_t j = row0 + wave + 4u * i;
        arow[i] = j < count ? (int64_t)j * n.dy_stride : -1;
    }
    const uint32_t b_col = tid & 127u, b_c = tid >> 7;
    float pa[kDxStageA], pb[kDxStageB];
    dx_fetch(n, arow, lane, b_c, col0 + b_col, pa, pb);

    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;

    for (uint32_t c0 = 0; c0 < n.C; c0 += kDxChunk) {
#pragma unroll
        for (int i = 0; i < kDxStageA; i++) tile_a[(wave + 4u * i) * kDxLdA + lane] = pa[i];
#pragma unroll
        for (int i = 0; i < kDxStageB; i++) tile_b[(b_c + 2u * i) * kDxLdB + b_col] = pb[i];
        __syncthreads();
        if (c0 + kDxChunk < n.C) dx_fetch(n, arow, c0 + kDxChunk + lane, c0 + kDxChunk + b_c, col0 + b_col, pa, pb);
        const uint32_t left = n.C - c0, steps = left >= (uint32_t)kDxChunk ? kDxChunk / 2 : (left + 1u) / 2u;  // an odd tail meets a zero
        const float *__restrict__ pa_lds = tile_a + r * kDxLdA + half;
        const float *__restrict__ pb_lds = tile_b + half * kDxLdB + wave * 32u + r;
        for (uint32_t kk = 0; kk < steps; kk++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa_lds[2 * kk], pb_lds[2 * kk * kDxLdB], acc, 0, 0, 0);
        __syncthreads();  // the next chunk overwrites what the products read
    }
    const uint32_t col = col0 + wave * 32u + r;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t j = row0 + (e & 3) + 8 * (e >> 2) + 4 * half;  // C/D map of the 32 x 32 tile
        if (j >= count) continue;
        const size_t at = (size_t)j * kH + col;
        n.dx[at] = n.x[at] > 0.0f ? acc[e] : 0.0f;
    }
}

// ---------------------------------------------------------------- weight and bias gradients

struct DwLayer {
    const float *dy;  // (B, dy_stride), C columns used
    const void *x;    // (B, K) floats at stride 512, or, gathered, the record's rows in their element type
    float *gw, *gb;   // (C, K) and (C) in the flat gradient vector
    int64_t x_stride;
    uint32_t dy_stride, C, K, x_type, gather;
};
struct DwArgs {
    DwLayer layer[2][4];
    const uint32_t *rows, *words;
};

// MODE 0: X is an activation buffer; 1: the record's rows through the list; 2: a column of ones (the bias)
template <int MODE>
__device__ __forceinline__ f32x16 dw_tile(const DwLayer &l, const uint32_t *__restrict__ rows, uint32_t count, uint32_t c, uint32_t k,
                                          uint32_t r, uint32_t half)
{
    const bool c_ok = c < l.C, k_ok = k < l.K;
    const float *__restrict__ dy = l.dy + (c_ok ? c : 0u);
    const uint32_t kc = k_ok ? k : 0u;
    const float *__restrict__ xf = static_cast<const float *>(l.x) + kc;
    const float one = r == 0 ? 1.0f : 0.0f;
    auto x_at = [&](uint32_t j) -> float {
        if (MODE == 2) return one;
        if (MODE == 1) return wide_load(l.x, l.x_type, (int64_t)rows[j] * l.x_stride + kc);
        return xf[(size_t)j * kH];
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) acc[e] = 0.0f;
    uint32_t j = 0;
    for (; j + 16u <= count; j += 16u) {  // eight sample pairs with their loads in front of the products
        float av[8], bv[8];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++) {
            const uint32_t jj = j + 2u * u + half;
            av[u] = dy[(size_t)jj * l.dy_stride];
            bv[u] = x_at(jj);
        }
#pragma unroll
        for (uint32_t u = 0; u < 8; u++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(c_ok ? av[u] : 0.0f, k_ok || MODE == 2 ? bv[u] : 0.0f, acc, 0, 0, 0);
    }
    for (; j < count; j += 2u) {  // the ragged end: a sample past the count is a zero operand
        const uint32_t jj = j + half;
        const bool in = jj < count;
        const float av = in && c_ok ? dy[(size_t)jj * l.dy_stride] : 0.0f;
        const float bv = in && (k_ok || MODE == 2) ? x_at(jj) : 0.0f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    return acc;
}

__global__ void __launch_bounds__(256) mrl_update_dw(DwArgs a)
{
    const uint32_t count = a.words[1];
    if (count == 0) return;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, r = lane & 31u, half = lane >> 5;
    // the wavefront's tile: layers in order, within a layer the row tile of dW slowest, then the column tile, the bias last
    uint32_t tile = blockIdx.x * 4u + wave, layer = 0, k_tiles = 0;
    for (; layer < 4; layer++) {
        const DwLayer &l = a.layer[blockIdx.z][layer];
        k_tiles = (l.K + 31u) / 32u;
        const uint32_t tiles = (l.C + 31u) / 32u * (k_tiles + 1u);
        if (tile < tiles) break;
        tile -= tiles;
    }
    if (layer == 4) return;
    const DwLayer &l = a.layer[blockIdx.z][layer];
    const uint32_t c0 = tile / (k_tiles + 1u) * 32u, kt = tile % (k_tiles + 1u), k0 = kt * 32u;
    f32x16 acc;
    if (kt == k_tiles) acc = dw_tile<2>(l, a.rows, count, c0 + r, 0u, r, half);
    else if (l.gather) acc = dw_tile<1>(l, a.rows, count, c0 + r, k0 + r, r, half);
    else acc = dw_tile<0>(l, a.rows, count, c0 + r, k0 + r, r, half);
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t c = c0 + (e & 3) + 8 * (e >> 2) + 4 * half;  // C/D map of the 32 x 32 tile: row = output unit, column = lane r
        if (c >= l.C) continue;
        if (kt == k_tiles) {
            if (r == 0) l.gb[c] = acc[e];
        } else if (k0 + r < l.K) {
            l.gw[(size_t)c * l.K + k0 + r] = acc[e];
        }
    }
}

// ---------------------------------------------------------------- the stats row's end, in mrl_clip_adam

struct UpdateStatsRow {
    const double *partial_stats;
    const uint32_t *words;
    float *row;  // nullptr: no stats
    float ent_coef, vf_coef;

    __device__ void operator()(uint32_t, float total_norm) const
    {
        if (!row) return;
        const uint32_t samples = words[0], count = words[1], status = words[2];
        double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const uint32_t groups = (count + kUpdateHeadThreads - 1) / kUpdateHeadThreads;
        for (uint32_t w = 0; w < groups; w++)
            for (int c = 0; c < 6; c++) sum[c] += partial_stats[(size_t)w * 8 + c];
        const double n = count ? (double)count : 1.0;
        const double pg = sum[0] / n, v_loss = 0.5 * (sum[1] / n), entropy = sum[2] / n;
        row[0] = (float)pg;
        row[1] = (float)v_loss;
        row[2] = (float)entropy;
        row[3] = (float)(sum[3] / n);
        row[4] = (float)(sum[4] / n);
        row[5] = (float)(sum[5] / n);
        row[6] = total_norm;
        row[7] = (float)(pg - (double)ent_coef * entropy + v_loss * (double)vf_coef);
        row[8] = (float)samples;
        row[9] = (float)status;
    }
};

}  // namespace

void launch_agent_update(const AgentUpdateArgs &g, hipStream_t stream)
{
    if (g.epochs == 0) return;
    const uint32_t D = g.policy.obs_dim, S = g.policy.state_dim, A = g.policy.num_actions, n = g.capacity;
    const uint64_t critic_params = wide_net_params(S, 1);
    const uint32_t P = (uint32_t)(critic_params + wide_net_params(D, A));
    const mrl_agent_record &rec = g.record;
    const uint32_t cells = rec.num_steps * rec.num_worlds;
    const UpdateWorkspace ws = update_workspace(g.workspace, n, P);
    const bool norm = g.cfg.flags & MRL_PPO_NORM_ADV;

    hipLaunchKernelGGL(mrl_update_rows, dim3(1), dim3(1024), 0, stream, rec.active, cells, n, ws.rows, ws.words);
    if (norm) hipLaunchKernelGGL(mrl_update_moments, dim3(1), dim3(1024), 0, stream, g.advantages, ws.rows, ws.words, ws.mean_std);
    MRL_HIP(hipGetLastError());

    WideForwardArgs fwd{};
    fwd.params = g.opt.params_dev;
    fwd.obs = WideInput{rec.obs, (int64_t)D, g.obs_type};
    fwd.state = WideInput{rec.states, (int64_t)S, g.state_type};
    fwd.D = D, fwd.S = S, fwd.A = A, fwd.max_rows = n, fwd.nets = 2;
    fwd.rows = ws.rows, fwd.count = ws.words + 1;
    for (int net = 0; net < 2; net++)
        for (int layer = 0; layer < 3; layer++) fwd.hidden[net][layer] = ws.act[net][layer];
    fwd.logits = ws.logits, fwd.value = ws.value;

    UpdateHeadArgs head{};
    head.rows = ws.rows, head.words = ws.words, head.logits = ws.logits, head.value = ws.value;
    head.masks = rec.action_masks, head.actions = rec.actions, head.logprobs = rec.logprobs, head.values = rec.values;
    head.advantages = g.advantages, head.returns = g.returns, head.mean_std = norm ? ws.mean_std : nullptr;
    head.d_logits = ws.d_logits, head.d_value = ws.d_value, head.partial_stats = ws.partial_stats;
    head.A = A, head.flags = g.cfg.flags;
    head.clip_coef = g.cfg.clip_coef, head.ent_coef = g.cfg.ent_coef, head.vf_coef = g.cfg.vf_coef;

    // per net: where the layers' parameters start, critic first; a layer is its weight (out, in) and then its bias
    const uint32_t first_k[2] = {S, D}, last_out[2] = {1u, A};
    const float *dy4[2] = {ws.d_value, ws.d_logits};
    const uint32_t dy4_stride[2] = {1u, kWideMaxActions};
    DxArgs dx[3]{};  // [0]: through layer 4 into dh[.][2]; [1]: layer 3 into dh[.][1]; [2]: layer 2 into dh[.][0]
    DwArgs dw{};
    dw.rows = ws.rows, dw.words = ws.words;
    uint32_t dw_waves = 0;
    for (uint32_t net = 0; net < 2; net++) {
        uint64_t at = net ? critic_params : 0;
        uint32_t waves = 0;
        for (uint32_t layer = 0; layer < 4; layer++) {
            const uint32_t K = layer == 0 ? first_k[net] : kH, C = layer == 3 ? last_out[net] : kH;
            DwLayer &l = dw.layer[net][layer];
            l.dy = layer == 3 ? dy4[net] : ws.dh[net][layer];
            l.dy_stride = layer == 3 ? dy4_stride[net] : kH;
            l.C = C, l.K = K;
            l.gw = ws.grad + at, l.gb = ws.grad + at + (uint64_t)C * K;
            if (layer == 0) {
                l.x = net ? rec.obs : rec.states, l.x_type = net ? g.obs_type : g.state_type, l.x_stride = K, l.gather = 1;
            } else {
                l.x = ws.act[net][layer - 1], l.x_type = MRL_FLOAT32, l.x_stride = kH, l.gather = 0;
                DxNet &d = dx[3 - layer].net[net];
                d.dy = l.dy, d.dy_stride = l.dy_stride, d.C = C;
                d.weight = g.opt.params_dev + at;
                d.x = ws.act[net][layer - 1], d.dx = ws.dh[net][layer - 1];
            }
            waves += (C + 31) / 32 * ((K + 31) / 32 + 1);
            at += (uint64_t)C * K + C;
        }
        dw_waves = waves > dw_waves ? waves : dw_waves;
    }
    for (int i = 0; i < 3; i++) dx[i].words = ws.words;

    AdamStepArgs ad = adam_step_args(g.cfg.beta1, g.cfg.beta2, g.cfg.eps, g.cfg.max_grad_norm > 0.0f, g.cfg.max_grad_norm);
    ad.partial_grads = ws.grad;
    ad.grad = ws.grad_sum;
    ad.sumsq = ws.sumsq;
    ad.params = g.opt.params_dev;
    ad.exp_avg = g.opt.exp_avg;
    ad.exp_avg_sq = g.opt.exp_avg_sq;
    ad.skip = ws.words + 2;
    ad.stride = P;
    ad.segments = 1;
    ad.groups = 1;
    ad.blocks = (P + kAdamThreads - 1) / kAdamThreads;
    ad.num_params[0] = P;
    UpdateStatsRow row{ws.partial_stats, ws.words, nullptr, g.cfg.ent_coef, g.cfg.vf_coef};

    const uint32_t row_tiles = (n + kDxRows - 1) / kDxRows;
    for (uint32_t k = 0; k < g.epochs; k++) {
        launch_wide_forward(fwd, stream);
        hipLaunchKernelGGL(mrl_update_head, dim3((n + kUpdateHeadThreads - 1) / kUpdateHeadThreads), dim3(kUpdateHeadThreads), 0, stream, head);
        for (int i = 0; i < 3; i++)
            hipLaunchKernelGGL(mrl_update_dx, dim3(row_tiles, kH / kDxCols, 2), dim3(kDxThreads), 0, stream, dx[i]);
        hipLaunchKernelGGL(mrl_update_dw, dim3((dw_waves + 3) / 4, 1, 2), dim3(256), 0, stream, dw);
        MRL_HIP(hipGetLastError());
        ad.grads_row = g.grads ? g.grads + (size_t)k * P : nullptr;
        adam_set_step(ad, (double)g.opt.step + 1.0 + (double)k, {g.cfg.lr, g.cfg.lr});
        row.row = g.stats ? g.stats + (size_t)k * kUpdateStats : nullptr;
        launch_adam_step(ad, row, stream);
    }
}

}  // namespace mrl
