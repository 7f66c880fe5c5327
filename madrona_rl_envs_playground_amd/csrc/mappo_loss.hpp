// What MAPPO's two device updates share (cnn_update.hip for the kitchens' CNN actor-critic, mlpbase_update.hip for the balance
// beam's MLPBase one; DESIGN.md sections 16 and 18): the per-sample loss head of R_MAPPO.ppo_update (train/MAPPO/r_mappo.py:91-164),
// the accumulator tile of a weight gradient that lives in the workgroup's partial vector, the ValueNorm recurrence up front and the
// stats row's end.  The networks differ, the losses do not: one definition, so the two updates cannot drift apart.  The steps of a
// tile that use these -- sample table, loss head, the backward pass of the head and of a 64 x 64 layer -- are in mappo_grad.hpp.
#pragma once

#include "adam_step.hpp"

namespace mrl {

constexpr uint32_t kMappoMaxGroups = 256;  // workgroups per net, hence partial gradient vectors per net and row, however large B is
constexpr uint32_t kMappoStats = 8;        // columns of a stats row
constexpr uint32_t kMappoKnownFlags = MRL_MAPPO_VALUENORM | MRL_MAPPO_HUBER_LOSS | MRL_MAPPO_CLIPPED_VALUE_LOSS | MRL_MAPPO_MAX_GRAD_NORM;
constexpr uint32_t kMappoTile = 32;        // samples per tile of either gradient kernel

typedef float mappo_f32x16 __attribute__((ext_vector_type(16)));

// the value the compiler must take as new: keeps per-lane address arithmetic of the tile loop's body inside the loop (hoisted, the
// addresses of every accumulator element of every phase would be live across the whole body and spill)
__device__ __forceinline__ uint32_t opaque(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// the C/D map of the 32 x 32 tile: element e of lane (r, half) is row (e & 3) + 8 (e >> 2) + 4 half, column r
__device__ __forceinline__ uint32_t tile_row(int e, uint32_t half) { return (e & 3) + 8 * (e >> 2) + 4 * half; }

// the accumulator of C[row0 + row][col] as the previous tile left it in the partial vector (0 before the first tile)
__device__ __forceinline__ mappo_f32x16 acc_load(const float *__restrict__ g, uint32_t ld, uint32_t rows, uint32_t col, bool col_ok, bool first,
                                                 uint32_t half)
{
    mappo_f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t row = tile_row(e, half);
        acc[e] = !first && col_ok && row < rows ? g[(size_t)row * ld + col] : 0.0f;
    }
    return acc;
}

__device__ __forceinline__ void acc_store(float *__restrict__ g, uint32_t ld, uint32_t rows, uint32_t col, bool col_ok, uint32_t half,
                                          const mappo_f32x16 &acc)
{
#pragma unroll
    for (int e = 0; e < 16; e++) {
        const uint32_t row = tile_row(e, half);
        if (col_ok && row < rows) g[(size_t)row * ld + col] = acc[e];
    }
}

// the reference's huber_loss (utils/util.py:46-50) or mse_loss and its derivative in e
__device__ __forceinline__ float value_term(float e, float delta, bool huber, float &slope)
{
    if (!huber || fabsf(e) <= delta) {
        slope = e;
        return e * e / 2.0f;
    }
    if (e > delta) {
        slope = delta;
        return delta * (fabsf(e) - delta / 2.0f);
    }
    slope = 0.0f;  // e < -delta: neither mask of huber_loss is set
    return 0.0f;
}

// the loss's own numbers, as they cross the C ABI
struct MappoLoss {
    float clip_param, entropy_coef, value_loss_coef, huber_delta;
    uint32_t flags;
};

// The actor's sample: d[i] = dLoss / d(logit i) of -mean(min(ratio A, clamp(ratio) A)) - entropy_coef mean(H) over `count` samples,
// and the sample's terms of the four sums (surrogate, entropy, ratio, clipped).  The soft-max is categorical_sample's
// (random_policy.hpp) with every log-prob kept: logf as there, so that the new log-prob of the recorded action is the act's bit
// for bit.
template <int A>
__device__ __forceinline__ void mappo_actor_sample(const float (&lg)[A], int action, float old_logprob, float adv, const MappoLoss &c,
                                                   float count, float (&d)[A], double (&stat)[4])
{
    float top = lg[0];
#pragma unroll
    for (int i = 1; i < A; i++) top = lg[i] > top ? lg[i] : top;
    float e[A], sum = 0.0f;
#pragma unroll
    for (int i = 0; i < A; i++) {
        e[i] = expf(lg[i] - top);
        sum += e[i];
    }
    const float logsum = logf(sum);
    float logp[A], prob[A], entropy = 0.0f, newlogprob = 0.0f;
#pragma unroll
    for (int i = 0; i < A; i++) {
        logp[i] = (lg[i] - top) - logsum;  // the act's log-prob
        prob[i] = e[i] / sum;
        entropy = fmaf(-prob[i], logp[i], entropy);
        newlogprob = action == i ? logp[i] : newlogprob;
    }
    const float ratio = expf(newlogprob - old_logprob);
    const float lo = 1.0f - c.clip_param, hi = 1.0f + c.clip_param;
    const float surr1 = ratio * adv, surr2 = fminf(fmaxf(ratio, lo), hi) * adv;
    // torch.min hands the gradient to the smaller argument and halves it on a tie; clamp passes it inside [lo, hi]
    const float one = surr1 < surr2 ? 1.0f : (surr1 == surr2 ? 0.5f : 0.0f);
    const float through = one + (ratio >= lo && ratio <= hi ? 1.0f - one : 0.0f);
    const float g_logprob = (-adv * through) * ratio / count;
    const float g_entropy = c.entropy_coef / count;  // of -entropy_coef * mean(H): dH/dl_i = -p_i (logp_i + H)
#pragma unroll
    for (int i = 0; i < A; i++)
        d[i] = fmaf(g_logprob, (action == i ? 1.0f : 0.0f) - prob[i], g_entropy * (prob[i] * (logp[i] + entropy)));
    stat[0] += (double)fminf(surr1, surr2);
    stat[1] += (double)entropy;
    stat[2] += (double)ratio;
    stat[3] += fabsf(ratio - 1.0f) > c.clip_param ? 1.0 : 0.0;
}

// The critic's sample: dLoss / dv of value_loss_coef mean(max(L(e), L(e_c))) (or mean(L(e))) over `count` samples, and the
// sample's term of the value loss.  row_norm: this row's ValueNorm (mean, sqrt(var)), or nullptr.
__device__ __forceinline__ float mappo_critic_sample(float v, float old, float target, const float *__restrict__ row_norm, const MappoLoss &c,
                                                     float count, double (&stat)[4])
{
    const bool huber = c.flags & MRL_MAPPO_HUBER_LOSS;
    if (row_norm) target = (target - row_norm[0]) / row_norm[1];
    float slope, slope_c;
    const float plain = value_term(target - v, c.huber_delta, huber, slope);
    float worst = plain, g = -slope;
    if (c.flags & MRL_MAPPO_CLIPPED_VALUE_LOSS) {
        const float moved = v - old;
        const float near = old + fminf(fmaxf(moved, -c.clip_param), c.clip_param);
        const float clipped = value_term(target - near, c.huber_delta, huber, slope_c);
        const float one = plain > clipped ? 1.0f : (plain == clipped ? 0.5f : 0.0f);
        const bool inside = moved >= -c.clip_param && moved <= c.clip_param;
        worst = fmaxf(plain, clipped);
        g = one * -slope + (inside ? (1.0f - one) * -slope_c : 0.0f);
    }
    stat[0] += (double)worst;
    return c.value_loss_coef * g / count;
}

// The stats row's end, in mrl_clip_adam: the net's columns from its workgroups' four sums and its total norm
struct MappoStatsRow {
    const double *partial_stats;
    float *row;  // nullptr: no stats
    uint32_t groups, minibatch_size;

    __device__ void operator()(uint32_t net, float total_norm) const
    {
        if (!row) return;
        double sum[4] = {0.0, 0.0, 0.0, 0.0};
        for (uint32_t w = 0; w < groups; w++)
            for (int c = 0; c < 4; c++) sum[c] += partial_stats[((size_t)net * groups + w) * kMappoStats + c];
        const double count = (double)minibatch_size;
        if (net) {
            row[0] = (float)(sum[0] / count);
            row[1] = total_norm;
        } else {
            row[2] = (float)(-(sum[0] / count));
            row[3] = (float)(sum[1] / count);
            row[4] = total_norm;
            row[5] = (float)(sum[2] / count);
            row[6] = (float)(sum[3] / count);
            row[7] = 0.0f;
        }
    }
};

// MappoStatsRow for member blockIdx.z of a bank update: the first member's, moved member_partial doubles / member_row floats per member
struct MappoBankStatsRow {
    MappoStatsRow first;
    uint64_t member_partial, member_row;

    __device__ void operator()(uint32_t net, float total_norm) const
    {
        if (!first.row) return;
        MappoStatsRow own = first;
        own.partial_stats += (size_t)blockIdx.z * member_partial;
        own.row += (size_t)blockIdx.z * member_row;
        own(net, total_norm);
    }
};

// The caller's scratch, in floats: every row's ValueNorm (mean, sqrt(var)) and (mean, mean of squares) of its returns; the
// workgroups' partial gradient vectors (2 nets, groups, stride) and partial stats (2, groups, 8 doubles); the summed gradient
// (2, stride); the reduce launch's per-block sums of g^2 (2, blocks).  stride = the actor's parameter count, padded.
struct MappoWorkspace {
    uint64_t row_norm, row_sums, partial_grads, partial_stats, grad, sumsq, total;
    uint64_t stride, groups, blocks;
};

inline MappoWorkspace mappo_workspace(uint64_t actor_params, uint32_t minibatch_size, uint32_t num_minibatches)
{
    const auto pad = [](uint64_t n) { return (n + 3) & ~uint64_t(3); };  // every array on a 16-byte boundary
    const uint64_t tiles = ((uint64_t)minibatch_size + kMappoTile - 1) / kMappoTile;
    MappoWorkspace w;
    w.groups = tiles < kMappoMaxGroups ? tiles : kMappoMaxGroups;  // room for min(tiles, cap); share_samples may use fewer
    w.stride = pad(actor_params);
    w.blocks = (w.stride + kAdamThreads - 1) / kAdamThreads;
    w.row_norm = 0;
    w.row_sums = w.row_norm + pad(2 * (uint64_t)num_minibatches);
    w.partial_grads = w.row_sums + pad(2 * (uint64_t)num_minibatches);
    w.partial_stats = w.partial_grads + 2 * w.groups * w.stride;
    w.grad = w.partial_stats + pad(2 * 2 * w.groups * kMappoStats);
    w.sumsq = w.grad + 2 * w.stride;
    w.total = w.sumsq + pad(2 * w.blocks);
    return w;
}

// The members of a policy bank that one update call trains (mrl_mappo_bank_update, mrl_mappo_mlp_bank_update; DESIGN.md section
// 22): `count` consecutive bank rows, params_stride floats apart in the parameters and in both moments.  Every array a member has
// of its own follows the previous member's: indices (M, K, B), the ValueNorm state (M, 3), stats (M, K, 8), grads (M, K, P) and
// the workspace, M times mappo_workspace().total floats.  The plain calls train one member.
struct MappoMembers {
    uint32_t count;
    uint64_t params_stride;
};
constexpr MappoMembers kMappoOneMember{1, 0};

// ValueNorm's K-row recurrence, two launches up front (cnn_update.hip): every row's (mean, sqrt(var)) into row_norm (K, 2), the
// final state into `state`; row_sums (K, 2) is scratch.  With `members` members each runs its own recurrence on its own rows of
// indices and its own state; row_sums and row_norm of a member lie member_scratch floats behind the previous member's.
void launch_mappo_value_norm(const float *returns, const int32_t *indices, uint32_t num_minibatches, uint32_t minibatch_size,
                             uint32_t batch_size, const mrl_mappo_config &cfg, float *state, float *row_sums, float *row_norm,
                             hipStream_t stream, uint32_t members = 1, uint64_t member_scratch = 0);

}  // namespace mrl
