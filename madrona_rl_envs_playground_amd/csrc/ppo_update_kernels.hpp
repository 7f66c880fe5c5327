// mrl_ppo_update: the update phase of PPO for the Cartpole / Acrobot actor-critic, and for the same agent on the balance beam
// (D = 7, A = 4), without torch in the loop (include/mrl_envs.h, mrl_ppo_update; DESIGN.md sections 13 and 25).
//
// The reference's trainer runs, per minibatch, a gather, two forward passes, Categorical, the clipped losses, backward(),
// clip_grad_norm_ and Adam.step() in torch (scripts/cartpole_train_torch.py:275-315).  Here one row is THREE launches,
// after ONE launch up front for the mean and std of every row's advantages (they depend on no parameter):
//   mrl_ppo_grad    forward, loss head, back-propagation and the sums over samples.  Workgroup (g, net) is one wavefront
//                   and owns samples [g * share, (g + 1) * share) of the row for the critic (net 0) or the actor (net 1);
//                   it takes them 64 at a time, a lane per sample, weights in SGPRs as in mrl_policy_act, keeps its sums
//                   in registers over the whole share and writes ONE partial gradient vector.  dW2 = sum_s d2(s) h1(s)^T,
//                   the one 64 x 64 reduction across samples, runs on v_mfma_f32_32x32x2_f32 with k = samples: the
//                   activations go through LDS as [unit][sample], which is the transpose the instruction wants.
//   mrl_grad_reduce adds the partial vectors in ascending workgroup order and forms per-block sums of g^2.
//   mrl_clip_adam   total norm, clip, Adam and the stats row (adam_step.hpp: the tail every update shares; the whole
//                   parameter array is one segment).
// No float atomics and no wait on another workgroup anywhere: the same inputs give the same bits on every run.
//
// Arithmetic: every dot product and every sum that is not on the MFMA is fmaf or a plain add in a fixed order (the
// Makefile compiles with -ffp-contract=off); the MFMA is itself a k-ordered fmaf chain; tanhf / expf / logf are the
// accurate library versions.
//
// This header holds the kernels and what the launches share on the host.  It is compiled into two objects: ppo_update.hip, the
// plain update, and ppo_update_bank.hip, the update of M members of a bank in the same launches.  A bank
// launch hands the kernels one more argument, PpoMemberStrides, and the member travels in blockIdx.z: the MEMBER... pack below is
// empty for the plain instances, which therefore have the arguments, and in their own object the instructions, they always had.
#pragma once

#include "ppo_update.hpp"

#include <cmath>

namespace mrl {

namespace {

constexpr int kH = (int)kPolicyHidden;
constexpr int kT = (int)kPpoTile;
constexpr int kLd = kT + 1;  // row stride of the [unit][sample] images: a column and a row both spread over all banks
constexpr int kMaxD = 7, kMaxOut = 4;  // the balance beam's shape
constexpr int kMeanThreads = 1024;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct PpoGradArgs {
    const float *params;
    const float *obs;
    const int32_t *actions;
    const float *logprobs, *advantages, *returns, *values;
    const int32_t *indices;  // this row's B sample numbers
    const float *mean_std;   // this row's (mean, std + 1e-8), nullptr without MRL_PPO_NORM_ADV
    float *partial_grads;    // (groups, P)
    double *partial_stats;   // (groups, 8)
    uint64_t share;
    uint32_t minibatch_size;
    uint32_t num_params;
    float clip_coef, ent_coef, vf_coef;
    uint32_t flags;
};

// A bank launch's second argument -- floats (int32 for the indices) from a member's arrays to the next member's: its parameter row
// (P), its R rows of the index array (R B) and its workspace slice (mean_std, partial_grads, partial_stats; a whole number of
// 16-byte units, so partial_stats' doubles lie half as many doubles apart).
struct PpoMemberStrides {
    uint64_t params, indices, scratch;
};

// member blockIdx.z's array behind the first member's -- or, without the strides, the array itself
template <typename T>
__device__ __forceinline__ T *own(T *first, uint64_t)
{
    return first;
}
template <typename T>
__device__ __forceinline__ T *own(T *first, uint64_t stride, const PpoMemberStrides &)
{
    return first + (size_t)blockIdx.z * stride;
}
__device__ __forceinline__ uint64_t stride_of(uint64_t PpoMemberStrides::*) { return 0; }
__device__ __forceinline__ uint64_t stride_of(uint64_t PpoMemberStrides::*field, const PpoMemberStrides &m) { return m.*field; }

// XD and XOUT size the two small images per instance: Cartpole's and Acrobot's three instances share (6, 3), as before the beam
// brought (7, 4), so their LDS offsets, and with them their instruction streams, are what they were.
template <int XD, int XOUT>
struct PpoLds {
    static_assert(XD <= kMaxD && XOUT <= kMaxOut, "a shape beyond the largest one launch_ppo_update dispatches on");
    alignas(16) float h1[kH * kLd];  // first hidden layer, [unit][sample]; at the end the lanes' stat sums (as double)
    float h2[kH * kLd];  // second hidden layer; later d1 = dL/d(pre-activation of layer 1)
    float d2[kH * kLd];  // dL/d(pre-activation of layer 2)
    float x[XD * kT];
    float d3[XOUT * kT];  // dL/d(output)
};

// What a lane adds up over its samples for the stats row: the actor uses 0 pg, 2 entropy, 3 -logratio, 4 (ratio - 1) -
// logratio, 5 clipped or not; the critic 1, the max of the two squared errors.  The terms are float32; their sums are kept
// in double, so that a stat is its float32 terms' mean rounded once (a float32 sum over B terms would add its own error to
// a number the tests compare with another float32 computation's).
struct PpoHead {
    double stat[6];
};

// lines 275-292 and 309 for one sample: d3 = dLoss/dlogits
template <int A, typename... MEMBER>
__device__ __forceinline__ void actor_head(const PpoGradArgs &a, uint32_t at, const float (&l)[A], float (&d3)[A], PpoHead &s,
                                           const MEMBER &...member)
{
    const float count = (float)a.minibatch_size;
    // categorical_sample's soft-max (random_policy.hpp), all A log-probs kept, the log of the sum in double (below)
    float top = l[0];
#pragma unroll
    for (int i = 1; i < A; i++) top = fmaxf(top, l[i]);
    float e[A], sum = 0.0f;
#pragma unroll
    for (int i = 0; i < A; i++) {
        e[i] = expf(l[i] - top);
        sum += e[i];
    }
    // log of the float32 sum through the double-precision log, rounded once: logf is within an ulp but leans one way near
    // sum = 3 (three near-uniform actions), and a lean of a tenth of an ulp in every sample's logp does not average out of
    // old_approx_kl = mean(old - logp), which is a hundred times smaller than logp itself
    const float logsum = (float)log((double)sum);
    const int action = a.actions[at];
    float logp[A], prob[A], entropy = 0.0f, newlogprob = 0.0f;
#pragma unroll
    for (int i = 0; i < A; i++) {
        logp[i] = (l[i] - top) - logsum;
        prob[i] = e[i] / sum;
        entropy = fmaf(-prob[i], logp[i], entropy);
        newlogprob = action == i ? logp[i] : newlogprob;
    }
    const float logratio = newlogprob - a.logprobs[at];
    const float ratio = expf(logratio);
    float adv = a.advantages[at];
    if (a.mean_std) {
        const float *mean_std = own(a.mean_std, stride_of(&PpoMemberStrides::scratch, member...), member...);
        adv = (adv - mean_std[0]) / mean_std[1];
    }
    const float lo = 1.0f - a.clip_coef, hi = 1.0f + a.clip_coef;
    const float pg1 = -adv * ratio, pg2 = -adv * fminf(fmaxf(ratio, lo), hi);
    // torch.max hands the gradient to the larger argument and halves it on a tie; clamp passes it inside [lo, hi]
    const float first = pg1 > pg2 ? 1.0f : (pg1 == pg2 ? 0.5f : 0.0f);
    const float through = first + (ratio >= lo && ratio <= hi ? 1.0f - first : 0.0f);
    const float g_logprob = (-adv * through) * ratio / count;
    const float g_entropy = a.ent_coef / count;  // of -ent_coef * mean(H): dH/dl_i = -p_i (logp_i + H)
#pragma unroll
    for (int i = 0; i < A; i++)
        d3[i] = fmaf(g_logprob, (action == i ? 1.0f : 0.0f) - prob[i], g_entropy * (prob[i] * (logp[i] + entropy)));
    s.stat[0] += (double)fmaxf(pg1, pg2);
    s.stat[2] += (double)entropy;
    s.stat[3] += (double)-logratio;
    s.stat[4] += (double)((ratio - 1.0f) - logratio);
    s.stat[5] += fabsf(ratio - 1.0f) > a.clip_coef ? 1.0 : 0.0;
}

// lines 295-307 for one sample: d3 = dLoss/dvalue
__device__ __forceinline__ void critic_head(const PpoGradArgs &a, uint32_t at, const float (&out)[1], float (&d3)[1], PpoHead &s)
{
    const float count = (float)a.minibatch_size;
    const float v = out[0], ret = a.returns[at];
    const float err = v - ret, plain = err * err;
    float worst = plain, g = 2.0f * err;
    if (a.flags & MRL_PPO_CLIP_VLOSS) {
        const float old = a.values[at], moved = v - old;
        const float err_c = (old + fminf(fmaxf(moved, -a.clip_coef), a.clip_coef)) - ret, clipped = err_c * err_c;
        const float first = plain > clipped ? 1.0f : (plain == clipped ? 0.5f : 0.0f);
        const bool inside = moved >= -a.clip_coef && moved <= a.clip_coef;
        worst = fmaxf(plain, clipped);
        g = first * (2.0f * err) + (inside ? (1.0f - first) * (2.0f * err_c) : 0.0f);
    }
    d3[0] = (a.vf_coef * 0.5f) * g / count;
    s.stat[1] += (double)worst;
}

// One net over this workgroup's share.  p: the net's parameters; gout: its part of this workgroup's partial vector.
template <int D, int OUT, bool ACTOR, class Lds, typename... MEMBER>
__device__ __forceinline__ void ppo_grad_net(const PpoGradArgs &a, const float *__restrict__ p, float *__restrict__ gout,
                                             double *__restrict__ sout, Lds &lds, const MEMBER &...member)
{
    const float *__restrict__ w1 = p, *__restrict__ b1 = w1 + kH * D;
    const float *__restrict__ w2 = b1 + kH, *__restrict__ b2 = w2 + kH * kH;
    const float *__restrict__ w3 = b2 + kH, *__restrict__ b3 = w3 + OUT * kH;
    const int lane = threadIdx.x, r = lane & 31, half = lane >> 5;
    const uint64_t begin = blockIdx.x * a.share;
    const uint64_t end = begin + a.share < a.minibatch_size ? begin + a.share : a.minibatch_size;

    f32x16 acc[2][2];  // dW2, rows 32 jt .. + 31 (the unit of layer 2), columns 32 it .. + 31 (the unit of layer 1)
#pragma unroll
    for (int jt = 0; jt < 2; jt++)
#pragma unroll
        for (int it = 0; it < 2; it++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[jt][it][e] = 0.0f;
    float gw1[D], gw3[OUT], gb3[OUT], gb1 = 0.0f, gb2 = 0.0f;  // with the lane as the unit
#pragma unroll
    for (int d = 0; d < D; d++) gw1[d] = 0.0f;
#pragma unroll
    for (int o = 0; o < OUT; o++) gw3[o] = gb3[o] = 0.0f;
    PpoHead head;
#pragma unroll
    for (int c = 0; c < 6; c++) head.stat[c] = 0.0;

    for (uint64_t base = begin; base < end; base += kT) {
        // ---- a lane per sample.  A lane past the end runs on zeros and contributes d3 = 0, hence +0 to every sum.
        const bool live = base + lane < end;
        const uint32_t at = live ? (uint32_t)own(a.indices, stride_of(&PpoMemberStrides::indices, member...), member...)[base + lane] : 0u;
        float x[D];
#pragma unroll
        for (int d = 0; d < D; d++) x[d] = 0.0f;
        if (live) {
            if (D % 2) {  // an odd row length: rows lie D * 4 bytes apart, so only a dword is aligned
                const float *__restrict__ row = a.obs + (size_t)at * D;
#pragma unroll
                for (int d = 0; d < D; d++) x[d] = row[d];
            } else if (D == 4) {
                const float4 o = reinterpret_cast<const float4 *>(a.obs)[at];
                x[0] = o.x, x[1] = o.y, x[2] = o.z, x[3] = o.w;
            } else {
                const float2 *row = reinterpret_cast<const float2 *>(a.obs) + (size_t)at * (D / 2);
#pragma unroll
                for (int d = 0; d < D / 2; d++) {
                    const float2 o = row[d];
                    x[2 * d] = o.x, x[2 * d + 1] = o.y;
                }
            }
        }
#pragma unroll
        for (int d = 0; d < D; d++) lds.x[d * kT + lane] = x[d];
        float out[OUT];
        {
            // one tanhf in the code instead of 64: layer 1 goes to LDS unit by unit and comes back as the register array
#pragma unroll 1
            for (int j = 0; j < kH; j++) {
                float sum = b1[j];
#pragma unroll
                for (int i = 0; i < D; i++) sum = fmaf(w1[j * D + i], x[i], sum);
                lds.h1[j * kLd + lane] = tanhf(sum);
            }
            float h1[kH];
#pragma unroll
            for (int i = 0; i < kH; i++) h1[i] = lds.h1[i * kLd + lane];  // (this lane's own stores)
#pragma unroll
            for (int o = 0; o < OUT; o++) out[o] = b3[o];
#pragma unroll 1
            for (int j = 0; j < kH; j++) {
                float sum = b2[j];
#pragma unroll
                for (int i = 0; i < kH; i++) sum = fmaf(w2[j * kH + i], h1[i], sum);
                const float h2 = tanhf(sum);
                lds.h2[j * kLd + lane] = h2;
#pragma unroll
                for (int o = 0; o < OUT; o++) out[o] = fmaf(w3[o * kH + j], h2, out[o]);
            }
        }
        float d3[OUT];
#pragma unroll
        for (int o = 0; o < OUT; o++) d3[o] = 0.0f;
        if (live) {
            if constexpr (ACTOR) actor_head<OUT>(a, at, out, d3, head, member...);
            else critic_head(a, at, out, d3, head);
        }
#pragma unroll
        for (int o = 0; o < OUT; o++) lds.d3[o * kT + lane] = d3[o];
        float d1[kH];  // sum_j w2[j][i] d2[j]
#pragma unroll
        for (int i = 0; i < kH; i++) d1[i] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < kH; j++) {
            float back = 0.0f;
#pragma unroll
            for (int o = 0; o < OUT; o++) back = fmaf(w3[o * kH + j], d3[o], back);
            const float h2 = lds.h2[j * kLd + lane];  // (this lane's own store)
            const float d2 = back * (1.0f - h2 * h2);
            lds.d2[j * kLd + lane] = d2;
#pragma unroll
            for (int i = 0; i < kH; i++) d1[i] = fmaf(w2[j * kH + i], d2, d1[i]);
        }
        __syncthreads();
        // ---- a lane per unit of layer 2: dW3, db3, db2, samples in ascending order
#pragma unroll 8
        for (int s = 0; s < kT; s++) {
            const float h2 = lds.h2[lane * kLd + s];
#pragma unroll
            for (int o = 0; o < OUT; o++) {
                const float d = lds.d3[o * kT + s];
                gw3[o] = fmaf(d, h2, gw3[o]);
                gb3[o] += d;
            }
            gb2 += lds.d2[lane * kLd + s];
        }
        __syncthreads();
        // ---- back to a lane per sample: d1 takes h2's place
#pragma unroll
        for (int i = 0; i < kH; i++) {
            const float h1 = lds.h1[i * kLd + lane];
            lds.h2[i * kLd + lane] = d1[i] * (1.0f - h1 * h1);
        }
        __syncthreads();
        // ---- a lane per unit of layer 1: dW1, db1
#pragma unroll 8
        for (int s = 0; s < kT; s++) {
            const float d = lds.h2[lane * kLd + s];
#pragma unroll
            for (int i = 0; i < D; i++) gw1[i] = fmaf(d, lds.x[i * kT + s], gw1[i]);
            gb1 += d;
        }
        // ---- dW2 on the matrix core: A[row = unit of layer 2][k = sample] = d2, B[k = sample][col = unit of layer 1] = h1.
        // Lane (r, half) feeds row / column r and k = half; k-step kk pairs sample kk with sample kk + 32, so the two
        // halves of the wavefront read different banks.
#pragma unroll 4
        for (int kk = 0; kk < kT / 2; kk++) {
            const int s = kk + 32 * half;
            const float a0 = lds.d2[r * kLd + s], a1 = lds.d2[(32 + r) * kLd + s];
            const float h0 = lds.h1[r * kLd + s], h1 = lds.h1[(32 + r) * kLd + s];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, h0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, h1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, h0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, h1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();  // the next tile overwrites what the loops above read
    }

    // ---- one partial vector, in parameter order: W1 (64, D), b1, W2 (64, 64), b2, W3 (OUT, 64), b3
#pragma unroll
    for (int d = 0; d < D; d++) gout[lane * D + d] = gw1[d];
    gout[kH * D + lane] = gb1;
    float *__restrict__ gw2 = gout + kH * D + kH;
#pragma unroll
    for (int jt = 0; jt < 2; jt++)
#pragma unroll
        for (int it = 0; it < 2; it++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int row = 32 * jt + (e & 3) + 8 * (e >> 2) + 4 * half;  // C/D map of the 32 x 32 tile
                gw2[row * kH + 32 * it + r] = acc[jt][it][e];
            }
    gw2[kH * kH + lane] = gb2;
    float *__restrict__ gw3out = gw2 + kH * kH + kH;
#pragma unroll
    for (int o = 0; o < OUT; o++) gw3out[o * kH + lane] = gw3[o];
    if (lane == 0) {
#pragma unroll
        for (int o = 0; o < OUT; o++) gw3out[OUT * kH + o] = gb3[o];
    }
    // ---- the stats' sums: lanes in ascending order
    double *sums = reinterpret_cast<double *>(lds.h1);
#pragma unroll
    for (int c = 0; c < 6; c++) sums[c * kT + lane] = head.stat[c];
    __syncthreads();
    if (lane < 6 && (ACTOR ? lane != 1 : lane == 1)) {
        double sum = 0.0;
        for (int s = 0; s < kT; s++) sum += sums[lane * kT + s];
        sout[lane] = sum;
    }
}

// MEMBER: nothing, or the PpoMemberStrides of a bank update -- then workgroup (g, net, z) works for member z on its own parameter
// row, index rows and workspace slice, and on everyone's batch arrays
template <int D, int A, typename... MEMBER>
__global__ void __launch_bounds__(kT) mrl_ppo_grad(PpoGradArgs a, MEMBER... member)
{
    static_assert(sizeof...(MEMBER) <= 1, "at most the member strides");
    __shared__ PpoLds<(D > 6 ? D : 6), (A > 3 ? A : 3)> lds;
    const float *params = own(a.params, stride_of(&PpoMemberStrides::params, member...), member...);
    float *gout = own(a.partial_grads, stride_of(&PpoMemberStrides::scratch, member...), member...) + (size_t)blockIdx.x * a.num_params;
    double *sout = own(a.partial_stats, stride_of(&PpoMemberStrides::scratch, member...) / 2, member...) + (size_t)blockIdx.x * kPpoStats;
    if (blockIdx.y == 0) ppo_grad_net<D, 1, false>(a, params, gout, sout, lds, member...);
    else ppo_grad_net<D, A, true>(a, params + mlp_net_params(D, kH, 1), gout + mlp_net_params(D, kH, 1), sout, lds, member...);
}

// line 287's mean and std (torch's unbiased one) of every row's advantages, one workgroup per row.  With the strides workgroup
// (k, 0, z) serves row k of member z: its index rows lie behind those of the members before it, its result in its own slice.
template <typename... MEMBER>
__global__ void __launch_bounds__(kMeanThreads) mrl_ppo_mean_std(const float *__restrict__ advantages, const int32_t *__restrict__ indices,
                                                                uint32_t minibatch_size, float *__restrict__ mean_std, MEMBER... member)
{
    static_assert(sizeof...(MEMBER) <= 1, "at most the member strides");
    __shared__ float scratch[kMeanThreads];
    indices = own(indices, stride_of(&PpoMemberStrides::indices, member...), member...);
    mean_std = own(mean_std, stride_of(&PpoMemberStrides::scratch, member...), member...);
    const int32_t *row = indices + (size_t)blockIdx.x * minibatch_size;
    float sum = 0.0f;
    for (uint32_t b = threadIdx.x; b < minibatch_size; b += kMeanThreads) sum += advantages[(uint32_t)row[b]];
    const float mean = block_sum<kMeanThreads>(sum, scratch) / (float)minibatch_size;
    float squares = 0.0f;
    for (uint32_t b = threadIdx.x; b < minibatch_size; b += kMeanThreads) {
        const float d = advantages[(uint32_t)row[b]] - mean;
        squares = fmaf(d, d, squares);
    }
    const float var = block_sum<kMeanThreads>(squares, scratch) / (float)(minibatch_size - 1u);
    if (threadIdx.x == 0) {
        mean_std[2 * blockIdx.x] = mean;
        mean_std[2 * blockIdx.x + 1] = sqrtf(var) + 1e-8f;
    }
}

// The stats row's end, in mrl_clip_adam: eight columns from the workgroups' six sums and the total norm
struct PpoStatsRow {
    const double *partial_stats;
    float *row;  // nullptr: no stats
    uint32_t groups, minibatch_size;
    float ent_coef, vf_coef;

    __device__ void operator()(uint32_t, float total_norm) const
    {
        if (row) fill(partial_stats, row, total_norm);
    }

    __device__ void fill(const double *partial_stats, float *row, float total_norm) const
    {
        double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t w = 0; w < groups; w++)
            for (int c = 0; c < 6; c++) sum[c] += partial_stats[(size_t)w * kPpoStats + c];
        const double count = (double)minibatch_size;
        const double pg = sum[0] / count, v_loss = 0.5 * (sum[1] / count), entropy = sum[2] / count;
        row[0] = (float)pg;
        row[1] = (float)v_loss;
        row[2] = (float)entropy;
        row[3] = (float)(sum[3] / count);
        row[4] = (float)(sum[4] / count);
        row[5] = (float)(sum[5] / count);
        row[6] = total_norm;
        row[7] = (float)(pg - (double)ent_coef * entropy + v_loss * (double)vf_coef);
    }
};

// the same for the members of a bank update: member blockIdx.z's sums from its own slice, into its own (R, 8) block of the stats
struct PpoMemberStatsRow {
    PpoStatsRow first;           // member 0's
    uint64_t member_stats_sums;  // doubles from a member's partial_stats to the next member's
    uint64_t member_rows;        // floats from a member's stats rows to the next member's: 8 R

    __device__ void operator()(uint32_t, float total_norm) const
    {
        if (first.row)
            first.fill(first.partial_stats + (size_t)blockIdx.z * member_stats_sums, first.row + (size_t)blockIdx.z * member_rows, total_norm);
    }
};

// What both launchers set up alike from validated arguments: the gradient kernel's and the tail's arguments, without what changes
// from row to row
struct PpoLaunch {
    uint32_t D, A, P;
    SampleShare share;
    PpoWorkspace ws;
    bool norm;
    PpoGradArgs g;
    AdamStepArgs ad;
    PpoStatsRow row;
};

inline PpoLaunch ppo_launch(const mrl_mlp_policy &shape, const mrl_ppo_optimizer &opt, const mrl_ppo_batch &batch, uint32_t num_minibatches,
                            uint32_t minibatch_size, const mrl_ppo_config &cfg, float *workspace)
{
    PpoLaunch l{};
    const uint32_t D = l.D = shape.obs_dim, A = l.A = shape.num_actions;
    const uint32_t P = l.P = (uint32_t)(mlp_net_params(D, kH, 1) + mlp_net_params(D, kH, A));
    const SampleShare share = l.share = share_samples(minibatch_size, kPpoTile, kPpoMaxGroups);
    const PpoWorkspace ws = l.ws = ppo_workspace(P, minibatch_size, num_minibatches);
    l.norm = cfg.flags & MRL_PPO_NORM_ADV;
    PpoGradArgs &g = l.g;
    g.params = opt.params_dev;
    g.obs = batch.obs;
    g.actions = batch.actions;
    g.logprobs = batch.logprobs;
    g.advantages = batch.advantages;
    g.returns = batch.returns;
    g.values = batch.values;
    g.partial_grads = workspace + ws.partial_grads;
    g.partial_stats = reinterpret_cast<double *>(workspace + ws.partial_stats);
    g.share = share.share;
    g.minibatch_size = minibatch_size;
    g.num_params = P;
    g.clip_coef = cfg.clip_coef;
    g.ent_coef = cfg.ent_coef;
    g.vf_coef = cfg.vf_coef;
    g.flags = cfg.flags;
    // clip_grad_norm_ (line 314) and torch.optim.Adam (line 315) over the whole parameter array
    AdamStepArgs &ad = l.ad = adam_step_args(cfg.beta1, cfg.beta2, cfg.eps, cfg.max_grad_norm > 0.0f, cfg.max_grad_norm);
    ad.partial_grads = g.partial_grads;
    ad.grad = workspace + ws.grad;
    ad.sumsq = workspace + ws.sumsq;
    ad.params = opt.params_dev;
    ad.exp_avg = opt.exp_avg;
    ad.exp_avg_sq = opt.exp_avg_sq;
    ad.stride = P;
    ad.segments = 1;
    ad.groups = share.groups;
    ad.blocks = (P + kAdamThreads - 1) / kAdamThreads;
    ad.num_params[0] = P;
    l.row = PpoStatsRow{g.partial_stats, nullptr, share.groups, minibatch_size, cfg.ent_coef, cfg.vf_coef};
    return l;
}

// one row's gradient launch; `member`: nothing, or a bank update's strides
template <typename... MEMBER>
inline void launch_ppo_grad(uint32_t D, uint32_t A, const dim3 &grid, const PpoGradArgs &g, hipStream_t stream, const MEMBER &...member)
{
    if (D == 7)
        hipLaunchKernelGGL((mrl_ppo_grad<7, 4, MEMBER...>), grid, dim3(kT), 0, stream, g, member...);
    else if (D == 6)
        hipLaunchKernelGGL((mrl_ppo_grad<6, 3, MEMBER...>), grid, dim3(kT), 0, stream, g, member...);
    else if (A == 3)
        hipLaunchKernelGGL((mrl_ppo_grad<4, 3, MEMBER...>), grid, dim3(kT), 0, stream, g, member...);
    else
        hipLaunchKernelGGL((mrl_ppo_grad<4, 2, MEMBER...>), grid, dim3(kT), 0, stream, g, member...);
    MRL_HIP(hipGetLastError());
}

}  // namespace

}  // namespace mrl
