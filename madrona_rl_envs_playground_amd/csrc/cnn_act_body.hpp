// The body of mrl_cnn_act (cnn_policy.hip describes the workgroup, the operand maps and the LDS image), templated on the map
// from a tile's row to its sample so that two kernels share it: mrl_cnn_act, whose tile t holds samples 32 t .. 32 t + 31 of the
// `players` mask, and mrl_cnn_act_bank (cnn_bank.hip), whose tile holds up to 32 samples of ONE policy of a bank, listed by the
// plan.  A map offers
//     bool sample(const CnnActArgs &a, uint32_t row, uint32_t &world, uint32_t &seat) const     false: the tile has no such row
// and the caller hands in the parameter array the tile runs.  A sample's arithmetic reads its own LDS rows and the tile's common
// weights only, so which other samples share its tile cannot change a bit of its outputs.
#pragma once

#include "cnn_policy.hpp"
#include "cnn_forward.hpp"
#include "random_policy.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_lds_image[];

template <class Map>
__device__ __forceinline__ void cnn_act_body(const CnnActArgs &a, const Map &map, const float *__restrict__ params)
{
    const uint32_t net = a.nets == 3u ? blockIdx.y : a.nets >> 1;  // 0 the actor, 1 the critic
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t S = a.W * a.H * a.F, k1 = a.lds.k1, K2 = kCnnChannels * a.lds.npos, out_dim = net ? 1u : kCnnActions;
    const float *__restrict__ conv_w = params + (net ? cnn_net_params(a.W, a.H, a.F, kCnnActions) : 0);
    const float *__restrict__ conv_b = conv_w + (size_t)kCnnChannels * k1;
    const float *__restrict__ fc1_w = conv_b + kCnnChannels, *__restrict__ fc1_b = fc1_w + (size_t)kCnnHidden * K2;
    const float *__restrict__ fc2_w = fc1_b + kCnnHidden, *__restrict__ fc2_b = fc2_w + kCnnHidden * kCnnHidden;
    const float *__restrict__ head_w = fc2_b + kCnnHidden, *__restrict__ head_b = head_w + out_dim * kCnnHidden;

    unsigned char *lds = cnn_lds_image;
    uint32_t *obs_words = reinterpret_cast<uint32_t *>(lds);
    float *w_lds = reinterpret_cast<float *>(lds + a.lds.conv_w_at);
    uint16_t *koff = reinterpret_cast<uint16_t *>(lds + a.lds.koff_at);
    float *act = reinterpret_cast<float *>(lds + a.lds.act_at);

    // the tile's observation rows, whole dwords from the 4-byte boundary at or below the row's start: LDS row rr holds the
    // row's bytes from byte `shift` on.  The first and the last dword are put together from the row's own bytes only.
    for (uint32_t rr = wave; rr < kCnnTile; rr += 4u) {
        uint32_t *__restrict__ dst = obs_words + rr * (a.lds.obs_ld / 4u);
        uint32_t world, seat;
        if (!map.sample(a, rr, world, seat)) {
            for (uint32_t d = lane; d < (S + 3u) / 4u; d += 64u) dst[d] = 0u;
            continue;
        }
        const uint8_t *__restrict__ row = reinterpret_cast<const uint8_t *>(a.obs) + ((size_t)world * a.P + seat) * S;
        const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(row) & 3u), words = (shift + S + 3u) / 4u;
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
    // the conv weights, rows conv_ld floats apart, a zero behind an odd K; the patch offset of every k
    for (uint32_t e = tid; e < kCnnChannels * k1; e += kCnnThreads) {
        const uint32_t c = e / k1, k = e - c * k1;
        w_lds[c * a.lds.conv_ld + k] = conv_w[e];
    }
    if (k1 != a.lds.k1_padded && tid < kCnnChannels) w_lds[tid * a.lds.conv_ld + k1] = 0.0f;
    for (uint32_t k = tid; k < a.lds.k1_padded; k += kCnnThreads) {
        const uint32_t f = k / 9u, ij = k - 9u * f, i = ij / 3u, j = ij - 3u * i;
        koff[k] = k < k1 ? (uint16_t)((j * a.W + i) * a.F + f) : (uint16_t)0;
    }
    __syncthreads();

    {
        // this lane's sample row in LDS
        uint32_t shift = 0, world, seat;
        if (map.sample(a, r, world, seat)) shift = (uint32_t)((reinterpret_cast<uintptr_t>(a.obs) + ((size_t)world * a.P + seat) * S) & 3u);
        const int8_t *__restrict__ my_obs = reinterpret_cast<const int8_t *>(lds) + r * a.lds.obs_ld + shift;
        const float *__restrict__ my_w = w_lds + r * a.lds.conv_ld;
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
    __syncthreads();  // the activation image is complete; the convolution's operands are dead

    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt);
    float *h1 = reinterpret_cast<float *>(lds + kCnnH1At), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt);
    cnn_fc_layer(act, a.lds.act_ld, K2, fc1_w, fc1_b, kCnnHidden, true, chunk, h1, kCnnFcLd, wave, lane);
    cnn_fc_layer(h1, kCnnFcLd, kCnnHidden, fc2_w, fc2_b, kCnnHidden, true, chunk, h2, kCnnFcLd, wave, lane);
    cnn_fc_layer(h2, kCnnFcLd, kCnnHidden, head_w, head_b, out_dim, false, chunk, outs, 8u, wave, lane);

    uint32_t world, seat;
    if (tid >= kCnnTile || !map.sample(a, tid, world, seat)) return;
    const size_t cell = (size_t)world * a.P + seat, agent = (size_t)seat * a.num_worlds + world;
    if (net) {
        if (a.values_row) a.values_row[cell] = outs[tid * 8u];
        if (a.dones_row) a.dones_row[cell] = a.done[world] != 0 ? 1.0f : 0.0f;
        if (a.rewards_row) a.rewards_row[cell] = (float)a.reward[agent];
        return;
    }
    const float l0 = outs[tid * 8u], l1 = outs[tid * 8u + 1], l2 = outs[tid * 8u + 2], l3 = outs[tid * 8u + 3], l4 = outs[tid * 8u + 4],
                l5 = outs[tid * 8u + 5];
    const float l[kCnnActions] = {l0, l1, l2, l3, l4, l5};  // statically indexed below: stays in registers
    int action;
    float logprob;
    categorical_sample<(int)kCnnActions>(l, policy_hash(a.seed, a.step, world, seat), a.flags & MRL_POLICY_GREEDY, action, logprob);
    a.action[agent] = action;
    if (a.actions_row) a.actions_row[cell] = action;
    if (a.logprobs_row) a.logprobs_row[cell] = logprob;
    if (a.logits_row) {
#pragma unroll
        for (int i = 0; i < (int)kCnnActions; i++) a.logits_row[cell * kCnnActions + i] = l[i];
    }
}

}  // namespace mrl
