// mrl_cnn_act: both nets of MAPPO's CNN actor-critic for Overcooked (train/MAPPO/utils/cnn.py:26-42, r_actor_critic.py,
// utils/distributions.py:55-68 with hidden_size 64) and the head, ONE launch per act (include/mrl_envs.h; DESIGN.md section 15;
// the index map is in cnn_policy.hpp).
//
// A workgroup of four wavefronts runs one net for a tile of 32 samples (sample = world n, seat p of the `players` mask, in
// that order); blockIdx.y chooses the net, so the actor's and the critic's workgroups of a tile run side by side and each
// reads the tile's 32 observation rows once, as the int8 the simulator wrote, into LDS.  All products are
// v_mfma_f32_32x32x2_f32: lane (r, half) feeds A[sample r][k = 2 kk + half] and B[k][column r], an output is 0, then fmaf over
// k ascending, and the bias is added to the finished sum.
//   convolution   a GEMM per output position (ow, oh): 32 samples x 32 channels, K = 9 F in torch's order k = f 9 + i 3 + j.  A is
//                 the int8 at obs row + patch base + offset(k), converted on the way to the register; the offsets of k sit in a
//                 small LDS table.  B, the conv weights, is the same for every position: wave w takes positions w, w + 4, ...
//                 three at a time, so one B read feeds three independent accumulators.  relu(acc + bias) goes to the LDS
//                 activation image at torch's flattened index c npos + ow (H - 2) + oh.
//   fc1, fc2, head  64, 64 and 6 / 1 columns: wave s < slabs owns the 32-column slab s and the whole k chain of its outputs; all
//                 four waves stage the weights, 64 k at a time, from the flat parameter array through LDS (rows 65 floats apart:
//                 lane r reads bank r + k), the next chunk's global loads issued before the current chunk's products.
//   head          lanes 0..31 of wave 0, a sample each: six logits as scalars out of LDS, soft-max, draw, log-prob
//                 (mrl_policy_act's rule); the critic's workgroup writes the value, the reward and the done flag.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "cnn_policy.hpp"
#include "cnn_forward.hpp"
#include "random_policy.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_lds_image[];

// sample s of the call -> (world, seat): seat = the (s % num_seats)-th set bit of the mask
__device__ __forceinline__ void cnn_sample(const CnnActArgs &a, uint32_t s, uint32_t &world, uint32_t &seat)
{
    world = s / a.num_seats;
    uint32_t idx = s - world * a.num_seats, mask = a.players;
    for (; idx > 0; idx--) mask &= mask - 1u;
    seat = (uint32_t)__ffs((int)mask) - 1u;
}

__global__ void __launch_bounds__(kCnnThreads) mrl_cnn_act(CnnActArgs a)
{
    const uint32_t net = a.nets == 3u ? blockIdx.y : a.nets >> 1;  // 0 the actor, 1 the critic
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t total = a.num_worlds * a.num_seats, tile0 = blockIdx.x * kCnnTile;
    const uint32_t S = a.W * a.H * a.F, k1 = a.lds.k1, K2 = kCnnChannels * a.lds.npos, out_dim = net ? 1u : kCnnActions;
    const float *__restrict__ conv_w = a.params + (net ? cnn_net_params(a.W, a.H, a.F, kCnnActions) : 0);
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
        const uint32_t s = tile0 + rr;
        uint32_t *__restrict__ dst = obs_words + rr * (a.lds.obs_ld / 4u);
        if (s >= total) {
            for (uint32_t d = lane; d < (S + 3u) / 4u; d += 64u) dst[d] = 0u;
            continue;
        }
        uint32_t world, seat;
        cnn_sample(a, s, world, seat);
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
        uint32_t shift = 0;
        if (tile0 + r < total) {
            uint32_t world, seat;
            cnn_sample(a, tile0 + r, world, seat);
            shift = (uint32_t)((reinterpret_cast<uintptr_t>(a.obs) + ((size_t)world * a.P + seat) * S) & 3u);
        }
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

    if (tid >= kCnnTile || tile0 + tid >= total) return;
    uint32_t world, seat;
    cnn_sample(a, tile0 + tid, world, seat);
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

void launch_cnn_act(const CnnActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.num_worlds * args.num_seats;
    if (total == 0 || args.nets == 0) return;
    allow_large_dynamic_lds<&mrl_cnn_act>(args.lds.total);
    const dim3 grid((uint32_t)((total + kCnnTile - 1) / kCnnTile), args.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_cnn_act, grid, dim3(kCnnThreads), args.lds.total, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
