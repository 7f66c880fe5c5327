// mrl_cnn_act_h512: both nets of MAPPO's CNN actor-critic at hidden_size 512 (train/MAPPO/utils/cnn.py:26-42 with the trainer's
// default, train/config.py:200) and the head, ONE launch per act (include/mrl_envs.h; the sums' order and
// the LDS image are in cnn_h512.hpp, the index map in cnn_policy.hpp).
//
// As in mrl_cnn_act a workgroup of four wavefronts runs one net for a tile of 32 samples, blockIdx.y chooses the net, the tile's
// rows reach LDS once as the int8 the simulator wrote (cnn_load_tile) and every product is v_mfma_f32_32x32x2_f32.  What the
// width changes is how the work is split:
//   channel loop  the 256 conv channels run as 8 blocks of 32.  A block's conv weights (the plain act's 32 x 9 F floats) go to
//                 region A beside the rows, cnn_conv_tile writes the block's 32 npos activations to the plain act's image, and
//                 the image is multiplied straight into fc1: wave w owns the column blocks 4 w .. 4 w + 3 of 32 columns each,
//                 64 accumulator registers per lane for the block's own sum and 64 for the running sum of the block sums, which
//                 live across all 8 blocks.  The next block's conv weights are
//                 stored to LDS before the products, so a block costs two barriers.
//   B operands    fc1 (3 to 11 MB a net), fc2 (1 MB) and the head are read from L2 straight into registers: lane (r, half)
//                 owns column r of its block, i.e. one row of torch's weight, and loads 8 consecutive k of it as two 16-byte
//                 loads (rows start on 4-byte boundaries only: the loads are typed so); half 0 feeds the even k, half 1 the
//                 odd ones.  One such fetch serves four matrix instructions per column block, and the fetch of the next 8 k
//                 is issued before the products of the current 8.  During the channel loop LDS has no room for a staged
//                 chunk of 512 columns (asymmetric_advantages leaves 6 KB), and a row's 32 bytes are used whole by the lane
//                 that loaded them, so staging would add a store and a load per weight and two barriers per chunk.
//   fc2, head     h1 (32 x 513 floats) overlies the dead convolution operands; fc2's sums wait in registers until every wave
//                 has read h1 and then replace it (h2); the head is one column block on wave 0; act_tail ends the act.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "cnn_h512_forward.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_h512_lds_image[];

__global__ void __launch_bounds__(kCnnThreads) mrl_cnn_act_h512(CnnActArgs a)
{
    const uint32_t net = act_net(a);
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

    unsigned char *lds = cnn_h512_lds_image;
    // tile t of the call holds samples 32 t .. 32 t + 31 of the `players` mask
    const uint32_t tile0 = blockIdx.x * kCnnTile, total = a.num_worlds * a.num_seats;
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        if (tile0 + rr >= total) return nullptr;
        uint32_t world, seat;
        seat_sample(a.players, a.num_seats, tile0 + rr, world, seat);
        return reinterpret_cast<const uint8_t *>(a.obs) + ((size_t)world * a.P + seat) * S;
    };
    cnn_load_tile(a, lds, row_address, nullptr, conv_w, true);  // the rows, the patch offsets and block 0's conv weights
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
    const float *a_row = reinterpret_cast<const float *>(lds + l.act_at) + r * l.act_ld + half;
    float *conv_lds = reinterpret_cast<float *>(lds + l.conv_w_at);
    for (uint32_t b = 0; b < kCnnH512Blocks; b++) {
        cnn_conv_tile(a, lds, shift, conv_b + b * kCnnChannels, wave, r, half);
        __syncthreads();  // block b's activations are complete, its conv weights dead
        if (b + 1u < kCnnH512Blocks) {
            // the next block's conv weights; the zero behind an odd K stays where cnn_load_tile put it
            const float *__restrict__ next = conv_w + (size_t)(b + 1u) * kCnnChannels * k1;
            for (uint32_t e = tid; e < kCnnChannels * k1; e += kCnnThreads) {
                const uint32_t c = e / k1, k = e - c * k1;
                conv_lds[c * l.conv_ld + k] = next[e];
            }
        }
        // the block's own sum from 0, then one add per output into the running sum (cnn_h512.hpp says why)
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
        __syncthreads();  // the activations are read, the next conv weights in place
    }

    // everything of the convolution is dead: h1 lies over it
    float *h = reinterpret_cast<float *>(lds), *outs = reinterpret_cast<float *>(lds + kCnnTile * kCnnH512HLd * 4u);
    h512_store(acc, fc1_b, h, wave, r, half);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) {
        w_row[j] = fc2_w + (size_t)((wave * 4u + j) * 32u + r) * kCnnH512Hidden;
#pragma unroll
        for (int e = 0; e < 16; e++) acc[j][e] = 0.0f;
    }
    const float *h_row = h + r * kCnnH512HLd + half;
    h512_products<4>(h_row, kCnnH512Hidden, w_row, odd, acc);
    __syncthreads();  // every wave has read h1: h2 replaces it
    h512_store(acc, fc2_b, h, wave, r, half);
    __syncthreads();
    if (wave == 0) {
        // the head: one column block, columns out_dim .. 31 read row 0 again and are not stored
        f32x16 out[1];
        const float *head_row[1] = {head_w + (size_t)(r < out_dim ? r : 0u) * kCnnH512Hidden};
#pragma unroll
        for (int e = 0; e < 16; e++) out[0][e] = 0.0f;
        h512_products<1>(h_row, kCnnH512Hidden, head_row, odd, out);
        if (r < out_dim) {
            const float bias = head_b[r];
#pragma unroll
            for (int e = 0; e < 16; e++) outs[((e & 3) + 8 * (e >> 2) + 4 * half) * 8u + r] = out[0][e] + bias;
        }
    }
    __syncthreads();

    if (tid >= kCnnTile || tile0 + tid >= total) return;
    uint32_t world, seat;
    seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
    act_tail<(int)kCnnActions>(a, outs, net, tid, world, seat, a.reward);
}

void launch_cnn_act_h512(const CnnActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.num_worlds * args.num_seats;
    if (total == 0 || args.nets == 0) return;
    const uint32_t bytes = cnn_h512_lds(args.W, args.H, args.F).total;
    allow_large_dynamic_lds<&mrl_cnn_act_h512>(bytes);
    const dim3 grid((uint32_t)((total + kCnnTile - 1) / kCnnTile), args.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_cnn_act_h512, grid, dim3(kCnnThreads), bytes, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
