// mrl_mlpbase_act_h512: both nets of MAPPO's MLPBase actor-critic at hidden_size 512 for the balance beam (train/MAPPO/utils/
// mlp.py with the trainer's default width, train/config.py:200) and the head, ONE launch per act (include/mrl_envs.h; DESIGN.md
// section 32; the network, the flat tensor, the order of every sum and the LDS image are in mlpbase_h512.hpp).
//
// A workgroup of four wavefronts runs one net for a tile of 32 RB samples (sample = world n, seat p of the `players` mask, in
// that order; RB = 1 or 2 row blocks of 32); blockIdx.y chooses the net.  The net is 1 + layer_N products of 512 x 512 (fc1: 8 x
// 512) and almost nothing else, so what decides the time is how often a weight is fetched:
//   weights     are read from L2 straight into the matrix instruction's B operand, never through LDS (1 MB a layer; a workgroup has
//               160 KiB).  Wave w owns the column blocks 4 w .. 4 w + 3 of 32 columns; lane (r, half) owns column r of each, i.e.
//               one row of torch's weight, and loads 8 consecutive k of it as two 16-byte loads (h512_fetch of cnn_h512_forward.hpp:
//               rows start on 4-byte boundaries only).  half 0 feeds the even k, half 1 the odd ones.  The fetch of the next 8 k
//               is issued before the products of the current 8.
//   row blocks  ONE such fetch serves every row block of the tile: 4 RB matrix instructions per column block.  With RB = 2 a
//               weight byte is used 64 times instead of 32 and the L2 traffic per sample halves; the price is 128 accumulator
//               registers a lane instead of 64 and half as many workgroups.  launch_mlpbase_act_h512 takes RB = 2 from
//               kMlpH512WideFrom samples on, where 32-row tiles alone would queue on every CU several times over.
//   h           RB x 32 rows of 513 floats in LDS.  A layer's sums wait in registers until every wave has read the previous h,
//               then relu(sum + bias) replaces it, and LayerNorm(512) runs in place, a wavefront per row, a lane eight columns
//               64 apart (no bank conflict), the row's two sums by mlpbase_h512.hpp's order.
//   fc1         K = 7: the A operand is LayerNorm(7)'s output in LDS (rows of 9, column 7 zero), B four scalar loads a lane;
//               four matrix instructions per block, the last k a zero product.
//   head        wave rb runs row block rb: one column block whose columns out_dim .. 31 read row 0 again and are not stored;
//               then act_tail (act_record.hpp), a sample per lane, ends the act exactly as mrl_mlpbase_act's.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "mlpbase_h512_forward.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char mlpbase_h512_lds_image[];

template <int RB>
__global__ void __launch_bounds__(kMlpH512Threads) mrl_mlpbase_act_h512(MlpBaseActArgs a)
{
    constexpr uint32_t kRows = 32u * RB;
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const bool odd = half != 0u;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = a.params + (net ? mlpbase_h512_net_params(a.layer_N, kMlpBaseActions) : 0u);
    float *h = reinterpret_cast<float *>(mlpbase_h512_lds_image);
    float *in0 = h + mlpbase_h512_in0_at(kRows), *outs = h + mlpbase_h512_out_at(kRows);
    // tile t of the call holds samples kRows t .. kRows t + kRows - 1 of the `players` mask
    const uint32_t tile0 = blockIdx.x * kRows, total = a.num_worlds * a.num_seats;

    {
        // the tile's observation rows: thread (row, k), k < 8; a row past the end is zeros, column 7 LayerNorm(7) sets
        const bool copies = a.obs_row && net == (a.nets == 2u ? 1u : 0u);
        const uint32_t k = tid & 7u;
        for (uint32_t rr = tid >> 3; rr < kRows; rr += kMlpH512Threads / 8u) {
            float v = 0.0f;
            if (tile0 + rr < total && k < kMlpBaseObs) {
                uint32_t world, seat;
                seat_sample(a.players, a.num_seats, tile0 + rr, world, seat);
                const int32_t word = a.obs[((size_t)seat * a.num_worlds + world) * kMlpBaseObs + k];
                v = (float)word;
                if (copies) a.obs_row[((size_t)world * a.P + seat) * kMlpBaseObs + k] = word;
            }
            in0[rr * kMlpLd0 + k] = v;
        }
    }
    __syncthreads();
    mlp512_layer_norm<1>(in0, kMlpLd0, kRows, kMlpBaseObs, params, params + kMlpBaseObs, wave, lane);

    f32x16 acc[RB][4];
    const float *a_row = h + r * kMlpH512Ld + half;
    for (uint32_t layer = 0; layer <= a.layer_N; layer++) {
        const float *__restrict__ w = params + mlpbase_h512_layer_at(layer);
        const float *__restrict__ bias = w + kMlpH512Hidden * (layer ? kMlpH512Hidden : kMlpBaseObs);
        if (layer == 0) {
            mlp512_fc1<RB>(in0, w, wave, r, half, acc);  // (nothing has read h yet: no barrier before the store)
        } else {
            const float *w_row[4];
#pragma unroll
            for (int j = 0; j < 4; j++) w_row[j] = w + (size_t)((wave * 4u + j) * 32u + r) * kMlpH512Hidden;
            mlp512_products<RB>(a_row, w_row, odd, acc);
            __syncthreads();  // every wave has read the previous h: this layer's replaces it
        }
        mlp512_store<RB>(acc, bias, h, wave, r, half);
        __syncthreads();
        mlp512_layer_norm<8>(h, kMlpH512Ld, kRows, kMlpH512Hidden, bias + kMlpH512Hidden, bias + 2u * kMlpH512Hidden, wave, lane);
    }

    if (wave < (uint32_t)RB) {
        // the head of row block `wave`: one column block, columns out_dim .. 31 read row 0 again and are not stored
        const float *__restrict__ head_w = params + mlpbase_h512_head_at(a.layer_N), *__restrict__ head_b = head_w + out_dim * kMlpH512Hidden;
        f32x16 out[1];
        const float *head_row[1] = {head_w + (size_t)(r < out_dim ? r : 0u) * kMlpH512Hidden};
#pragma unroll
        for (int e = 0; e < 16; e++) out[0][e] = 0.0f;
        h512_products<1>(a_row + wave * 32u * kMlpH512Ld, kMlpH512Hidden, head_row, odd, out);
        if (r < out_dim) {
            const float bias = head_b[r];
#pragma unroll
            for (int e = 0; e < 16; e++) outs[(wave * 32u + (e & 3) + 8 * (e >> 2) + 4 * half) * 8u + r] = out[0][e] + bias;
        }
    }
    __syncthreads();

    if (tid >= kRows || tile0 + tid >= total) return;
    uint32_t world, seat;
    seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
    act_tail<(int)kMlpBaseActions>(a, outs, net, tid, world, seat, a.reward);
}

template <int RB>
static void launch_rows(const MlpBaseActArgs &args, uint32_t total, hipStream_t stream)
{
    constexpr uint32_t rows = 32u * RB, bytes = mlpbase_h512_lds_floats(rows) * 4u;
    allow_large_dynamic_lds<&mrl_mlpbase_act_h512<RB>>(bytes);
    const dim3 grid((total + rows - 1) / rows, args.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_mlpbase_act_h512<RB>, grid, dim3(kMlpH512Threads), bytes, stream, args);
    MRL_HIP(hipGetLastError());
}

void launch_mlpbase_act_h512(const MlpBaseActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.num_worlds * args.num_seats;
    if (total == 0 || args.nets == 0) return;
    if (total >= kMlpH512WideFrom)
        launch_rows<2>(args, (uint32_t)total, stream);
    else
        launch_rows<1>(args, (uint32_t)total, stream);
}

}  // namespace mrl
