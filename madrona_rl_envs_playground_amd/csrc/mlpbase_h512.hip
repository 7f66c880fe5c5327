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
#include "cnn_h512_forward.hpp"
#include "mlpbase_forward.hpp"
#include "mlpbase_h512.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char mlpbase_h512_lds_image[];

// the products of 8 consecutive k, from k on: four matrix instructions per (column block, row block), k ascending.  a_row: this
// lane's LDS row of row block 0 from its own first k (row r, k = half); row block rb lies 32 rows of `ld` floats further.
template <int RB>
__device__ __forceinline__ void mlp512_multiply(const float *__restrict__ a_row, uint32_t ld, uint32_t k, const f32x4u (&b)[4][2], bool odd,
                                                f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        float av[RB];
#pragma unroll
        for (int rb = 0; rb < RB; rb++) av[rb] = a_row[rb * 32u * ld + k + 2u * s];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float bv = odd ? b[j][s >> 1][2 * (s & 1) + 1] : b[j][s >> 1][2 * (s & 1)];
#pragma unroll
            for (int rb = 0; rb < RB; rb++) acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[rb], bv, acc[rb][j], 0, 0, 0);
        }
    }
}

// acc[rb][j][row][column r of block j] = sum over k < 512 of h[32 rb + row][k] * w_row[j][k], one chain from 0, k ascending
template <int RB>
__device__ __forceinline__ void mlp512_products(const float *__restrict__ a_row, const float *const (&w_row)[4], bool odd, f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int rb = 0; rb < RB; rb++)
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[rb][j][e] = 0.0f;
    f32x4u b0[4][2], b1[4][2];
    h512_fetch<4>(w_row, 0u, b0);
    for (uint32_t k = 0; k < kMlpH512Hidden; k += 16u) {
        h512_fetch<4>(w_row, k + 8u, b1);
        mlp512_multiply<RB>(a_row, kMlpH512Ld, k, b0, odd, acc);
        if (k + 16u < kMlpH512Hidden) h512_fetch<4>(w_row, k + 16u, b0);
        mlp512_multiply<RB>(a_row, kMlpH512Ld, k + 8u, b1, odd, acc);
    }
}

// fc1: acc = in0 (rows of 9 floats, column 7 zero) times the (512, 7) weight, k = 0 .. 7 with w[.][7] = 0
template <int RB>
__device__ __forceinline__ void mlp512_fc1(const float *__restrict__ in0, const float *__restrict__ w, uint32_t wave, uint32_t r, uint32_t half,
                                           f32x16 (&acc)[RB][4])
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float *__restrict__ row = w + ((wave * 4u + j) * 32u + r) * kMlpBaseObs;
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[rb][j][e] = 0.0f;
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t k = 2u * s + half;
            const float bv = k < kMlpBaseObs ? row[k] : 0.0f;
#pragma unroll
            for (int rb = 0; rb < RB; rb++)
                acc[rb][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(in0[(rb * 32u + r) * kMlpLd0 + k], bv, acc[rb][j], 0, 0, 0);
        }
    }
}

// relu(acc + bias) of the lane's column of each block into h, by the C/D map of the 32 x 32 tile
template <int RB>
__device__ __forceinline__ void mlp512_store(const f32x16 (&acc)[RB][4], const float *__restrict__ bias, float *__restrict__ h, uint32_t wave,
                                             uint32_t r, uint32_t half)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t col = (wave * 4u + j) * 32u + r;
        const float b = bias[col];
#pragma unroll
        for (int rb = 0; rb < RB; rb++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const uint32_t row = rb * 32u + (e & 3) + 8 * (e >> 2) + 4 * half;
                const float v = acc[rb][j][e] + b;
                h[row * kMlpH512Ld + col] = v > 0.0f ? v : 0.0f;
            }
    }
}

// LayerNorm over `rows` rows of D = 7 (J = 1) or 512 (J = 8) columns in place, a wavefront per row (wave w takes rows w, w + 4,
// ...), lane l the columns l + 64 j, j < J.  The sums' order is mlpbase_h512.hpp's.  With D = 7 lane 7 writes the zero the padded
// product reads.  Ends behind a barrier.
template <int J>
__device__ __forceinline__ void mlp512_layer_norm(float *__restrict__ x, uint32_t ld, uint32_t rows, uint32_t D, const float *__restrict__ weight,
                                                  const float *__restrict__ bias, uint32_t wave, uint32_t lane)
{
    float w[J], b[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint32_t col = lane + 64u * j;
        w[j] = col < D ? weight[col] : 0.0f, b[j] = col < D ? bias[col] : 0.0f;
    }
    const float count = (float)D;
    for (uint32_t row = wave; row < rows; row += 4u) {
        float v[J], sum = 0.0f;
#pragma unroll
        for (int j = 0; j < J; j++) {
            const uint32_t col = lane + 64u * j;
            v[j] = col < D ? x[row * ld + col] : 0.0f;
            sum += v[j];
        }
        const float mean = wave_sum(sum) / count;
        float squares = 0.0f;
#pragma unroll
        for (int j = 0; j < J; j++) {
            v[j] = lane + 64u * j < D ? v[j] - mean : 0.0f;
            squares += v[j] * v[j];
        }
        const float rstd = 1.0f / sqrtf(wave_sum(squares) / count + kMlpBaseLnEps);
#pragma unroll
        for (int j = 0; j < J; j++) {
            const uint32_t col = lane + 64u * j;
            if (col < D)
                x[row * ld + col] = (v[j] * rstd) * w[j] + b[j];
            else if (col == D && (D & 1u))
                x[row * ld + col] = 0.0f;
        }
    }
    __syncthreads();
}

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
