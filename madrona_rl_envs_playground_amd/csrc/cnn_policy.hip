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
#include "cnn_act_body.hpp"

namespace mrl {

// tile t of the call holds samples 32 t .. 32 t + 31 (cnn_act_body's map)
struct CnnPlainMap {
    uint32_t tile0, total;
    __device__ __forceinline__ bool sample(const CnnActArgs &a, uint32_t row, uint32_t &world, uint32_t &seat) const
    {
        if (tile0 + row >= total) return false;
        seat_sample(a.players, a.num_seats, tile0 + row, world, seat);
        return true;
    }
};

__global__ void __launch_bounds__(kCnnThreads) mrl_cnn_act(CnnActArgs a)
{
    cnn_act_body(a, CnnPlainMap{blockIdx.x * kCnnTile, a.num_worlds * a.num_seats}, a.params);
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
