// mrl_mlpbase_act: both nets of MAPPO's MLPBase actor-critic for the balance beam (train/MAPPO/utils/mlp.py, r_actor_critic.py,
// utils/distributions.py:55-68 with hidden_size 64) and the head, ONE launch per act (include/mrl_envs.h; DESIGN.md section 18;
// the network, the flat tensor and the LDS image are in mlpbase_policy.hpp).
//
// A workgroup of four wavefronts runs one net for a tile of 32 samples (sample = world n, seat p of the `players` mask, in
// that order); blockIdx.y chooses the net.  It reads the tile's rows of OBSERVATION (P, N, 7) int32 in place, converting on load.
//   LayerNorm     a wavefront per row, one fixed summation order (mlpbase_forward.hpp, wave_sum)
//   Linear        cnn_fc_layer (cnn_forward.hpp): v_mfma_f32_32x32x2_f32, an output is 0, then fmaf over k ascending, and the bias
//                 is added to the finished sum; K = 7 is padded with one zero product
//   head          lanes 0..31 of wave 0, a sample each: soft-max, draw, log-prob (mrl_cnn_act's rule with four actions); the
//                 critic's workgroup writes the value, the reward and the done flag; the actor's (the critic's in a value-only
//                 act) copies the observation rows into the record.
// The balance beam's ACTION_MASK is all ones in every state (src/balance_beam_env/sim.cpp:197); the kernel does not read it.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "mlpbase_act_body.hpp"

namespace mrl {

// tile t of the call holds samples 32 t .. 32 t + 31 (mlpbase_act_body's map)
struct MlpBasePlainMap {
    uint32_t tile0, total;
    __device__ __forceinline__ bool has(uint32_t row) const { return tile0 + row < total; }
    __device__ __forceinline__ void locate(const MlpBaseActArgs &a, uint32_t row, uint32_t &world, uint32_t &seat) const
    {
        seat_sample(a.players, a.num_seats, tile0 + row, world, seat);
    }
};

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mlpbase_act(MlpBaseActArgs a)
{
    mlpbase_act_body(a, MlpBasePlainMap{blockIdx.x * kMlpBaseTile, a.num_worlds * a.num_seats}, a.params);
}

void launch_mlpbase_act(const MlpBaseActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.num_worlds * args.num_seats;
    if (total == 0 || args.nets == 0) return;
    constexpr uint32_t bytes = kMlpFwdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mlpbase_act>(bytes);
    const dim3 grid((uint32_t)((total + kMlpBaseTile - 1) / kMlpBaseTile), args.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_mlpbase_act, grid, dim3(kMlpBaseThreads), bytes, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
