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
#include "mlpbase_policy.hpp"
#include "mlpbase_forward.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char mlpbase_lds_image[];

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mlpbase_act(MlpBaseActArgs a)
{
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t total = a.num_worlds * a.num_seats, tile0 = blockIdx.x * kMlpBaseTile;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = a.params + (net ? mlpbase_net_params(a.layer_N, kMlpBaseActions) : 0u);
    float *lds = reinterpret_cast<float *>(mlpbase_lds_image);

    {
        // the tile's observation rows: thread (row, k), k < 8; column 7 is never read as an input
        const bool copies = a.obs_row && net == (a.nets == 2u ? 1u : 0u);
        const uint32_t rr = tid >> 3, k = tid & 7u, s = tile0 + rr;
        float v = 0.0f;
        if (s < total && k < kMlpBaseObs) {
            uint32_t world, seat;
            seat_sample(a.players, a.num_seats, s, world, seat);
            const int32_t word = a.obs[((size_t)seat * a.num_worlds + world) * kMlpBaseObs + k];
            v = (float)word;
            if (copies) a.obs_row[((size_t)world * a.P + seat) * kMlpBaseObs + k] = word;
        }
        lds[kMlpXhat0At + rr * kMlpLd0 + k] = v;
    }
    __syncthreads();
    mlpbase_forward(params, a.layer_N, out_dim, lds, wave, lane);

    if (tid >= kMlpBaseTile || tile0 + tid >= total) return;
    uint32_t world, seat;
    seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
    act_tail<(int)kMlpBaseActions>(a, lds + kMlpOutAt, net, tid, world, seat, a.reward);
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
