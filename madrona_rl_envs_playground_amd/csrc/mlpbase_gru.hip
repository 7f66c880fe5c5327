// mrl_mlpbase_gru_act: mrl_mlpbase_act for the recurrent actor-critic (mlpbase_gru.hpp; include/mrl_envs.h, MRL_MLPBASE_RECURRENT;
// DESIGN.md section 27), ONE launch per act.  Tiles and workgroups are mrl_mlpbase_act's: a workgroup of four wavefronts runs one
// net for a tile of 32 samples, blockIdx.y chooses the net.  Behind the base (mlpbase_forward<false>, the plain act's own function without its head) the
// workgroup loads the tile's 32 state rows of its net, writes them to the record's h0 row where the act starts a chunk, applies
// the mask from DONE[world], runs the GRU and its LayerNorm in LDS (mlpbase_gru_forward), the head and the plain act's tail, and
// writes h' back to the state tensor -- except in the closing value-only act, which changes neither state tensor.  A thread
// reads and writes the state elements it owns (tid, tid + 256, ...); samples outside `players` are no row of any tile, so their
// state rows keep every byte.  No float atomics, no workgroup waits on another: the same inputs give the same bits.
#include "mlpbase_gru.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char mlpbase_gru_lds_image[];

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mlpbase_gru_act(MlpBaseGruActArgs g)
{
    const MlpBaseActArgs &a = g.act;
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = a.params + (net ? gru_net_params(a.layer_N, kMlpBaseActions) : 0u);
    float *lds = reinterpret_cast<float *>(mlpbase_gru_lds_image);
    uint32_t *cell = reinterpret_cast<uint32_t *>(lds + kGruCellAt);
    float *keep = lds + kGruKeepAt, *hin = lds + kGruHinAt;
    const uint32_t tile0 = blockIdx.x * kMlpBaseTile, total = a.num_worlds * a.num_seats;

    {
        // the tile's observation rows: thread (row, k), k < 8; column 7 is never read as an input
        const bool copies = a.obs_row && net == (a.nets == 2u ? 1u : 0u);
        const uint32_t rr = tid >> 3, k = tid & 7u;
        float v = 0.0f;
        if (tile0 + rr < total) {
            uint32_t world, seat;
            seat_sample(a.players, a.num_seats, tile0 + rr, world, seat);
            if (k < kMlpBaseObs) {
                const int32_t word = a.obs[((size_t)seat * a.num_worlds + world) * kMlpBaseObs + k];
                v = (float)word;
                if (copies) a.obs_row[((size_t)world * a.P + seat) * kMlpBaseObs + k] = word;
            } else {
                cell[rr] = world * a.P + seat;
                keep[rr] = a.done[world] != 0 ? 0.0f : 1.0f;
            }
        } else if (k == kMlpBaseObs) {
            cell[rr] = kGruAbsent;
            keep[rr] = 0.0f;
        }
        lds[kMlpXhat0At + rr * kMlpLd0 + k] = v;
    }
    __syncthreads();
    mlpbase_forward<false>(params, a.layer_N, out_dim, lds, wave, lane);
    const float *x = lds + kMlpYAt + a.layer_N * kMlpBaseTile * kMlpLd;

    // the tile's state rows: the incoming state to the record where a chunk starts, then h * m
    float *__restrict__ state = g.h[net], *__restrict__ h0 = g.h0_row[net];
    for (uint32_t idx = tid; idx < kMlpBaseTile * kMlpBaseHidden; idx += kMlpBaseThreads) {
        const uint32_t rr = idx >> 6, col = idx & 63u, c = cell[rr];
        float v = 0.0f;
        if (c != kGruAbsent) {
            v = state[(size_t)c * kMlpBaseHidden + col];
            if (h0) h0[(size_t)c * kMlpBaseHidden + col] = v;
            v *= keep[rr];
        }
        hin[rr * kMlpLd + col] = v;
    }
    __syncthreads();
    mlpbase_gru_forward(params, a.layer_N, x, lds, tid);
    if (g.write_state) {
        for (uint32_t idx = tid; idx < kMlpBaseTile * kMlpBaseHidden; idx += kMlpBaseThreads) {
            const uint32_t rr = idx >> 6, col = idx & 63u, c = cell[rr];
            if (c != kGruAbsent) state[(size_t)c * kMlpBaseHidden + col] = hin[rr * kMlpLd + col];
        }
    }
    mlpbase_gru_head(params, a.layer_N, out_dim, lds, tid);

    if (tid >= kMlpBaseTile || tile0 + tid >= total) return;
    uint32_t world, seat;
    seat_sample(a.players, a.num_seats, tile0 + tid, world, seat);
    act_tail<(int)kMlpBaseActions>(a, lds + kMlpOutAt, net, tid, world, seat, a.reward);
}

void launch_mlpbase_gru_act(const MlpBaseGruActArgs &args, hipStream_t stream)
{
    const uint64_t total = (uint64_t)args.act.num_worlds * args.act.num_seats;
    if (total == 0 || args.act.nets == 0) return;
    constexpr uint32_t bytes = kGruFwdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mlpbase_gru_act>(bytes);
    const dim3 grid((uint32_t)((total + kMlpBaseTile - 1) / kMlpBaseTile), args.act.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_mlpbase_gru_act, grid, dim3(kMlpBaseThreads), bytes, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
