// The body of mrl_mlpbase_act (mlpbase_policy.hip describes the workgroup and the arithmetic), templated on the map from a
// tile's row to its sample so that two kernels share it: mrl_mlpbase_act, whose tile t holds samples 32 t .. 32 t + 31 of the
// `players` mask, and mrl_mlpbase_act_bank (mlpbase_bank.hip), whose tile holds up to 32 samples of ONE policy of a bank, listed
// by the plan.  A map offers
//     bool has(uint32_t row) const                                                              the tile has such a row
//     void locate(const MlpBaseActArgs &a, uint32_t row, uint32_t &world, uint32_t &seat) const   its sample, for a row it has
// (two calls and not cnn_act_body's one `sample`: the loader tests the row, then the column, then resolves the sample, and in that
// order the plain kernel compiles to the instructions it had before there was a map)
// and the caller hands in the parameter array the tile runs.  A sample's arithmetic reads its own LDS rows and the tile's common
// weights only, so which other samples share its tile cannot change a bit of its outputs.
#pragma once

#include "mlpbase_policy.hpp"
#include "mlpbase_forward.hpp"

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char mlpbase_lds_image[];

template <class Map>
__device__ __forceinline__ void mlpbase_act_body(const MlpBaseActArgs &a, const Map &map, const float *__restrict__ policy)
{
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t out_dim = net ? 1u : kMlpBaseActions;
    const float *__restrict__ params = policy + (net ? mlpbase_net_params(a.layer_N, kMlpBaseActions) : 0u);
    float *lds = reinterpret_cast<float *>(mlpbase_lds_image);

    {
        // the tile's observation rows: thread (row, k), k < 8; column 7 is never read as an input
        const bool copies = a.obs_row && net == (a.nets == 2u ? 1u : 0u);
        const uint32_t rr = tid >> 3, k = tid & 7u;
        float v = 0.0f;
        if (map.has(rr) && k < kMlpBaseObs) {
            uint32_t world, seat;
            map.locate(a, rr, world, seat);
            const int32_t word = a.obs[((size_t)seat * a.num_worlds + world) * kMlpBaseObs + k];
            v = (float)word;
            if (copies) a.obs_row[((size_t)world * a.P + seat) * kMlpBaseObs + k] = word;
        }
        lds[kMlpXhat0At + rr * kMlpLd0 + k] = v;
    }
    __syncthreads();
    mlpbase_forward(params, a.layer_N, out_dim, lds, wave, lane);

    if (tid >= kMlpBaseTile || !map.has(tid)) return;
    uint32_t world, seat;
    map.locate(a, tid, world, seat);
    act_tail<(int)kMlpBaseActions>(a, lds + kMlpOutAt, net, tid, world, seat, a.reward);
}

}  // namespace mrl
