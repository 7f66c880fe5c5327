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

namespace mrl {

extern __shared__ __attribute__((aligned(16))) unsigned char cnn_lds_image[];

template <class Map>
__device__ __forceinline__ void cnn_act_body(const CnnActArgs &a, const Map &map, const float *__restrict__ params)
{
    const uint32_t net = act_net(a);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, r = lane & 31u, half = lane >> 5;
    const uint32_t S = a.W * a.H * a.F, k1 = a.lds.k1, K2 = kCnnChannels * a.lds.npos, out_dim = net ? 1u : kCnnActions;
    const float *__restrict__ conv_w = params + (net ? cnn_net_params(a.W, a.H, a.F, kCnnActions) : 0);
    const float *__restrict__ conv_b = conv_w + (size_t)kCnnChannels * k1;
    const float *__restrict__ fc1_w = conv_b + kCnnChannels, *__restrict__ fc1_b = fc1_w + (size_t)kCnnHidden * K2;
    const float *__restrict__ fc2_w = fc1_b + kCnnHidden, *__restrict__ fc2_b = fc2_w + kCnnHidden * kCnnHidden;
    const float *__restrict__ head_w = fc2_b + kCnnHidden, *__restrict__ head_b = head_w + out_dim * kCnnHidden;

    unsigned char *lds = cnn_lds_image;
    float *act = reinterpret_cast<float *>(lds + a.lds.act_at);
    // a row of the tile in the simulator's slab, or nullptr where the tile has no such row
    const auto row_address = [&](uint32_t rr) -> const uint8_t * {
        uint32_t world, seat;
        if (!map.sample(a, rr, world, seat)) return nullptr;
        return reinterpret_cast<const uint8_t *>(a.obs) + ((size_t)world * a.P + seat) * S;
    };
    cnn_load_tile(a, lds, row_address, nullptr, conv_w, true);
    __syncthreads();
    cnn_conv_tile(a, lds, (uint32_t)(reinterpret_cast<uintptr_t>(row_address(r)) & 3u), conv_b, wave, r, half);
    __syncthreads();  // the activation image is complete; the convolution's operands are dead

    float *chunk = reinterpret_cast<float *>(lds + kCnnChunkAt);
    float *h1 = reinterpret_cast<float *>(lds + kCnnH1At), *h2 = reinterpret_cast<float *>(lds + kCnnH2At);
    float *outs = reinterpret_cast<float *>(lds + kCnnOutAt);
    cnn_fc_layer(act, a.lds.act_ld, K2, fc1_w, fc1_b, kCnnHidden, true, chunk, h1, kCnnFcLd, wave, lane);
    cnn_fc_layer(h1, kCnnFcLd, kCnnHidden, fc2_w, fc2_b, kCnnHidden, true, chunk, h2, kCnnFcLd, wave, lane);
    cnn_fc_layer(h2, kCnnFcLd, kCnnHidden, head_w, head_b, out_dim, false, chunk, outs, 8u, wave, lane);

    uint32_t world, seat;
    if (tid >= kCnnTile || !map.sample(a, tid, world, seat)) return;
    act_tail<(int)kCnnActions>(a, outs, net, tid, world, seat, a.reward);
}

}  // namespace mrl
