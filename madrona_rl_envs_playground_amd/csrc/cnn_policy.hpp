// MAPPO's CNN actor-critic for Overcooked on the device (C ABI: mrl_cnn_act, mrl_rollout_cnn in include/mrl_envs.h; DESIGN.md
// section 15).  The kernel lives in cnn_policy.hip; capi_mappo.hip validates the arguments and collects the simulator's tensors.
//
// THE INDEX MAP.  The simulator writes obs[n, p, y, x, f] (world-major, int8, y < H, x < W).  The reference hands the network
// the view (N, W, H, F) and moves the channels forward, so torch sees x[n, f, w, h] = obs[n, p, h, w, f]: the convolution's
// FIRST spatial axis is the kitchen's x.  For the conv weight Wc[c, f, i, j]:
//     conv[n, c, ow, oh] = bc[c] + sum over (f, i, j) of Wc[c, f, i, j] * obs[n, p, oh + j, ow + i, f]      ow < W - 2, oh < H - 2
// and torch's flatten gives fc1 the index c * (W - 2) * (H - 2) + ow * (H - 2) + oh.
// Every dot product is one chain of fused multiply-adds from 0 in ascending order of torch's own flattened weight index
// (conv: k = f * 9 + i * 3 + j; the linear layers: their input index; an odd K is padded with one zero product), and the bias is
// added to the finished sum.
#pragma once

#include "act_record.hpp"
#include "common.hpp"

#include <atomic>

namespace mrl {

constexpr uint32_t kCnnHidden = 64, kCnnChannels = 32, kCnnActions = 6, kCnnTile = 32, kCnnThreads = 256, kCnnChunk = 64;
constexpr uint32_t kCnnLdsLimit = 160u * 1024u;  // one workgroup's LDS on gfx950
constexpr uint64_t kCnnWorkspaceBytes = 256;

// one net: conv (32, F, 3, 3) + bias, fc1 (64, 32 * npos) + bias, fc2 (64, 64) + bias, head (out, 64) + bias
constexpr uint64_t cnn_net_params(uint64_t W, uint64_t H, uint64_t F, uint64_t out)
{
    return kCnnChannels * F * 9 + kCnnChannels + kCnnHidden * (kCnnChannels * (W - 2) * (H - 2)) + kCnnHidden +
           (uint64_t)kCnnHidden * kCnnHidden + kCnnHidden + out * kCnnHidden + out;
}

// The workgroup's LDS image (bytes), for 32 samples of one net:
//   region A, convolution: the observation rows as int8 (row stride obs_ld: room for a row that starts up to 3 bytes off a
//     4-byte boundary, in dwords an odd number so that the 32 rows sit on 32 banks), the conv weights (32 rows of conv_ld
//     floats, conv_ld odd), the patch offsets of k (uint16);
//   region A again, linear layers (the convolution's operands are dead by then): a 64-column x 64-k weight chunk, h1, h2
//     (rows of 65 floats) and the head's outputs (32 x 8);
//   region B: the convolution's output, 32 rows of act_ld = 32 * npos + 1 floats.
struct CnnLds {
    uint32_t obs_ld, conv_ld, k1, k1_padded, npos, act_ld;
    uint32_t conv_w_at, koff_at, act_at, total;  // byte offsets
};
constexpr uint32_t kCnnFcLd = kCnnChunk + 1;
constexpr uint32_t kCnnChunkAt = 0, kCnnH1At = kCnnHidden * kCnnFcLd * 4, kCnnH2At = kCnnH1At + kCnnTile * kCnnFcLd * 4,
                   kCnnOutAt = kCnnH2At + kCnnTile * kCnnFcLd * 4, kCnnFcBytes = kCnnOutAt + kCnnTile * 8 * 4;
inline CnnLds cnn_lds(uint32_t W, uint32_t H, uint32_t F)
{
    CnnLds l{};
    const uint32_t S = W * H * F;
    l.obs_ld = (S + 3u + 3u) & ~3u;
    if (((l.obs_ld / 4u) & 1u) == 0) l.obs_ld += 4u;
    l.k1 = 9u * F;
    l.k1_padded = (l.k1 + 1u) & ~1u;
    l.conv_ld = l.k1_padded | 1u;
    l.npos = (W - 2u) * (H - 2u);
    l.act_ld = kCnnChannels * l.npos + 1u;
    l.conv_w_at = kCnnTile * l.obs_ld;
    l.koff_at = l.conv_w_at + kCnnChannels * l.conv_ld * 4u;
    uint32_t region_a = (l.koff_at + l.k1_padded * 2u + 15u) & ~15u;
    if (region_a < kCnnFcBytes) region_a = kCnnFcBytes;
    l.act_at = region_a;
    l.total = l.act_at + kCnnTile * l.act_ld * 4u;
    return l;
}

struct CnnActArgs : ActArgs {
    const float *params;       // actor's tensors, then the critic's
    const int8_t *obs;         // (N, P, H, W, F)
    const int32_t *reward;     // REWARD (P, N)
    // on an 8-byte boundary, so that the kernels fetch it in wide scalar loads: four bytes off, mrl_mappo_grad (cnn_update.hip)
    // compiles to 30 more spilled SGPRs and 60 more instructions
    alignas(8) CnnLds lds;
    uint32_t W, H, F;
};

void launch_cnn_act(const CnnActArgs &args, hipStream_t stream);

// Before a launch of KERNEL with `bytes` of dynamic LDS: more than the default limit, and the runtime is told once per device
// and kernel (a refusal shows in the launch that follows).
template <auto KERNEL>
inline void allow_large_dynamic_lds(uint32_t bytes)
{
    static std::atomic<bool> told[64];
    int device = 0;
    if (bytes > 64u * 1024u && hipGetDevice(&device) == hipSuccess && device >= 0 && device < 64 && !told[device].load()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCnnLdsLimit) !=
            hipSuccess)
            (void)hipGetLastError();
        told[device].store(true);
    }
}

}  // namespace mrl
