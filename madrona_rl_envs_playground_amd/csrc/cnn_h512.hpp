// MAPPO's CNN actor-critic at the reference trainer's default hidden_size 512 (train/config.py:200; CNNLayer then is
// Conv2d(F, 256, 3 x 3), Linear(256 npos, 512), Linear(512, 512) and a head of 6 logits or one value): the act and the rollout
// (C ABI: mrl_cnn_act and mrl_rollout_cnn with mrl_cnn_policy.hidden = 512).  The kernel lives in
// cnn_h512.hip; capi_mappo.hip validates the arguments.  The index map is cnn_policy.hpp's.
//
// THE ORDER OF EVERY SUM.  As in the plain act, a dot product is a chain of fused multiply-adds from 0 in ascending order of
// torch's own flattened weight index, and the bias is added to the finished sum:
//   convolution   k = f 9 + i 3 + j, an odd K padded with one zero product (cnn_conv_pass);
//   fc1           the 256 channels run as 8 blocks of 32.  Block b's 32 npos activations are the contiguous range
//                 [b 32 npos, (b + 1) 32 npos) of torch's index c npos + ow (H - 2) + oh.  Each block's sum is its OWN chain from 0
//                 over that range, and the eight block sums are added in ascending b to a running sum that starts at 0 (both sets
//                 of accumulators stay in registers).  One chain over all 256 npos products -- 6400 at npos 25 -- drifted to 9 times
//                 torch float32's own distance from the float64 module there; chains of 32 npos do not;
//   fc2, head     k = 0 .. 511, one chain.
// A matrix instruction takes k = 2 kk (lanes 0..31) and 2 kk + 1 (lanes 32..63), in that order.
#pragma once

#include "cnn_policy.hpp"

namespace mrl {

constexpr uint32_t kCnnH512Hidden = 512, kCnnH512Channels = 256;
constexpr uint32_t kCnnH512Blocks = kCnnH512Channels / kCnnChannels;  // channel blocks of the plain act's 32
constexpr uint32_t kCnnH512HLd = kCnnH512Hidden + 1;                  // a row of h1 / h2 in LDS: odd, lane r reads bank r + k

// one net: conv (256, F, 3, 3) + bias, fc1 (512, 256 * npos) + bias, fc2 (512, 512) + bias, head (out, 512) + bias
constexpr uint64_t cnn_h512_net_params(uint64_t W, uint64_t H, uint64_t F, uint64_t out)
{
    return kCnnH512Channels * F * 9 + kCnnH512Channels + kCnnH512Hidden * (kCnnH512Channels * (W - 2) * (H - 2)) + kCnnH512Hidden +
           (uint64_t)kCnnH512Hidden * kCnnH512Hidden + kCnnH512Hidden + out * kCnnH512Hidden + out;
}

// The workgroup's LDS image (bytes), for 32 samples of one net:
//   during the channel loop  exactly the plain act's image cnn_lds(W, H, F): the int8 rows (loaded once), ONE block's conv
//     weights and the patch offsets in region A, that block's activations (32 rows of 32 npos + 1 floats) in region B;
//   behind fc1 (all of that is dead)  h, 32 rows of 513 floats -- h1, then h2 in place: fc2's sums wait in registers until every
//     wave has read h1 -- and the head's outputs (32 x 8).
// The weights of fc1, fc2 and the head never pass through LDS (cnn_h512.hip says why).
struct CnnH512Lds {
    CnnLds conv;
    uint32_t h_at, out_at, total;  // byte offsets
};
inline CnnH512Lds cnn_h512_lds(uint32_t W, uint32_t H, uint32_t F)
{
    CnnH512Lds l{};
    l.conv = cnn_lds(W, H, F);
    l.h_at = 0;
    l.out_at = kCnnTile * kCnnH512HLd * 4u;
    const uint32_t behind = l.out_at + kCnnTile * 8u * 4u;
    l.total = l.conv.total > behind ? l.conv.total : behind;
    return l;
}

// `args` as for launch_cnn_act (args.lds = cnn_lds(W, H, F)), args.params a hidden-512 parameter array
void launch_cnn_act_h512(const CnnActArgs &args, hipStream_t stream);

}  // namespace mrl
