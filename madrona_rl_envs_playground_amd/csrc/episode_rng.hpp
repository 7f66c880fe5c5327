// The reference's episode-seeded generator (rng.hpp:5-40), as every game that numbers its episodes draws a fresh world
// from it: Cartpole, Acrobot, the balance beam, Hanabi's deal.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mrl {

__device__ __forceinline__ uint32_t seed_of(uint32_t episode)
{
    // rng.hpp:7-26
    uint32_t v0 = episode, v1 = 0, sum = 0;
#pragma unroll
    for (int round = 0; round < 8; round++) {
        sum += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + sum) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + sum) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}

__device__ __forceinline__ float next_uniform(uint32_t &g)
{
    // rng.hpp:28-36
    g = 1664525u * g + 1013904223u;
    return (float)(g & 0x00FFFFFFu) / (float)0x01000000;
}

// the episode's first four draws, each mapped to [lo, lo + span): a fresh Cartpole (cartpole_env/sim.cpp:55-65) or
// Acrobot (acrobat_env/sim.cpp:59-65) state
__device__ __forceinline__ float4 uniform4(uint32_t episode, float lo, float span)
{
    uint32_t g = seed_of(episode);
    float4 s;
    s.x = lo + next_uniform(g) * span;
    s.y = lo + next_uniform(g) * span;
    s.z = lo + next_uniform(g) * span;
    s.w = lo + next_uniform(g) * span;
    return s;
}

}  // namespace mrl
