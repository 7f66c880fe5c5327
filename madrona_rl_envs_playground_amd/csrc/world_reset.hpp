// mrl_reset_worlds (include/mrl_envs.h): restart the worlds a caller picks, in every game.  Kernels: world_reset.hip.
//
// Hanabi, Cartpole and the balance beam: the re-seeding launch of the two-launch step (phase 2) already restarts a set of
// flagged worlds as episodes counter, counter + 1, ... in ascending world order and advances the counter.  A forced reset
// is that launch run on the CALLER'S flags: mrl_reset_mask_counts turns the byte mask into what phase 2 reads -- one 64-bit
// ballot word per 64 worlds (Cartpole, balance beam) or int32 flags (Hanabi), and the number of flagged worlds per
// workgroup of the phase-2 grid -- in scratch buffers of the simulator's own, and phase 2 then runs with a scratch
// RESET_COUNT, so DONE, REWARD and RESET_COUNT keep the values of the last step.
//
// Overcooked and Simplecooked have no episode index: every restart is the same start state.  The simulator keeps world 0
// as its construction left it (state and observation slab: FreshWorldOwner) and mrl_cooked_reset copies it over the
// masked worlds, one wavefront per world, whatever the step kernel's launch shape, player count or layout.
#pragma once

#include "common.hpp"

#include <initializer_list>
#include <utility>

namespace mrl {

// The fill kernels behind the simulators' constant tensors; on the null stream.  fill_ids: world_id[i] = i % n,
// row_id[i] = i / n for i < rows * n; row_id == nullptr: a game with one row (Cartpole, Acrobot).  (kitchen_host.hpp, which includes this header, still repeats the two declarations.)
void fill_ids(int32_t *world_id, int32_t *row_id, uint32_t rows, uint32_t n);
void fill_i32(int32_t *dst, int32_t value, size_t count);

// Scratch of a forced reset in the counter games: the phase-2 inputs built from the mask, and the RESET_COUNT phase 2 writes.
struct ResetScratch {
    unsigned long long *words = nullptr;
    int32_t *flags = nullptr;
    uint32_t *block_counts = nullptr;
    uint32_t *reset_count = nullptr;
    void init(DeviceArena &arena, uint32_t grid, uint32_t chunk, uint32_t num_worlds, bool with_words, bool with_flags)
    {
        if (with_words) words = arena.alloc<unsigned long long>(((size_t)grid * chunk + 63) / 64);
        if (with_flags) flags = arena.alloc<int32_t>(num_worlds);
        block_counts = arena.alloc<uint32_t>(grid);
        reset_count = arena.alloc<uint32_t>(1);
    }
    // mrl_reset_mask_counts over the phase-2 grid (grid workgroups of `chunk` worlds); mask_dev == nullptr: every world
    void build(const uint8_t *mask_dev, uint32_t n, uint32_t grid, uint32_t chunk, hipStream_t stream) const;
};

// A fresh world of Overcooked / Simplecooked: up to three per-world state arrays (32-bit words) and the observation slab.
struct FreshWorld {
    enum { kArrays = 3 };  // (an enum: a static constexpr member here breaks the host pass of grid_common.hpp's inline asm)
    uint32_t *dst[kArrays] = {};        // the simulator's arrays: world w's entry is dst[k] + w * words[k]
    const uint32_t *src[kArrays] = {};  // the fresh world's entries
    uint32_t words[kArrays] = {};
    const uint8_t *obs_src = nullptr;   // obs_bytes, 16-byte aligned
    uint8_t *obs = nullptr;             // world w's slab at obs + w * obs_bytes
    uint32_t obs_bytes = 0;
    uint32_t obs_grain = 1;             // 16, 4 or 1: the widest store that keeps every slab's stores aligned
};

struct FreshWorldOwner {
    FreshWorld f{};
    // the copy of world 0: arrays = {simulator array, 32-bit words per world}, obs = the construction's slab (world 0
    // first).  Synchronous: called once, right after construction.
    void init(DeviceArena &arena, std::initializer_list<std::pair<uint32_t *, uint32_t>> arrays, const uint8_t *obs, uint32_t obs_bytes);
    // mrl_cooked_reset: the masked worlds (mask_dev == nullptr: all n) <- the copy; their observation slabs go to obs_dest
    void launch(const uint8_t *mask_dev, uint32_t n, uint8_t *obs_dest, hipStream_t stream) const;
};

}  // namespace mrl
