// Host side of what the four games that number their episodes share (HanabiSim in hanabi.hip, CartpoleSim in
// cartpole.hip, BalanceSim in balance.hip, AcrobotSim in acrobot.hip; the device side is episode_scan.hpp): the
// double-buffered episode counter and the launch-to-launch state around it, the choice between the single-launch step and
// the two-launch pair, phase 2 in its four forms and the forced reset, which are all the game's one re-seeding launch on
// different inputs; for the three games with one lane per world also the status words of their single-launch step, its
// launch with or without in-kernel statistics (single_launch) and the random-policy rollout as one step per launch; and
// the frame of the four mrl::create_* functions (create_episode_sim).  Host-only code.
#pragma once

#include "common.hpp"
#include "episode_scan.hpp"
#include "episode_stats.hpp"
#include "world_reset.hpp"

#include <stdexcept>

namespace mrl {

// The grid both launches of the two-launch step run on: at most kMaxScanBlocks workgroups, each owning `chunk`
// consecutive worlds, chunk a multiple of what one workgroup steps at a time.
struct ScanGrid {
    uint32_t chunk, grid;
};
inline ScanGrid scan_grid(uint32_t num_worlds, uint32_t worlds_per_workgroup)
{
    const uint32_t groups = (num_worlds + worlds_per_workgroup - 1) / worlds_per_workgroup;
    const uint32_t blocks = groups < kMaxScanBlocks ? groups : kMaxScanBlocks;
    const uint32_t chunk = ((groups + blocks - 1) / blocks) * worlds_per_workgroup;
    return ScanGrid{chunk, (num_worlds + chunk - 1) / chunk};
}

// A persistent rollout kernel keeps every workgroup alive for the whole rollout and they wait for each other: does its
// grid fit the GPU in one go?
inline bool grid_resident(const void *kernel, int block_threads, uint32_t grid, int gpu_id)
{
    int per_cu = 0, cus = 0;
    MRL_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, 0));
    MRL_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, gpu_id));
    // (the occupancy query can be one workgroup per CU too high, MI355X_MICROARCH.md "Residency and
    // cooperative launch": keep one per CU in hand near the edge; the cooperative launch is the check)
    const int usable = per_cu > 4 ? per_cu - 1 : per_cu;
    return (uint64_t)grid <= (uint64_t)usable * (uint64_t)cus;
}

struct EpisodeSim : mrl_sim {
    uint32_t grid = 0, chunk = 0;  // of the two-launch step (scan_grid)
    int32_t *action = nullptr;     // the ACTION tensor (allocated by the game, among its per-world tensors)
    uint32_t *counter = nullptr;   // [2]: double-buffered episode counter, [parity] is current
    uint32_t parity = 0, epoch = 0;  // epoch: tag of the single-launch step's status words
    uint32_t *block_counts = nullptr, *reset_count = nullptr;
    uint32_t *shard_count = nullptr;  // SHARD_COUNT: finished worlds of the last mrl_step_phase1
    LaunchStateOwner launch_state;    // parity / epoch in device memory once a caller wants to capture steps (common.hpp)
    AlarmOwner alarm;                 // raised when a bounded wait expired: a persistent rollout's, or the mailbox exchange's of a sharded step
    HealTest heal;                    // test hook of the healing look-back (mrl_debug_set fused_heal_test)
    bool fused = false;               // mrl_step is one launch with the in-kernel look-back, not the two-launch pair
    // single-launch step of Cartpole, the balance beam and Acrobot (alloc_fused): 32-bit status words and, per kGroup
    // workgroups, their total (grouped_prefix); fused_grid == 0: the batch is too large for it.  Hanabi has 64-bit words of its own.
    uint32_t *status = nullptr;
    unsigned long long *group_total = nullptr;
    uint32_t fused_grid = 0;

    // ---- what a game supplies ----
    // Where a re-seeding launch finds the finished worlds -- mask words (Cartpole, balance beam) or flags (Hanabi), and their
    // number per workgroup -- and where it leaves RESET_COUNT.  A game reads one of words / flags; the other is null.
    struct Finished {
        unsigned long long *words;
        int32_t *flags;
        uint32_t *block_counts;
        uint32_t *reset_count;
    };
    // What a counted launch reads and writes: this step's first episode, where the next step's goes, and the same in device mode.
    struct Counters {
        const uint32_t *base;
        uint32_t *next;
        DeviceCounter device;
    };
    // the random policy drawn inside the step (mrl_rollout_random); action_out == nullptr: the caller's actions.  Not
    // Hanabi: its policy travels in its HanabiParams and its launch_fused does not look at a Drawn
    struct Drawn {
        int32_t *action_out = nullptr;
        uint64_t seed = 0;
        uint32_t step = 0;
    };
    virtual void launch_fused(const int32_t *actions, const Drawn &drawn, const FusedExchange &fx, const Counters &c, hipStream_t stream) = 0;
    virtual void launch_reseed(const Finished &from, const GatheredCounts &gathered, const Counters &c, hipStream_t stream) = 0;
    // phase 1 with the policy's draws made in the step kernel and written to action_out (nullptr: the caller's actions):
    // the games whose two-launch step kernel can draw (balance beam, Acrobot), for rollout_random below
    virtual void launch_step(const int32_t *, int32_t *, uint64_t, uint32_t, hipStream_t)
    {
        throw std::runtime_error("this game's step kernel draws no actions");
    }
    Finished stepped{};  // what phase 1 leaves (alloc_episode; Hanabi sets its flags)
    // mrl_enable_episode_stats: the single-launch steps of Cartpole, Acrobot and the balance beam keep the statistics in
    // their own kernel (their launch_fused asks this, launches the kStats instantiation and sets stats_taken); every other
    // step is followed by the general update launch (capi.hip).  A measurement build without the in-kernel form, to
    // compare the two: make EXTRA_CXXFLAGS=-DMRL_STATS_GENERAL_ONLY (tools/episode_stats_probe.py)
#ifdef MRL_STATS_GENERAL_ONLY
    bool stats_in_step() const { return false; }
#else
    bool stats_in_step() const { return stats != nullptr; }
#endif

    // One launch that takes episode numbers: the device copy of the state advanced first, the counter's halves as of before
    // the flip.  (Graph replay depends on this order.)  launch(Counters)
    template <typename Launch> void counted_launch(bool new_epoch, const uint32_t *external_base, hipStream_t stream, Launch &&launch)
    {
        if (new_epoch) epoch += 1;
        if (launch_state.device_mode) launch_state.advance(stream);  // then parity / epoch come from device memory
        launch(Counters{external_base ? external_base : counter + parity, counter + (parity ^ 1u),
                        launch_state.counter_args(counter, external_base != nullptr)});
        MRL_HIP(hipGetLastError());
        parity ^= 1u;
    }
    void fused_step(const int32_t *actions, const Drawn &drawn, const FusedExchange &fx, hipStream_t stream)
    {
        counted_launch(true, nullptr, stream, [&](const Counters &c) { launch_fused(actions, drawn, fx, c, stream); });
    }
    // What a lane-per-world game's launch_fused is: the kernel's instantiation with or without the in-kernel statistics on
    // fused_grid, `lead...` being the kernel's arguments in front of the statistics argument, which is appended here.  The
    // call returns the launch itself, to be called with whatever the kernel takes behind it (Cartpole's diagnostic stamps).
    template <typename WithStats, typename Plain, typename... Lead>
    auto single_launch(WithStats with_stats, Plain plain, uint32_t block, hipStream_t stream, Lead... lead)
    {
        return [=](auto... tail) {
            if (stats_in_step())
                hipLaunchKernelGGL(with_stats, dim3(fused_grid), dim3(block), 0, stream, lead..., stats->lane(), tail...);
            else
                hipLaunchKernelGGL(plain, dim3(fused_grid), dim3(block), 0, stream, lead..., NoStats{}, tail...);
            stats_taken = stats_in_step();
        };
    }
    void reseed(const Finished &from, const uint32_t *external_base, const GatheredCounts &gathered, hipStream_t stream)
    {
        counted_launch(false, external_base, stream, [&](const Counters &c) { launch_reseed(from, gathered, c, stream); });
    }

    void step(const int32_t *actions, hipStream_t stream) override
    {
        if (fused)
            fused_step(actions, Drawn{}, FusedExchange{}, stream);
        else
            mrl_sim::step(actions, stream);
    }
    // a shard's step with the other ranks' counts taken from the mailboxes inside the single launch (episode_scan.hpp)
    void step_exchanged(const int32_t *actions, hipStream_t stream) override
    {
        if (fused)
            fused_step(actions, Drawn{}, fused_exchange_of(exchange, alarm.alarm()), stream);
        else
            mrl_sim::step_exchanged(actions, stream);
    }
    void publish_shard_count(hipStream_t stream) override
    {
        hipLaunchKernelGGL(sum_block_counts, dim3(1), dim3(256), 0, stream, block_counts, grid, shard_count, mail_of(exchange));
        MRL_HIP(hipGetLastError());
    }
    // mrl_rollout_random, one step per launch (two without the single-launch step); the draws are made inside the step.
    // Cartpole and Hanabi, which have a persistent rollout kernel in front of this, override it.
    void rollout_random(uint32_t num_steps, uint64_t seed, uint32_t first_step, hipStream_t stream) override
    {
        for (uint32_t k = 0; k < num_steps; k++) {
            if (fused) {
                fused_step(action, Drawn{action, seed, first_step + k}, FusedExchange{}, stream);
            } else {
                launch_step(action, action, seed, first_step + k, stream);
                phase2(nullptr, stream);
            }
        }
    }
    void phase2(const uint32_t *episode_base_dev, hipStream_t stream) override { reseed(stepped, episode_base_dev, GatheredCounts{}, stream); }
    void phase2_gathered(const uint32_t *counts, uint32_t num_ranks, uint32_t rank, hipStream_t stream) override
    {
        GatheredCounts g;
        g.counts = counts;
        g.num_ranks = num_ranks;
        g.rank = rank;
        reseed(stepped, nullptr, g, stream);
    }
    void phase2_exchanged(hipStream_t stream) override { reseed(stepped, nullptr, polled_counts(exchange, alarm.alarm()), stream); }
    // mrl_reset_worlds: phase 2 on the caller's mask, with a scratch RESET_COUNT (world_reset.hpp)
    ResetScratch forced;
    void reset_worlds(const uint8_t *mask_dev, hipStream_t stream) override
    {
        forced.build(mask_dev, num_worlds, grid, chunk, stream);
        reseed(Finished{forced.words, forced.flags, forced.block_counts, forced.reset_count}, nullptr, GatheredCounts{}, stream);
    }

    bool scan_timed_out() const override { return alarm.raised(); }
    bool capturable() const override { return launch_state.device_mode; }
    void prepare_graph_capture(hipStream_t stream) override { launch_state.to_device(parity, epoch, stream); }
    void set_episode_counter(uint32_t next_episode, hipStream_t stream) override
    {
        if (launch_state.device_mode) {  // which half is current is only known on the device
            hipLaunchKernelGGL(set_current_counter, dim3(1), dim3(1), 0, stream, counter, launch_state.dev, next_episode);
            MRL_HIP(hipGetLastError());
        } else {
            MRL_HIP(hipMemcpyAsync(counter + parity, &next_episode, sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        MRL_HIP(hipStreamSynchronize(stream));
    }

    // ---- construction (create_episode_sim below is the frame; these are what a game's part of it calls) ----
    // first: grid and chunk of the two-launch step (the game's own allocations depend on them)
    void size_scan_grid(uint32_t worlds_per_workgroup)
    {
        const ScanGrid g = scan_grid(num_worlds, worlds_per_workgroup);
        chunk = g.chunk;
        grid = g.grid;
    }
    // Then what lives in device memory.  Every game makes these allocations BEHIND its per-world tensors and in exactly the
    // sequence it used before this header existed, which is why the alarm and the launch state are left to the game
    // (alarm.init, launch_state.init: the balance beam has them the other way round) and why what is already allocated is
    // skipped here (Hanabi allocates block_counts and shard_count itself, right behind its DONE tensor).  Where these few
    // words land decides the speed of a kernel that is otherwise the same: Cartpole's single-launch step at 1 M worlds,
    // 9.1-9.2 us, ran 9.7-9.9 us with all of this allocated in front of the tensors, and 9.4-9.6 us with only the launch
    // state and the alarm in front of its status words instead of behind them (profiles/episode_host_bench_ab.txt).
    // alloc_episode: the counts, the step's own mask words (Cartpole, balance beam), the counter, the forced reset's scratch
    // with mask words or flags, whichever the game's re-seeding launch reads
    void alloc_episode(bool with_words, bool with_flags)
    {
        if (!block_counts) block_counts = arena.alloc<uint32_t>(grid);
        if (with_words) stepped.words = arena.alloc<unsigned long long>(((size_t)grid * chunk + 63) / 64);
        counter = arena.alloc<uint32_t>(2);
        reset_count = arena.alloc<uint32_t>(1);
        if (!shard_count) shard_count = arena.alloc<uint32_t>(1);
        forced.init(arena, grid, chunk, num_worlds, with_words, with_flags);
        stepped.block_counts = block_counts;
        stepped.reset_count = reset_count;
    }
    // the single-launch step's status words, where the game's own block stood (see above: the sequence of allocations is the
    // game's); nothing for a batch of more than kMaxFusedBlocks workgroups
    void alloc_fused(uint32_t worlds_per_workgroup)
    {
        const uint32_t blocks = (num_worlds + worlds_per_workgroup - 1) / worlds_per_workgroup;
        if (blocks > kMaxFusedBlocks) return;
        fused_grid = blocks;
        status = arena.alloc<uint32_t>(blocks);
        group_total = arena.alloc<unsigned long long>((blocks + kGroup - 1) / kGroup);
    }
    // mrl_debug_set fused_step: 0 = the library's choice (one launch wherever the game has one for this batch: `exists`),
    // 1 = one launch where possible, 2 = always two; fused_heal_test: see HealTest (one word per workgroup of the single launch)
    void read_step_knobs(bool exists, uint32_t fused_blocks)
    {
        fused = exists && debug_get("fused_step", 0) != 2;
        heal.mod = (uint32_t)debug_get("fused_heal_test", 0);
        heal.seen = arena.alloc<uint32_t>(fused_blocks);
    }
    // test hook (mrl_debug_set inject_scan_timeout), for the games that export SCAN_TIMEOUT
    void inject_scan_timeout()
    {
        if (debug_get("inject_scan_timeout", 0)) hipLaunchKernelGGL(raise_alarm_kernel, dim3(1), dim3(1), 0, 0, alarm.alarm());
    }
};

// mrl::create_<game> of the four games: refuses an empty batch, binds the device, and runs init(sim) -- the game's
// allocations in the game's own sequence (see alloc_episode), its first episodes -- on a new Sim that does not outlive a throw.
template <typename Sim, typename Init> mrl_sim *create_episode_sim(const char *name, int game, int gpu_id, uint32_t num_worlds, Init &&init)
{
    if (num_worlds == 0) {
        set_error("%s: num_worlds must be > 0", name);
        throw HipError{MRL_ERR_INVALID};
    }
    bind_device(gpu_id);
    auto *sim = new Sim();
    try {
        sim->game = game;
        sim->device = gpu_id;
        sim->num_worlds = num_worlds;
        init(sim);
        MRL_HIP(hipDeviceSynchronize());
    } catch (...) {
        delete sim;
        throw;
    }
    return sim;
}

}  // namespace mrl
