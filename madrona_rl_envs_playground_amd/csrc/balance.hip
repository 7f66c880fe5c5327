// "Balance beam" world step for gfx950 (the reference's balance_beam_env): two agents on a line of five
// spaces, three steps per episode; one lane per world.
//
// Semantics: /root/reference/src/balance_beam_env/sim.cpp:76-92 (actionSystem: moves -2, -1, +1, +2),
// :94-97 (timeSystem), :99-112 (observationSystem: a three-deep history of own and partner positions,
// shifted by one per step), :114-151 (checkDone: reward, out-of-range and time-out termination),
// :45-74 (resetWorld from the episode-seeded generator, rng.hpp:5-40), graph :155-171.
//
// The whole world state is IN the observation the reference exports: obs.x[0] = own position + BUFFER,
// obs.time = steps left (sim.cpp:109-111), so the kernel keeps no other per-world array.  The history
// shift of the reference runs `for (i = 2*TIME; i > 0; i--) x[i] = x[i-1]` over an array of 2*TIME
// entries, i.e. it also writes x[6], which is the `time` field that follows it in the struct
// (sim.hpp:52-55) and is assigned right after; and x[TIME] is assigned right after as well.  Net effect,
// reproduced here: x[5] = x[4], x[4] = x[3], x[2] = x[1], x[1] = x[0], x[3] = partner + BUFFER,
// x[0] = own + BUFFER.
//
// Episode indices are taken in ascending world order within a step (see cartpole.hip):
//   mrl_step_phase1  mrl_balance_step : moves, history, reward, done flag, per-workgroup finished counts
//   mrl_step_phase2  mrl::reseed_finished<BalanceReseed>: exclusive prefix over the counts, re-seed finished worlds
//                    (episode_scan.hpp)
// and mrl_step is the two in a row.
#include "episode_host.hpp"
#include "episode_rng.hpp"
#include "random_policy.hpp"

namespace {

constexpr int kBlock = 256;
constexpr int kTime = 3, kSpaces = 5, kBuffer = 2, kRow = 2 * kTime + 1;  // sim.cpp:9-13, sim.hpp:8

struct Row {
    int32_t x[kRow];  // x[0..5] history, x[6] = time left
};

__device__ __forceinline__ Row load_row(const int32_t *obs, uint32_t n, uint32_t agent, uint32_t w)
{
    Row r;
    const int32_t *src = obs + ((size_t)agent * n + w) * kRow;
#pragma unroll
    for (int k = 0; k < kRow; k++) r.x[k] = src[k];
    return r;
}

__device__ __forceinline__ void store_row(int32_t *obs, uint32_t n, uint32_t agent, uint32_t w, const Row &r)
{
    int32_t *dst = obs + ((size_t)agent * n + w) * kRow;
#pragma unroll
    for (int k = 0; k < kRow; k++) dst[k] = r.x[k];
}

// resetWorld (sim.cpp:45-74): positions from the episode's generator, empty history
__device__ __forceinline__ void fresh_rows(uint32_t episode, Row &r0, Row &r1)
{
    uint32_t g = mrl::seed_of(episode);
    const int32_t loc0 = (int32_t)(kSpaces * mrl::next_uniform(g));
    const int32_t loc1 = (int32_t)(kSpaces * mrl::next_uniform(g));
#pragma unroll
    for (int k = 0; k < 2 * kTime; k++) r0.x[k] = r1.x[k] = 0;
    r0.x[0] = loc0 + kBuffer;
    r0.x[kTime] = loc1 + kBuffer;
    r1.x[0] = loc1 + kBuffer;
    r1.x[kTime] = loc0 + kBuffer;
    r0.x[2 * kTime] = r1.x[2 * kTime] = kTime - 1;
}

// what the re-seeding launches store for a world that starts `episode` (mrl::reseed_finished, mrl::reseed_all)
struct BalanceReseed {
    int32_t *obs;
    uint32_t n;
    __device__ __forceinline__ void operator()(uint32_t world, uint32_t episode) const
    {
        Row r0, r1;
        fresh_rows(episode, r0, r1);
        store_row(obs, n, 0, world, r0);
        store_row(obs, n, 1, world, r1);
    }
};

__device__ __forceinline__ int32_t move_of(int32_t choice)
{
    // sim.cpp:78-91; anything else leaves the agent where it is
    return choice == 0 ? -2 : choice == 1 ? -1 : choice == 2 ? 1 : choice == 3 ? 2 : 0;
}

__device__ __forceinline__ void shift_history(Row &r, int32_t own, int32_t partner, int32_t time)
{
    // sim.cpp:104-111, see the header of this file
    r.x[5] = r.x[4];
    r.x[4] = r.x[3];
    r.x[2] = r.x[1];
    r.x[1] = r.x[0];
    r.x[kTime] = partner + kBuffer;
    r.x[0] = own + kBuffer;
    r.x[2 * kTime] = time;
}

// One world's step on its two rows: moves, history, reward, termination (sim.cpp:76-151).  Pure in (rows, actions):
// the single-launch step's healing look-back re-runs it on another workgroup's inputs to learn how many of its worlds finish.
__device__ __forceinline__ bool move_world(Row &r0, Row &r1, int32_t a0, int32_t a1, float &rew)
{
    const int32_t loc0 = r0.x[0] - kBuffer + move_of(a0), loc1 = r1.x[0] - kBuffer + move_of(a1);
    const int32_t time = r0.x[2 * kTime] - 1;
    shift_history(r0, loc0, loc1, time);
    shift_history(r1, loc1, loc0, time);
    // checkDone (sim.cpp:114-151): double arithmetic, rounded to float once
    const int32_t gap = loc0 > loc1 ? loc0 - loc1 : loc1 - loc0;
    rew = (float)(loc0 == loc1 ? 1.0 : -gap * 0.2);
    bool over = false;
    if (loc0 < 0 || loc0 >= kSpaces || loc1 < 0 || loc1 >= kSpaces) {
        over = true;
        rew = (float)(-kSpaces * (time + 1) * 0.2);
    }
    return over || time == 0;
}

__device__ __forceinline__ void actions_of(const int32_t *action, uint32_t n, uint32_t w, bool sampled, uint64_t seed, uint32_t step, int32_t &a0, int32_t &a1)
{
    if (sampled) {  // uniform over the four moves, drawn here (include/mrl_envs.h: mrl_rollout_random)
        a0 = (int32_t)mrl::scale(mrl::policy_hash(seed, step, w, 0), 4u);
        a1 = (int32_t)mrl::scale(mrl::policy_hash(seed, step, w, 1), 4u);
    } else {
        a0 = action[w];
        a1 = action[(size_t)n + w];
    }
}

// workgroup b owns worlds [b*chunk, (b+1)*chunk), chunk a multiple of kBlock
__global__ void __launch_bounds__(kBlock) mrl_balance_step(uint32_t n, uint32_t chunk, const int32_t *action,  // (no __restrict__: mrl_rollout_random passes the ACTION tensor as action_out too)
                                                           int32_t *__restrict__ obs, float *__restrict__ reward,
                                                           int32_t *__restrict__ done, uint32_t *__restrict__ block_counts,
                                                           unsigned long long *__restrict__ finished_mask,
                                                           int32_t *action_out, uint64_t sample_seed, uint32_t sample_step)
{
    // Besides the int32 done flags of the DONE tensor every wave stores the ballot of its 64 flags as one word of
    // finished_mask (world w = bit w % 64 of word w / 64; chunk and kBlock are multiples of 64): the reset launch reads
    // those words -- 128 bytes per 1024 worlds -- instead of walking the flags round by round.
    __shared__ uint32_t s_wave[kBlock / 64];
    const uint32_t first = blockIdx.x * chunk, last = min(n, first + chunk);
    uint32_t finished = 0;  // wave-uniform
    for (uint32_t w0 = first; w0 < last; w0 += kBlock) {  // uniform trip count
        const uint32_t w = w0 + threadIdx.x;
        bool over = false;
        if (w < last) {
        Row r0 = load_row(obs, n, 0, w), r1 = load_row(obs, n, 1, w);
        int32_t a0, a1;
        actions_of(action, n, w, action_out != nullptr, sample_seed, sample_step, a0, a1);
        if (action_out) {
            action_out[w] = a0;
            action_out[(size_t)n + w] = a1;
        }
        float rew;
        over = move_world(r0, r1, a0, a1, rew);
        if (!over) {  // a finished world's rows come from the reset
            store_row(obs, n, 0, w, r0);
            store_row(obs, n, 1, w, r1);
        }
        reward[w] = rew;
        reward[(size_t)n + w] = rew;
        done[w] = over ? 1 : 0;
        }
        finished += mrl::note_finished(over, w, w < last, finished_mask);
    }
    mrl::post_wave_count(finished, s_wave);
    __syncthreads();
    mrl::store_block_count(s_wave, block_counts);
}

// The whole step in ONE launch (mrl_step on one GPU).  A third of the worlds finish in every step (episodes last at most
// three), so the two-launch pair writes a third of the rows twice over -- stepped rows it then skips, fresh rows as 28-byte
// pieces scattered by the re-seeding launch -- and that launch costs 15 us of the 36 at 1 M worlds.  Here workgroup b owns
// worlds [1024 b, 1024 b + 1024), four per thread in registers; a finished world's rows are replaced by the fresh episode's
// BEFORE they are stored, so every row is written exactly once, in the step's own coalesced stream.  Episode indices: the
// protocol of DESIGN.md 4.6 (rows are stored only behind the __syncthreads that makes the workgroup's own count globally visible).
constexpr int kFusedWorlds = 4;  // worlds per thread
__device__ __forceinline__ uint32_t recount_chunk(uint32_t n, const int32_t *action, const int32_t *obs, uint32_t j, bool sampled, uint64_t seed,
                                                   uint32_t step)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t first = j * (kFusedWorlds * kBlock), last = min(n, first + kFusedWorlds * kBlock);
    uint32_t count = 0;
    for (uint32_t w0 = first; w0 < last; w0 += 64u) {
        const uint32_t w = w0 + lane, wc = w < last ? w : first;
        Row r0 = load_row(obs, n, 0, wc), r1 = load_row(obs, n, 1, wc);
        int32_t a0, a1;
        actions_of(action, n, wc, sampled, seed, step, a0, a1);
        float rew;
        const bool over = move_world(r0, r1, a0, a1, rew) && w < last;
        count += (uint32_t)__popcll(__ballot(over));
    }
    return count;
}

// kStats (mrl_enable_episode_stats): the lane also keeps its four worlds' episode returns (both players receive the same
// reward) and step counts -- loaded with the rows, stored with reward and done -- and thread 0 adds the workgroup's
// finished episodes to TOTALS block b behind one more LDS barrier (episode_stats.hpp).  Without it the kernel is what it was.
template <bool kStats>
__global__ void __launch_bounds__(kBlock) mrl_balance_step_fused(uint32_t n, const int32_t *action, int32_t *__restrict__ obs,
                                                                 float *__restrict__ reward, int32_t *__restrict__ done,
                                                                 uint32_t *status, unsigned long long *group_total, uint32_t epoch,
                                                                 const uint32_t *episode_base,
                                                                 uint32_t *next_counter, uint32_t *__restrict__ reset_count, int32_t *action_out,
                                                                 uint64_t sample_seed, uint32_t sample_step, const mrl::HealTest heal,
                                                                 const mrl::DeviceCounter device_counter,
                                                                 const mrl::FusedExchange fx,  // sharded batch: the other ranks' counts (episode_scan.hpp)
                                                                 const mrl::StatsArg<kStats> stats)
{
    __shared__ uint32_t s_wave[kFusedWorlds][kBlock / 64];
    __shared__ mrl::EpisodeNumbers s_numbers;
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t first = b * (kFusedWorlds * kBlock), last = min(n, first + kFusedWorlds * kBlock);
    const bool last_block = b == gridDim.x - 1, sampled = action_out != nullptr;
    device_counter.apply(episode_base, next_counter, epoch);  // (the launch state may live in device memory: common.hpp)
    mrl::heal_test_delay(heal, b, gridDim.x, epoch);          // test hook only
    const uint32_t base = *episode_base;
    Row r0[kFusedWorlds], r1[kFusedWorlds];
    float rew[kFusedWorlds];
    bool over[kFusedWorlds];
    uint32_t rank[kFusedWorlds];  // among the workgroup's finished worlds, in ascending world order (round u covers worlds first + 256 u ...)
    using Stats = mrl::StatsWorlds<2>;
    [[maybe_unused]] Stats tally;
    [[maybe_unused]] typename Stats::World running[kFusedWorlds];
#pragma unroll
    for (int u = 0; u < kFusedWorlds; u++) {
        const uint32_t w = first + u * kBlock + threadIdx.x, wc = w < last ? w : first;
        r0[u] = load_row(obs, n, 0, wc);
        r1[u] = load_row(obs, n, 1, wc);
        if constexpr (kStats) running[u] = Stats::load(stats, wc);
        int32_t a0, a1;
        actions_of(action, n, wc, sampled, sample_seed, sample_step, a0, a1);
        if (sampled && w < last) {
            action_out[w] = a0;
            action_out[(size_t)n + w] = a1;
        }
        over[u] = move_world(r0[u], r1[u], a0, a1, rew[u]) && w < last;
        rank[u] = mrl::cast_vote(over[u], s_wave[u]);
    }
    __syncthreads();
    const uint32_t block_total = mrl::tally_votes<kFusedWorlds, kBlock>(s_wave, rank);
    if (threadIdx.x == 0) mrl::publish_count(status, b, epoch, block_total);
    __syncthreads();  // the count is globally visible (vmcnt(0) in front of the barrier) before any row of this workgroup changes
    const bool needs_prefix = block_total != 0 || last_block;
    if (threadIdx.x < 64)  // (a workgroup that closes a group of 256 looks back whatever its count)
        mrl::fused_lookback(s_numbers, status, group_total, epoch, block_total, needs_prefix, heal, fx, [&](uint32_t j) {
            return recount_chunk(n, action, obs, j, sampled, sample_seed, sample_step);
        });
    mrl::lds_barrier();
    const uint32_t own_before = needs_prefix ? s_numbers.own_before : 0u;
    const uint32_t before = own_before + (needs_prefix ? s_numbers.lower_ranks : 0u);
    // (Storing the rows of the worlds that go on while the look-back is under way, and the fresh rows behind it, was measured:
    // 32.6 against 30.4 us per step at 1 M worlds -- the 28-byte rows of neighbouring worlds share cache lines, and writing a
    // line in two passes costs more than the 2 us of waiting.)
#pragma unroll
    for (int u = 0; u < kFusedWorlds; u++) {
        const uint32_t w = first + u * kBlock + threadIdx.x;
        if (w < last) {
            if (over[u]) fresh_rows(base + before + rank[u], r0[u], r1[u]);  // the finished world's next episode, stored in its place
            store_row(obs, n, 0, w, r0[u]);
            store_row(obs, n, 1, w, r1[u]);
            reward[w] = rew[u];
            reward[(size_t)n + w] = rew[u];
            done[w] = over[u] ? 1 : 0;
            if constexpr (kStats) tally.finish(stats, w, running[u], rew[u], over[u]);
        }
    }
    if constexpr (kStats) {
        if (block_total != 0) {  // uniform per workgroup
            __shared__ double s_stats[kBlock / 64][3];
            tally.to_lds(&s_stats[0][0], wave, lane);
            mrl::lds_barrier();
            if (threadIdx.x == 0) Stats::add_totals(stats, &s_stats[0][0], kBlock / 64, b, block_total);
        }
    }
    if (last_block && threadIdx.x == 0) mrl::close_step(own_before, block_total, base, s_numbers.all_counts, reset_count, next_counter);
}

struct BalanceSim final : mrl::EpisodeSim {
    int32_t *obs = nullptr, *done = nullptr, *world_id = nullptr, *agent_id = nullptr, *active = nullptr, *mask = nullptr;
    float *reward = nullptr;

    void launch_fused(const int32_t *actions, const Drawn &drawn, const mrl::FusedExchange &fx, const Counters &c, hipStream_t stream) override
    {
        single_launch(mrl_balance_step_fused<true>, mrl_balance_step_fused<false>, kBlock, stream, num_worlds, actions ? actions : action, obs,
                      reward, done, status, group_total, epoch, c.base, c.next, reset_count, drawn.action_out, drawn.seed, drawn.step, heal, c.device,
                      fx)();
    }
    void launch_step(const int32_t *actions, int32_t *action_out, uint64_t seed, uint32_t sample_step, hipStream_t stream) override
    {
        hipLaunchKernelGGL(mrl_balance_step, dim3(grid), dim3(kBlock), 0, stream, num_worlds, chunk, actions ? actions : action, obs, reward,
                           done, block_counts, stepped.words, action_out, seed, sample_step);
        MRL_HIP(hipGetLastError());
    }
    void phase1(const int32_t *actions, hipStream_t stream) override { launch_step(actions, nullptr, 0, 0, stream); }
    void launch_reseed(const Finished &from, const mrl::GatheredCounts &gathered, const Counters &c, hipStream_t stream) override
    {
        hipLaunchKernelGGL((mrl::reseed_finished<kBlock, BalanceReseed>), dim3(grid), dim3(kBlock), 0, stream, num_worlds, chunk,
                           BalanceReseed{obs, num_worlds}, from.block_counts, from.words, c.base, c.next, from.reset_count, gathered, c.device);
    }
    void reseed_shard(uint32_t world_offset, uint32_t num_worlds_total, hipStream_t stream) override
    {
        hipLaunchKernelGGL(mrl::reseed_all<BalanceReseed>, dim3((num_worlds + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, num_worlds,
                           world_offset, BalanceReseed{obs, num_worlds});
        MRL_HIP(hipGetLastError());
        MRL_HIP(hipMemsetAsync(done, 0, sizeof(int32_t) * num_worlds, stream));
        MRL_HIP(hipMemsetAsync(reward, 0, sizeof(float) * 2 * num_worlds, stream));
        set_episode_counter(num_worlds_total, stream);
    }

    bool tensor(int slot, mrl_tensor_desc *out) override
    {
        const int64_t N = num_worlds;
        switch (slot) {
        case MRL_BALANCE_DONE: *out = mrl::make_desc(done, MRL_INT32, device, {N}); return true;
        case MRL_BALANCE_ACTIVE_AGENT: *out = mrl::make_desc(active, MRL_INT32, device, {2, N}); return true;
        case MRL_BALANCE_ACTION: *out = mrl::make_desc(action, MRL_INT32, device, {2, N, 1}); return true;
        case MRL_BALANCE_OBSERVATION: *out = mrl::make_desc(obs, MRL_INT32, device, {2, N, kRow}); return true;
        case MRL_BALANCE_ACTION_MASK: *out = mrl::make_desc(mask, MRL_INT32, device, {2, N, 4}); return true;
        case MRL_BALANCE_REWARD: *out = mrl::make_desc(reward, MRL_FLOAT32, device, {2, N}); return true;
        case MRL_BALANCE_WORLD_ID: *out = mrl::make_desc(world_id, MRL_INT32, device, {2, N}); return true;
        case MRL_BALANCE_AGENT_ID: *out = mrl::make_desc(agent_id, MRL_INT32, device, {2, N}); return true;
        case MRL_BALANCE_RESET_COUNT: *out = mrl::make_desc(reset_count, MRL_UINT32, device, {1}); return true;
        case MRL_BALANCE_SHARD_COUNT: *out = mrl::make_desc(shard_count, MRL_UINT32, device, {1}); return true;
        default: return false;
        }
    }
    size_t action_elems() const override { return (size_t)2 * num_worlds; }
    const char *kernel_name() const override { return fused ? "mrl_balance_step_fused" : "mrl_balance_step"; }
    // actions 8 + both agents' rows r/w 2 * 2 * 28 + reward 8 + done 4
    uint64_t bytes_per_world_step() const override { return 8 + 4 * kRow * 4 + 8 + 4; }
    void launch_shape(uint32_t out[4]) const override
    {
        out[0] = grid;
        out[1] = kBlock;
        out[2] = out[3] = 0;
    }
};

}  // namespace

mrl_sim *mrl::create_balance(int gpu_id, uint32_t num_worlds)
{
    return create_episode_sim<BalanceSim>("balance", MRL_GAME_BALANCE, gpu_id, num_worlds, [&](BalanceSim *sim) {
        sim->size_scan_grid(kBlock);
        const size_t N = num_worlds;
        sim->action = sim->arena.alloc<int32_t>(2 * N);
        sim->obs = sim->arena.alloc<int32_t>(2 * N * kRow);
        sim->done = sim->arena.alloc<int32_t>(N);
        sim->reward = sim->arena.alloc<float>(2 * N);
        sim->world_id = sim->arena.alloc<int32_t>(2 * N, false);
        sim->agent_id = sim->arena.alloc<int32_t>(2 * N, false);
        sim->active = sim->arena.alloc<int32_t>(2 * N, false);
        sim->mask = sim->arena.alloc<int32_t>(2 * N * 4, false);
        sim->alloc_episode(true, false);
        sim->launch_state.init(sim->arena);
        sim->alarm.init(sim->arena);
        sim->alloc_fused(kFusedWorlds * kBlock);
        sim->read_step_knobs(sim->fused_grid != 0, sim->fused_grid);  // one launch: every row written once
        mrl::fill_ids(sim->world_id, sim->agent_id, 2, num_worlds);
        mrl::fill_i32(sim->active, 1, 2 * N);
        mrl::fill_i32(sim->mask, 1, 2 * N * 4);
        sim->reseed_shard(0, num_worlds, 0);  // Sim::Sim (sim.cpp:173-202): world w starts as episode w
    });
}
