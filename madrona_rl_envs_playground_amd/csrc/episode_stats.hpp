// Episode returns and lengths kept on the device (mrl_enable_episode_stats, include/mrl_envs.h).
// Host side: the five tensors, which live in ONE allocation of their own made when the caller enables them -- behind
// and outside everything a simulator's arena holds, so no existing tensor moves (episode_host.hpp on what a moved word
// costs) -- and the launches of episode_stats.hip; device side: what the single-launch steps of the three one-lane-per-world games
// do in their own kernels instead of that launch.
#pragma once

#include "common.hpp"

#include <type_traits>

namespace mrl {

constexpr uint32_t kStatsBlockWorlds = 1024;  // worlds per TOTALS block = per workgroup of the update launch

// ---- device side of the statistics taken INSIDE a single-launch step (Cartpole, Acrobot, balance beam) ----
// Those workgroups own exactly the 1024 worlds of a TOTALS block, and the lane that holds a world's reward and done flag
// in registers keeps the world's return and step count as well: no second launch.  Everything here is private to the
// workgroup (its own worlds' values, its own TOTALS block), so none of the look-back's ordering rules apply to it.
// The five tensors share one allocation, each on a 256-byte boundary: EPISODE_RETURN, LAST_RETURN (`players` rows of n
// floats), EPISODE_STEPS, LAST_STEPS (n words), TOTALS.  A kernel is handed the base alone and works the rest out when it
// gets there -- three scalar registers instead of eleven held across a transition that has none to spare (Acrobot's).
struct StatsLane {
    char *base;
    uint32_t n, players;
    __host__ __device__ static size_t up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
    __host__ __device__ size_t per_player() const { return up(sizeof(float) * (size_t)players * n); }
    __host__ __device__ size_t per_world() const { return up(sizeof(int32_t) * (size_t)n); }
    __host__ __device__ float *ret() const { return reinterpret_cast<float *>(base); }
    __host__ __device__ float *last_ret() const { return reinterpret_cast<float *>(base + per_player()); }
    __host__ __device__ int32_t *steps() const { return reinterpret_cast<int32_t *>(base + 2 * per_player()); }
    __host__ __device__ int32_t *last_steps() const { return reinterpret_cast<int32_t *>(base + 2 * per_player() + per_world()); }
    __host__ __device__ double *totals() const { return reinterpret_cast<double *>(base + 2 * per_player() + 2 * per_world()); }
};
struct NoStats {};
// the trailing argument of a step kernel with a `bool kStats` template parameter
template <bool kStats> using StatsArg = std::conditional_t<kStats, StatsLane, NoStats>;

__device__ __forceinline__ double stats_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);  // a fixed tree: the same order every run
    return v;
}

// One lane's worlds.  load() early, with the step's own loads; finish() where the step stores the world's reward and done
// flag; then, outside divergent code, to_lds() and -- behind a barrier -- add_totals() by one thread.
template <int kPlayers> struct StatsWorlds {
    double step_sum = 0., ret_sum[kPlayers] = {};

    struct World {
        int32_t steps;
        float ret[kPlayers];
    };
    // w: in bounds (the caller clamps)
    __device__ __forceinline__ static World load(const StatsLane &st, uint32_t w)
    {
        World v;
        v.steps = st.steps()[w];
#pragma unroll
        for (int p = 0; p < kPlayers; p++) v.ret[p] = st.ret()[(size_t)p * st.n + w];
        return v;
    }
    // the definition in include/mrl_envs.h for world w < n, which received `reward` (all players the same: the three games'
    // rewards are) and finished or not
    __device__ __forceinline__ void finish(const StatsLane &st, uint32_t w, World v, float reward, bool over)
    {
        int32_t steps = v.steps + 1;
#pragma unroll
        for (int p = 0; p < kPlayers; p++) {
            float r = v.ret[p] + reward;
            if (over) {
                st.last_ret()[(size_t)p * st.n + w] = r;
                ret_sum[p] += (double)r;
                r = 0.f;
            }
            st.ret()[(size_t)p * st.n + w] = r;
        }
        if (over) {
            st.last_steps()[w] = steps;
            step_sum += (double)steps;
            steps = 0;
        }
        st.steps()[w] = steps;
    }
    // s_sums: [waves][1 + kPlayers] doubles in LDS; every lane of the wave calls it
    __device__ __forceinline__ void to_lds(double *s_sums, uint32_t wave, uint32_t lane)
    {
        const double steps = stats_wave_sum(step_sum);
        if (lane == 0) s_sums[wave * (1 + kPlayers)] = steps;
#pragma unroll
        for (int p = 0; p < kPlayers; p++) {
            const double r = stats_wave_sum(ret_sum[p]);
            if (lane == 0) s_sums[wave * (1 + kPlayers) + 1 + p] = r;
        }
    }
    // ONE thread of the workgroup, behind a barrier after to_lds, and only if a world of the workgroup finished
    __device__ __forceinline__ static void add_totals(const StatsLane &st, const double *s_sums, uint32_t waves, uint32_t block, uint32_t finished)
    {
        double *row = st.totals() + (size_t)block * (2 + kPlayers);
        row[0] += (double)finished;
        for (int c = 0; c < 1 + kPlayers; c++) {
            double sum = 0.;
            for (uint32_t w = 0; w < waves; w++) sum += s_sums[w * (1 + kPlayers) + c];
            row[1 + c] += sum;
        }
    }
};

struct EpisodeStats {
    uint32_t num_worlds = 0, players = 0, blocks = 0;
    int device = 0;
    // what the update launch reads: the game's own REWARD (int32 or float32, `players` rows of num_worlds) and DONE
    mrl_tensor_desc reward{}, done{};
    void *block = nullptr;  // the one allocation
    float *ret = nullptr, *last_ret = nullptr;
    int32_t *steps = nullptr, *last_steps = nullptr;
    double *totals = nullptr;  // (blocks, 2 + players): episodes, their steps, their return per player

    ~EpisodeStats()
    {
        if (block) (void)hipFree(block);
    }
    size_t totals_bytes() const { return sizeof(double) * blocks * (2 + (size_t)players); }
    // allocates and zeroes; synchronises the stream
    void init(mrl_sim *sim, hipStream_t stream);
    // one launch behind a completed step: the definition in include/mrl_envs.h
    void update(hipStream_t stream) const;
    // mrl_reset_worlds / mrl_reseed_shard: running values of the masked worlds (nullptr: all) -> 0
    void clear_running(const uint8_t *mask_dev, hipStream_t stream) const;
    void clear_totals(hipStream_t stream) const { MRL_HIP(hipMemsetAsync(totals, 0, totals_bytes(), stream)); }
    bool tensor(int slot, mrl_tensor_desc *out) const;
    StatsLane lane() const { return StatsLane{static_cast<char *>(block), num_worlds, players}; }
};

}  // namespace mrl
