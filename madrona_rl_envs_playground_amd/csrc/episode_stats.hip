// Episode returns and lengths as a product of the step (mrl_enable_episode_stats, include/mrl_envs.h): the general
// launch that runs behind a completed step of any game, and the one that clears the running values of chosen worlds.
#include "episode_stats.hpp"

#include <stdexcept>

namespace mrl {
namespace {

constexpr int kStatsBlock = 256, kStatsUnroll = 4;  // 256 threads x 4 worlds: workgroup b is TOTALS block b
constexpr int kStatsMaxPlayers = 64;                // Overcooked's limit, the largest of the six games
static_assert(kStatsBlock * kStatsUnroll == (int)kStatsBlockWorlds, "one workgroup per TOTALS block");

// Thread t of workgroup b owns worlds 1024 b + 256 u + t, u = 0..3.  Per world: one more step, reward added to the return
// (one float32 add per player), and for a finished world LAST_* written and the running values zeroed.  What the
// finished worlds of the workgroup add to TOTALS block b is summed inside the workgroup in a fixed order -- lane's four
// worlds, shuffle tree per wave, the four waves through LDS -- and added by ONE thread per column: no atomics, and
// nothing at all for a workgroup without a finished world.
template <typename R>
__global__ void __launch_bounds__(kStatsBlock) mrl_episode_stats_update(uint32_t n, uint32_t players, const R *__restrict__ reward,
                                                                        const int32_t *__restrict__ done, float *__restrict__ ret,
                                                                        int32_t *__restrict__ steps, float *__restrict__ last_ret,
                                                                        int32_t *__restrict__ last_steps, double *__restrict__ totals)
{
    __shared__ double s_red[kStatsBlock / 64][2 + kStatsMaxPlayers];
    const uint32_t first = blockIdx.x * kStatsBlockWorlds;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool fin[kStatsUnroll];
    double count = 0., step_sum = 0.;
#pragma unroll
    for (int u = 0; u < kStatsUnroll; u++) {
        const uint32_t w = first + u * kStatsBlock + threadIdx.x;
        fin[u] = false;
        if (w < n) {
            fin[u] = done[w] != 0;
            int32_t st = steps[w] + 1;
            if (fin[u]) {
                last_steps[w] = st;
                count += 1.;
                step_sum += (double)st;
                st = 0;
            }
            steps[w] = st;
        }
    }
    count = stats_wave_sum(count);
    step_sum = stats_wave_sum(step_sum);
    if (lane == 0) {
        s_red[wave][0] = count;
        s_red[wave][1] = step_sum;
    }
    __syncthreads();
    double finished = 0.;
    for (int w = 0; w < kStatsBlock / 64; w++) finished += s_red[w][0];
    const bool any = finished != 0.;  // uniform per workgroup
    for (uint32_t p = 0; p < players; p++) {
        const size_t row = (size_t)p * n;
        double ret_sum = 0.;
#pragma unroll
        for (int u = 0; u < kStatsUnroll; u++) {
            const uint32_t w = first + u * kStatsBlock + threadIdx.x;
            if (w < n) {
                float r = ret[row + w] + (float)reward[row + w];
                if (fin[u]) {
                    last_ret[row + w] = r;
                    ret_sum += (double)r;
                    r = 0.f;
                }
                ret[row + w] = r;
            }
        }
        if (any) {
            ret_sum = stats_wave_sum(ret_sum);
            if (lane == 0) s_red[wave][2 + p] = ret_sum;
        }
    }
    if (!any) return;
    __syncthreads();
    const uint32_t columns = 2 + players;
    if (threadIdx.x < columns) {
        double sum = 0.;
        for (int w = 0; w < kStatsBlock / 64; w++) sum += s_red[w][threadIdx.x];
        totals[(size_t)blockIdx.x * columns + threadIdx.x] += sum;
    }
}

__global__ void mrl_episode_stats_clear(uint32_t n, uint32_t players, const uint8_t *__restrict__ mask, float *__restrict__ ret,
                                        int32_t *__restrict__ steps)
{
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n || (mask && !mask[w])) return;
    steps[w] = 0;
    for (uint32_t p = 0; p < players; p++) ret[(size_t)p * n + w] = 0.f;
}

bool contiguous(const mrl_tensor_desc &d)
{
    int64_t run = 1;
    for (int k = d.ndim - 1; k >= 0; k--) {
        if (d.shape[k] != 1 && d.strides[k] != run) return false;
        run *= d.shape[k];
    }
    return true;
}

int64_t numel(const mrl_tensor_desc &d)
{
    int64_t count = 1;
    for (int k = 0; k < d.ndim; k++) count *= d.shape[k];
    return count;
}

}  // namespace

void EpisodeStats::init(mrl_sim *sim, hipStream_t stream)
{
    // REWARD and DONE sit in the same slots of a game's list as in the reference's ExportID
    const bool one_lane = sim->game == MRL_GAME_CARTPOLE || sim->game == MRL_GAME_ACROBOT;
    if (!sim->tensor(one_lane ? MRL_CARTPOLE_REWARD : MRL_OVERCOOKED_REWARD, &reward) || !sim->tensor(MRL_OVERCOOKED_DONE, &done))
        throw std::runtime_error("mrl_enable_episode_stats: the game exports no REWARD / DONE tensor");
    num_worlds = sim->num_worlds;
    device = sim->device;
    const int64_t elems = numel(reward);
    if ((reward.dtype != MRL_INT32 && reward.dtype != MRL_FLOAT32) || done.dtype != MRL_INT32 || !contiguous(reward) || !contiguous(done) ||
        numel(done) != (int64_t)num_worlds || elems % num_worlds != 0 || elems / num_worlds < 1 || elems / num_worlds > kStatsMaxPlayers)
        throw std::runtime_error("mrl_enable_episode_stats: unexpected REWARD / DONE layout");
    players = (uint32_t)(elems / num_worlds);
    blocks = (num_worlds + kStatsBlockWorlds - 1) / kStatsBlockWorlds;
    // one allocation, every tensor on a 256-byte boundary (the layout is StatsLane's)
    const StatsLane shape{nullptr, num_worlds, players};
    const size_t bytes = 2 * shape.per_player() + 2 * shape.per_world() + StatsLane::up(totals_bytes());
    MRL_HIP(hipMalloc(&block, bytes));
    const StatsLane at = lane();
    ret = at.ret();
    last_ret = at.last_ret();
    steps = at.steps();
    last_steps = at.last_steps();
    totals = at.totals();
    MRL_HIP(hipMemsetAsync(block, 0, bytes, stream));
    MRL_HIP(hipStreamSynchronize(stream));
}

void EpisodeStats::update(hipStream_t stream) const
{
    if (reward.dtype == MRL_INT32)
        hipLaunchKernelGGL(mrl_episode_stats_update<int32_t>, dim3(blocks), dim3(kStatsBlock), 0, stream, num_worlds, players,
                           static_cast<const int32_t *>(reward.data), static_cast<const int32_t *>(done.data), ret, steps, last_ret, last_steps,
                           totals);
    else
        hipLaunchKernelGGL(mrl_episode_stats_update<float>, dim3(blocks), dim3(kStatsBlock), 0, stream, num_worlds, players,
                           static_cast<const float *>(reward.data), static_cast<const int32_t *>(done.data), ret, steps, last_ret, last_steps,
                           totals);
    MRL_HIP(hipGetLastError());
}

void EpisodeStats::clear_running(const uint8_t *mask_dev, hipStream_t stream) const
{
    hipLaunchKernelGGL(mrl_episode_stats_clear, dim3((num_worlds + 255) / 256), dim3(256), 0, stream, num_worlds, players, mask_dev, ret, steps);
    MRL_HIP(hipGetLastError());
}

bool EpisodeStats::tensor(int slot, mrl_tensor_desc *out) const
{
    const auto shaped = [&](void *data, int dtype, const mrl_tensor_desc &like) {
        mrl_tensor_desc d = like;  // the shape (and the contiguous strides) of the game's own tensor
        d.data = data;
        d.dtype = dtype;
        return d;
    };
    switch (slot) {
    case MRL_STATS_EPISODE_RETURN: *out = shaped(ret, MRL_FLOAT32, reward); return true;
    case MRL_STATS_EPISODE_STEPS: *out = shaped(steps, MRL_INT32, done); return true;
    case MRL_STATS_LAST_RETURN: *out = shaped(last_ret, MRL_FLOAT32, reward); return true;
    case MRL_STATS_LAST_STEPS: *out = shaped(last_steps, MRL_INT32, done); return true;
    case MRL_STATS_TOTALS: *out = make_desc(totals, MRL_FLOAT64, device, {(int64_t)blocks, 2 + (int64_t)players}); return true;
    default: return false;
    }
}

void episode_stats_destroy(EpisodeStats *stats) { delete stats; }

}  // namespace mrl
