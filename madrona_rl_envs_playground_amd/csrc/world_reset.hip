// The kernels of mrl_reset_worlds (world_reset.hpp says how they are used), and the two fill kernels behind the
// simulators' constant tensors.
#include "episode_scan.hpp"
#include "kitchen_host.hpp"

namespace {

// One workgroup per workgroup of the phase-2 grid (worlds [b * chunk, (b + 1) * chunk)); mask == nullptr: every world.
// words: world i is bit i % 64 of words[i / 64] (chunk a multiple of 64); flags: 1 / 0 per world; either may be null.
__global__ void __launch_bounds__(256) mrl_reset_mask_counts(const uint8_t *__restrict__ mask, uint32_t n, uint32_t chunk,
                                                             unsigned long long *__restrict__ words, int32_t *__restrict__ flags,
                                                             uint32_t *__restrict__ block_counts)
{
    __shared__ uint32_t s_wave[4];
    const uint32_t first = blockIdx.x * chunk, last = min(n, first + chunk);
    uint32_t count = 0;  // wave-uniform
    for (uint32_t i0 = first; i0 < last; i0 += 256) {  // uniform trip count
        const uint32_t i = i0 + threadIdx.x;
        const bool on = i < last && (!mask || mask[i] != 0);
        if (flags && i < last) flags[i] = on ? 1 : 0;
        count += mrl::note_finished(on, i, words && i < last, words);
    }
    mrl::post_wave_count(count, s_wave);
    __syncthreads();
    mrl::store_block_count(s_wave, block_counts);
}

// One wavefront per world; a world outside the mask costs the load of its mask byte.
__global__ void __launch_bounds__(256) mrl_cooked_reset(const uint8_t *__restrict__ mask, uint32_t n, const mrl::FreshWorld f)
{
    const uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (w >= n || (mask && mask[w] == 0)) return;  // wave-uniform
    for (int k = 0; k < mrl::FreshWorld::kArrays; k++)
        for (uint32_t j = lane; j < f.words[k]; j += 64) f.dst[k][(size_t)w * f.words[k] + j] = f.src[k][j];
    uint8_t *slab = f.obs + (size_t)w * f.obs_bytes;
    if (f.obs_grain == 16) {
        for (uint32_t j = lane; j < f.obs_bytes / 16; j += 64) reinterpret_cast<uint4 *>(slab)[j] = reinterpret_cast<const uint4 *>(f.obs_src)[j];
    } else if (f.obs_grain == 4) {
        for (uint32_t j = lane; j < f.obs_bytes / 4; j += 64) reinterpret_cast<uint32_t *>(slab)[j] = reinterpret_cast<const uint32_t *>(f.obs_src)[j];
    } else {
        for (uint32_t j = lane; j < f.obs_bytes; j += 64) slab[j] = f.obs_src[j];
    }
}

__global__ void mrl_fill_ids(int32_t *world_id, int32_t *row_id, uint32_t rows, uint32_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)rows * n) {
        world_id[i] = (int32_t)(i % n);
        if (row_id) row_id[i] = (int32_t)(i / n);
    }
}

__global__ void mrl_fill_i32(int32_t *dst, int32_t value, size_t count)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = value;
}

}  // namespace

void mrl::fill_ids(int32_t *world_id, int32_t *row_id, uint32_t rows, uint32_t n)
{
    const size_t count = (size_t)rows * n;
    hipLaunchKernelGGL(mrl_fill_ids, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, world_id, row_id, rows, n);
    MRL_HIP(hipGetLastError());
}

void mrl::fill_i32(int32_t *dst, int32_t value, size_t count)
{
    hipLaunchKernelGGL(mrl_fill_i32, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, dst, value, count);
    MRL_HIP(hipGetLastError());
}

void mrl::ResetScratch::build(const uint8_t *mask_dev, uint32_t n, uint32_t grid, uint32_t chunk, hipStream_t stream) const
{
    hipLaunchKernelGGL(mrl_reset_mask_counts, dim3(grid), dim3(256), 0, stream, mask_dev, n, chunk, words, flags, block_counts);
    MRL_HIP(hipGetLastError());
}

void mrl::FreshWorldOwner::init(DeviceArena &arena, std::initializer_list<std::pair<uint32_t *, uint32_t>> arrays, const uint8_t *obs,
                                uint32_t obs_bytes)
{
    size_t state_words = 0;
    for (const auto &a : arrays) state_words += a.second;
    state_words = (state_words + 3) & ~(size_t)3;  // the slab behind the state starts on a 16-byte boundary
    uint32_t *copy = arena.alloc<uint32_t>(state_words + (obs_bytes + 15u) / 16u * 4u, false);
    int k = 0;
    size_t at = 0;
    for (const auto &a : arrays) {
        f.dst[k] = a.first;
        f.src[k] = copy + at;
        f.words[k] = a.second;
        MRL_HIP(hipMemcpy(copy + at, a.first, sizeof(uint32_t) * a.second, hipMemcpyDeviceToDevice));
        at += a.second;
        k++;
    }
    uint8_t *slab = reinterpret_cast<uint8_t *>(copy + state_words);
    MRL_HIP(hipMemcpy(slab, obs, obs_bytes, hipMemcpyDeviceToDevice));
    f.obs_src = slab;
    f.obs_bytes = obs_bytes;
}

void mrl::FreshWorldOwner::launch(const uint8_t *mask_dev, uint32_t n, uint8_t *obs_dest, hipStream_t stream) const
{
    FreshWorld g = f;
    g.obs = obs_dest;
    const uintptr_t both = reinterpret_cast<uintptr_t>(obs_dest) | (uintptr_t)f.obs_bytes;
    g.obs_grain = (both & 15u) == 0 ? 16u : ((both & 3u) == 0 ? 4u : 1u);
    hipLaunchKernelGGL(mrl_cooked_reset, dim3((n + 3u) / 4u), dim3(256), 0, stream, mask_dev, n, g);
    MRL_HIP(hipGetLastError());
}
