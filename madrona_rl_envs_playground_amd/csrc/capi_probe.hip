// mrl_probe_stream (include/mrl_envs.h) and its two kernels: the only device code of the C API's own files.
#include "capi_internal.hpp"

#include <algorithm>

namespace mrl {

// ---- roofline.peak_measured of bench.py: float4 streams over caller buffers ----
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int kMode>
__global__ void __launch_bounds__(256) mrl_probe_stream_kernel(f32x4 *__restrict__ dst, const f32x4 *__restrict__ src, size_t chunks)
{
    // every workgroup streams through ONE contiguous range (like a wave of the step kernels writing its group's
    // slab): 4 x 4 KB in flight per workgroup and trip
    const size_t per_block = (chunks + gridDim.x - 1) / gridDim.x;
    const size_t first = (size_t)blockIdx.x * per_block, last = first + per_block < chunks ? first + per_block : chunks;
    const f32x4 fill = {1.f, 2.f, 3.f, 4.f};
    size_t i = first + threadIdx.x;
    for (; i + 3 * 256 < last; i += 4 * 256) {
        f32x4 a = fill, b = fill, c = fill, d = fill;
        if (kMode == 0) {
            a = src[i];
            b = src[i + 256];
            c = src[i + 512];
            d = src[i + 768];
        }
        if (kMode == 2) {  // write-through, like the observation stores of the step kernels
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i), "v"(a) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i + 256), "v"(b) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i + 512), "v"(c) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(dst + i + 768), "v"(d) : "memory");
        } else {
            dst[i] = a;
            dst[i + 256] = b;
            dst[i + 512] = c;
            dst[i + 768] = d;
        }
    }
    for (; i < last; i += 256) dst[i] = kMode == 0 ? src[i] : fill;
}

// Modes 3 / 4: the bytes and stores of mode 2 in TWO passes inside one launch.  The first pass stores the aligned
// kBlockBytes blocks (64 / 128) of a fixed pseudo-random quarter of the block indices, the second pass the rest -- what a
// step kernel does when it sends the blocks that cannot change ahead of the others.  Asks whether two halves of a
// 128-byte line that reach the L2 at different times cost more than the line written at once.
template <int kBlockBytes>
__global__ void __launch_bounds__(256) mrl_probe_stream_two_pass_kernel(f32x4 *__restrict__ dst, size_t chunks)
{
    const size_t per_block = (chunks + gridDim.x - 1) / gridDim.x;
    const size_t first = (size_t)blockIdx.x * per_block, last = first + per_block < chunks ? first + per_block : chunks;
    const f32x4 fill = {1.f, 2.f, 3.f, 4.f};
    constexpr int kShift = kBlockBytes == 64 ? 2 : 3;  // 16-byte chunks per block
    for (int pass = 0; pass < 2; pass++) {
        for (size_t i = first + threadIdx.x; i < last; i += 256) {
            const bool early = (((uint32_t)(i >> kShift) * 2654435761u) >> 30) == 0u;
            if (early == (pass == 0)) asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i), "v"(fill) : "memory");
        }
    }
}

}  // namespace mrl

using mrl::guarded;

extern "C" {

int mrl_probe_stream(void *dst_dev, const void *src_dev, uint64_t bytes, int mode, int gpu_id, void *hip_stream)
{
    if (!dst_dev || (mode == 0 && !src_dev) || mode < 0 || mode > 4 || bytes < 16 || (bytes & 15u) ||
        (reinterpret_cast<uintptr_t>(dst_dev) & 15u) || (reinterpret_cast<uintptr_t>(src_dev) & 15u)) {
        mrl::set_error("mrl_probe_stream: need 16-byte aligned device buffers, a multiple of 16 bytes and mode 0..4");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        const size_t chunks = bytes / 16;
        const unsigned grid = (unsigned)std::min<size_t>((chunks + 1023) / 1024, 256 * 32);
        auto *dst = static_cast<mrl::f32x4 *>(dst_dev);
        auto *src = static_cast<const mrl::f32x4 *>(src_dev);
        hipStream_t stream = (hipStream_t)hip_stream;
        if (mode == 0)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<0>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 1)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<1>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 2)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<2>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 3)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_two_pass_kernel<64>), dim3(grid), dim3(256), 0, stream, dst, chunks);
        else
            hipLaunchKernelGGL((mrl::mrl_probe_stream_two_pass_kernel<128>), dim3(grid), dim3(256), 0, stream, dst, chunks);
        MRL_HIP(hipGetLastError());
    });
}

}  // extern "C"
