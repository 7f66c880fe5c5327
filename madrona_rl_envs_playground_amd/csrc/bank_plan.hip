// Every bank's plan of an act and, at the end, every bank's resample (bank_plan.hpp has the workspace; DESIGN.md sections 19 to 21).
//
// A cell s = n P + p is acted when seat p is in `players` and 0 <= ids[s] < K.  Pass one counts the acted cells of every policy,
// chunks of 1024 cells at a time (a wave finds its distinct ids with ballots, one integer LDS add per id and wave); the counts
// become list starts and tile starts, and the tile table is filled a tile per thread by a search in the tile starts; pass two
// places every acted cell at start[k] + (cells of k in earlier chunks, waves and lanes): the lists are in ascending s on every
// run, whatever the timing.  Up to 2048 cells it is ONE workgroup of 1024 threads, mrl_bank_plan; beyond, where one workgroup's
// walk over the chunks would cost more than the act, three launches: a workgroup per chunk counts (mrl_bank_plan_count), one
// workgroup adds the chunks up and writes the table (mrl_bank_plan_scan), a workgroup per chunk places (mrl_bank_plan_place).
// No workgroup waits for another inside a kernel.  Integer atomics in LDS only, no float atomics, no scratch.
#include "bank_plan.hpp"
#include "random_policy.hpp"

namespace mrl {

// cell s of the call: its id, whether it is acted (valid) and whether its id lies beyond the bank on a seat of the mask
__device__ __forceinline__ void plan_cell(const BankPlanArgs &a, uint32_t s, int32_t &id, bool &valid, bool &beyond)
{
    id = -1;
    bool masked = false;
    if (s < a.cells) {
        masked = (a.players >> (s % a.P)) & 1u;
        id = a.ids[s];
    }
    valid = masked && id >= 0 && (uint32_t)id < a.num_policies;
    beyond = masked && id >= 0 && (uint32_t)id >= a.num_policies;
}

// For the wave's lanes with `valid`, by distinct id: rank = the number of earlier lanes of the wave with this lane's id, total =
// the number of lanes with it, first = this lane is the earliest of them.  The loop runs once per distinct id of the wave.
__device__ __forceinline__ void plan_wave_ranks(bool valid, uint32_t id, uint32_t lane, uint32_t &rank, uint32_t &total, bool &first)
{
    rank = total = 0u;
    first = false;
    unsigned long long left = __ballot(valid);
    while (left) {
        const int leader = __ffsll(left) - 1;
        const uint32_t lid = (uint32_t)__shfl((int)id, leader);
        const bool mine = valid && id == lid;
        const unsigned long long same = __ballot(mine);
        if (mine) {
            rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            total = (uint32_t)__popcll(same);
            first = (int)lane == leader;
        }
        left &= ~same;
    }
}

// Pass one over the 1024 cells from `begin`: adds the chunk's cells per policy to count[] and its ids beyond the bank to
// *out_of_range (both LDS, integer adds, one per distinct id and wave), and writes the ids as this act uses them.
__device__ __forceinline__ void plan_count_chunk(const BankPlanArgs &a, uint32_t begin, uint32_t *count, uint32_t *out_of_range)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, s = begin + tid;
    int32_t id;
    bool valid, beyond;
    plan_cell(a, s, id, valid, beyond);
    const unsigned long long votes = __ballot(beyond);
    if (lane == 0 && votes) atomicAdd(out_of_range, (uint32_t)__popcll(votes));
    uint32_t rank, total;
    bool first;
    plan_wave_ranks(valid, (uint32_t)id, lane, rank, total, first);
    if (first) atomicAdd(&count[id], total);
    if (a.ids_row && s < a.cells) a.ids_row[s] = valid ? id : -1;
}

// Pass two over the 1024 cells from `begin`; the whole workgroup calls it.  before[k] (LDS) is the number of policy k's cells in
// front of this chunk, start[k] where its list begins; the chunk's acted cells go to start[k] + before[k] + (cells of k in
// earlier waves) + (cells of k in earlier lanes): ascending s, whatever the timing.  before[k] is advanced past the chunk.
__device__ __forceinline__ void plan_place_chunk(const BankPlanArgs &a, uint32_t begin, const uint32_t *start, uint32_t *before,
                                                 uint32_t *wave_count)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, K = a.num_policies, s = begin + tid;
    uint32_t *__restrict__ lists = a.workspace + a.at.lists_at;
    for (uint32_t e = tid; e < 16u * K; e += kBankPlanThreads) wave_count[(e / K) * kBankMaxPolicies + e % K] = 0u;
    __syncthreads();
    int32_t id;
    bool valid, beyond;
    plan_cell(a, s, id, valid, beyond);
    uint32_t rank, total;
    bool first;
    plan_wave_ranks(valid, (uint32_t)id, lane, rank, total, first);
    if (first) wave_count[wave * kBankMaxPolicies + id] = total;
    __syncthreads();
    if (tid < K) {  // the waves' counts of policy tid -> where each wave's cells of it begin
        uint32_t at = before[tid];
#pragma unroll
        for (uint32_t v = 0; v < 16; v++) {
            const uint32_t c = wave_count[v * kBankMaxPolicies + tid];
            wave_count[v * kBankMaxPolicies + tid] = at;
            at += c;
        }
        before[tid] = at;
    }
    __syncthreads();
    // start[id] + ... < start[id] + count[id] <= acted <= cells: pass one counted the same cells
    if (valid) lists[start[id] + wave_count[wave * kBankMaxPolicies + id] + rank] = s;
    __syncthreads();
}

// From the counts (LDS): the list starts and the tile starts, the header words, count[] and start[] in the workspace, the tile
// table.  The whole workgroup calls it behind a barrier; it ends behind one.
__device__ __forceinline__ void plan_table(const BankPlanArgs &a, const uint32_t *count, uint32_t *start, uint32_t *tile_start, uint32_t out_of_range)
{
    const uint32_t tid = threadIdx.x, K = a.num_policies;
    uint32_t *__restrict__ ws = a.workspace;
    if (tid == 0) {
        uint32_t cells = 0, tiles = 0;
        for (uint32_t k = 0; k < K; k++) {
            start[k] = cells, tile_start[k] = tiles;
            cells += count[k];
            tiles += (count[k] + kBankTile - 1u) / kBankTile;
        }
        start[K] = cells, tile_start[K] = tiles;
        ws[0] = tiles, ws[1] = cells, ws[2] = out_of_range, ws[3] = 0u;
    }
    __syncthreads();
    if (tid < K) ws[a.at.count_at + tid] = count[tid], ws[a.at.start_at + tid] = start[tid];
    // tile t belongs to the policy k with tile_start[k] <= t < tile_start[k + 1]
    const uint32_t tiles = tile_start[K];  // <= at.max_tiles: sum of ceil(c_k / 32) <= cells / 32 + K
    for (uint32_t t = tid; t < tiles; t += kBankPlanThreads) {
        uint32_t lo = 0, hi = K;  // tile_start[lo] <= t < tile_start[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (tile_start[mid] <= t)
                lo = mid;
            else
                hi = mid;
        }
        const uint32_t within = (t - tile_start[lo]) * kBankTile, left = count[lo] - within;
        uint32_t *__restrict__ entry = ws + a.at.table_at + 4u * (size_t)t;
        entry[0] = lo, entry[1] = start[lo] + within, entry[2] = left < kBankTile ? left : kBankTile, entry[3] = 0u;
    }
    __syncthreads();
}

// the plan of a small call (cells <= kBankPlanSingle), one workgroup: count, table, place
__global__ void __launch_bounds__(kBankPlanThreads) mrl_bank_plan(BankPlanArgs a)
{
    __shared__ uint32_t count[kBankMaxPolicies], before[kBankMaxPolicies];
    __shared__ uint32_t start[kBankMaxPolicies + 1], tile_start[kBankMaxPolicies + 1];
    __shared__ uint32_t wave_count[16 * kBankMaxPolicies];
    __shared__ uint32_t out_of_range;
    const uint32_t tid = threadIdx.x;
    if (tid < a.num_policies) count[tid] = before[tid] = 0u;
    if (tid == 0) out_of_range = 0u;
    __syncthreads();
    for (uint32_t begin = 0; begin < a.cells; begin += kBankPlanThreads) plan_count_chunk(a, begin, count, &out_of_range);
    __syncthreads();
    plan_table(a, count, start, tile_start, out_of_range);
    for (uint32_t begin = 0; begin < a.cells; begin += kBankPlanThreads) plan_place_chunk(a, begin, start, before, wave_count);
}

// The plan of a larger call, three launches with a workgroup per chunk of 1024 cells in the first and the last.  The chunks'
// counts travel through the workspace's last region, a row of chunk_ld words per chunk: [k] the chunk's cells of policy k, which
// the scan turns into the cells of k in front of the chunk; [Kp] the chunk's ids beyond the bank.
__global__ void __launch_bounds__(kBankPlanThreads) mrl_bank_plan_count(BankPlanArgs a)
{
    __shared__ uint32_t count[kBankMaxPolicies];
    __shared__ uint32_t out_of_range;
    const uint32_t tid = threadIdx.x;
    if (tid < a.num_policies) count[tid] = 0u;
    if (tid == 0) out_of_range = 0u;
    __syncthreads();
    plan_count_chunk(a, blockIdx.x * kBankPlanThreads, count, &out_of_range);
    __syncthreads();
    uint32_t *__restrict__ row = a.workspace + a.at.chunks_at + (size_t)blockIdx.x * a.at.chunk_ld;
    if (tid < a.num_policies) row[tid] = count[tid];
    if (tid == 0) row[a.at.chunk_ld - 4u] = out_of_range;
}

__global__ void __launch_bounds__(kBankPlanThreads) mrl_bank_plan_scan(BankPlanArgs a, uint32_t chunks)
{
    __shared__ uint32_t count[kBankMaxPolicies];
    __shared__ uint32_t start[kBankMaxPolicies + 1], tile_start[kBankMaxPolicies + 1];
    __shared__ uint32_t out_of_range;
    const uint32_t tid = threadIdx.x;
    uint32_t *__restrict__ rows = a.workspace + a.at.chunks_at;
    if (tid < a.num_policies || tid == kBankPlanThreads - 1u) {  // (K <= 256: the last thread is nobody's policy)
        const uint32_t column = tid < a.num_policies ? tid : (uint32_t)a.at.chunk_ld - 4u;
        uint32_t sum = 0;
        for (uint32_t c = 0; c < chunks; c++) {
            const uint32_t own = rows[(size_t)c * a.at.chunk_ld + column];
            rows[(size_t)c * a.at.chunk_ld + column] = sum;
            sum += own;
        }
        if (tid < a.num_policies)
            count[tid] = sum;
        else
            out_of_range = sum;
    }
    __syncthreads();
    plan_table(a, count, start, tile_start, out_of_range);
}

__global__ void __launch_bounds__(kBankPlanThreads) mrl_bank_plan_place(BankPlanArgs a)
{
    __shared__ uint32_t start[kBankMaxPolicies], before[kBankMaxPolicies];
    __shared__ uint32_t wave_count[16 * kBankMaxPolicies];
    const uint32_t tid = threadIdx.x;
    if (tid < a.num_policies) {
        start[tid] = a.workspace[a.at.start_at + tid];
        before[tid] = a.workspace[a.at.chunks_at + (size_t)blockIdx.x * a.at.chunk_ld + tid];
    }
    __syncthreads();
    plan_place_chunk(a, blockIdx.x * kBankPlanThreads, start, before, wave_count);
}

void launch_bank_plan(const BankPlanArgs &plan, hipStream_t stream)
{
    if (plan.cells <= kBankPlanSingle) {
        hipLaunchKernelGGL(mrl_bank_plan, dim3(1), dim3(kBankPlanThreads), 0, stream, plan);
        MRL_HIP(hipGetLastError());
        return;
    }
    const uint32_t chunks = (plan.cells + kBankPlanThreads - 1u) / kBankPlanThreads;
    hipLaunchKernelGGL(mrl_bank_plan_count, dim3(chunks), dim3(kBankPlanThreads), 0, stream, plan);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(mrl_bank_plan_scan, dim3(1), dim3(kBankPlanThreads), 0, stream, plan, chunks);
    MRL_HIP(hipGetLastError());
    hipLaunchKernelGGL(mrl_bank_plan_place, dim3(chunks), dim3(kBankPlanThreads), 0, stream, plan);
    MRL_HIP(hipGetLastError());
}

__global__ void __launch_bounds__(256) mrl_cnn_bank_resample_kernel(CnnResampleArgs a)
{
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.num_worlds || a.done[n] == 0) return;
    const uint32_t episode = (uint32_t)a.episodes[n] + 1u;
    a.episodes[n] = (int32_t)episode;
    for (uint32_t p = 0; p < a.P; p++) {
        if (!((a.players >> p) & 1u)) continue;
        const int32_t id = a.ids[(size_t)n * a.P + p];
        if (id < 0) continue;
        const uint32_t first = a.first[p], num = a.num[p];
        uint32_t next;
        if (a.mode == MRL_CNN_RESAMPLE_ROBIN)
            next = first + ((uint32_t)id - first + 1u) % num;
        else
            next = first + (((policy_hash(a.seed, episode, n, p) >> 8) * num) >> 24);  // 24 bits times num <= 256: no overflow
        a.ids[(size_t)n * a.P + p] = (int32_t)next;
    }
}

void launch_cnn_bank_resample(const CnnResampleArgs &args, hipStream_t stream)
{
    if (args.num_worlds == 0) return;
    hipLaunchKernelGGL(mrl_cnn_bank_resample_kernel, dim3((args.num_worlds + 255u) / 256u), dim3(256), 0, stream, args);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
