// What the three policy banks share below the C API (capi_bank.hip; cnn_bank.hip, mlpbase_bank.hip, wide_bank.hip; DESIGN.md sections 19 to 21):
// the plan of a bank act -- the acted cells of every policy gathered into that policy's sample list, the lists cut into tiles of at
// most 32 samples --, the MAPPO banks' arguments and launcher, the tile table's reader and the resample.  Kernels: bank_plan.hip.
//
// THE WORKSPACE, in uint32 words (include/mrl_envs.h repeats this: a test reads it back).  M = N P cells, Kp = K rounded up to a
// multiple of 4, max_tiles = ceil(M / 32) + K:
//     [0] tiles   [1] acted   [2] out_of_range   [3] 0
//     [4, 4 + Kp)                     count[k]: the acted cells of policy k
//     [4 + Kp, 4 + 2 Kp)              start[k]: where policy k's list begins in `lists` (the exclusive prefix of count)
//     [4 + 2 Kp, 4 + 2 Kp + 4 max_tiles)   the tile table, four words per tile: policy, first (an index into lists), rows, 0
//     then M rounded up to a multiple of 4: lists, samples s = n P + p, every policy's in ascending s
//     then ceil(M / 1024) rows of Kp + 4 words: the plan's own (per chunk of 1024 cells, the cells of every policy in front of
//     the chunk and the chunk's ids beyond the bank; written only when M > 2048)
#pragma once

#include "common.hpp"

namespace mrl {

constexpr uint32_t kBankMaxPolicies = 256, kBankPlanThreads = 1024;
constexpr uint32_t kBankPlanSingle = 2048;  // up to this many cells one workgroup plans; beyond, a workgroup per 1024 cells
constexpr uint32_t kBankTile = 32;          // the samples of a tile: both nets' act kernels run tiles of 32

struct BankLayout {
    uint64_t count_at, start_at, table_at, lists_at, chunks_at, words;  // word offsets
    uint64_t max_tiles, chunk_ld;
};
constexpr BankLayout bank_layout(uint64_t num_worlds, uint64_t num_players, uint64_t num_policies)
{
    const uint64_t M = num_worlds * num_players, Kp = (num_policies + 3u) & ~(uint64_t)3u, max_tiles = (M + kBankTile - 1) / kBankTile + num_policies;
    const uint64_t lists_at = 4 + 2 * Kp + 4 * max_tiles, chunks_at = lists_at + ((M + 3u) & ~(uint64_t)3u);
    const uint64_t chunks = (M + kBankPlanThreads - 1) / kBankPlanThreads, chunk_ld = Kp + 4;
    return BankLayout{4, 4 + Kp, 4 + 2 * Kp, lists_at, chunks_at, chunks_at + chunks * chunk_ld, max_tiles, chunk_ld};
}

struct BankPlanArgs {
    const int32_t *ids;      // (N, P)
    int32_t *ids_row;        // (N, P) or nullptr: k where the cell is acted, -1 elsewhere
    uint32_t *workspace;     // the layout above
    uint32_t cells, P, players, num_policies;
    BankLayout at;
};

// the plan on `stream`: one launch up to kBankPlanSingle cells, three beyond
void launch_bank_plan(const BankPlanArgs &args, hipStream_t stream);

// The bank's part of the arguments of mrl_cnn_act_bank and mrl_mlpbase_act_bank, behind the network's own act arguments
struct BankActArgs {
    const int32_t *ids;      // (N, P)
    int32_t *ids_row;        // (N, P) or nullptr: k where the cell was acted, -1 elsewhere
    uint32_t *workspace;     // the layout above
    uint64_t stride;         // floats between two rows of the bank
    uint32_t num_policies;
};

// A MAPPO bank act (`args`: an ActArgs `act` and `bank`) on `stream`: the plan, then KERNEL(args, layout) over the plan's tiles.
// acted <= N * num_seats, so tiles <= ceil(N num_seats / 32) + K <= at.max_tiles: every workgroup's entry read lies in the table.
template <auto KERNEL, class Args>
inline void launch_act_bank(const Args &args, uint32_t threads, uint32_t lds_bytes, hipStream_t stream)
{
    const auto &a = args.act;
    const BankActArgs &b = args.bank;
    if ((uint64_t)a.num_worlds * a.P == 0 || a.nets == 0) return;
    const BankLayout at = bank_layout(a.num_worlds, a.P, b.num_policies);
    launch_bank_plan(BankPlanArgs{b.ids, b.ids_row, b.workspace, a.num_worlds * a.P, a.P, a.players, b.num_policies, at}, stream);
    const uint64_t bound = ((uint64_t)a.num_worlds * a.num_seats + kBankTile - 1) / kBankTile + b.num_policies;
    hipLaunchKernelGGL(KERNEL, dim3((uint32_t)bound, a.nets == 3u ? 2u : 1u), dim3(threads), lds_bytes, stream, args, at);
    MRL_HIP(hipGetLastError());
}

// whether workgroup x has a tile, and its entry of the tile table (policy, first, rows, 0): inside the table whatever x, a tile's only then
__device__ __forceinline__ bool bank_has_tile(const uint32_t *__restrict__ ws, uint32_t x) { return x < ws[0]; }
__device__ __forceinline__ const uint32_t *bank_entry(const uint32_t *__restrict__ ws, uint64_t table_at, uint32_t x)
{
    return ws + table_at + 4u * (size_t)x;
}

// a tile of the plan as an act body's map: rows of one policy's list (Args: the act's arguments, for P)
struct BankTileMap {
    const uint32_t *list;
    uint32_t rows;
    __device__ __forceinline__ bool has(uint32_t row) const { return row < rows; }
    template <class Args>
    __device__ __forceinline__ void locate(const Args &a, uint32_t row, uint32_t &world, uint32_t &seat) const
    {
        const uint32_t s = list[row];
        world = s / a.P;
        seat = s - world * a.P;
    }
    template <class Args>
    __device__ __forceinline__ bool sample(const Args &a, uint32_t row, uint32_t &world, uint32_t &seat) const
    {
        if (!has(row)) return false;
        locate(a, row, world, seat);
        return true;
    }
};

// the resample of every bank, mrl_cnn_bank_resample_kernel: it reads DONE, the ids and the episodes only
struct CnnResampleArgs {
    const int32_t *done;     // DONE (N)
    int32_t *ids;            // (N, P)
    int32_t *episodes;       // (N)
    uint64_t seed;
    uint32_t num_worlds, P, players, mode;
    uint16_t first[32], num[32];  // per seat
};

void launch_cnn_bank_resample(const CnnResampleArgs &args, hipStream_t stream);

}  // namespace mrl
