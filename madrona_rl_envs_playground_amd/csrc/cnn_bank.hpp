// A bank of K CNN policies and a policy per (world, seat) cell (C ABI: mrl_cnn_act_bank, mrl_cnn_bank_resample,
// mrl_rollout_cnn_bank in include/mrl_envs.h).  The kernels live in cnn_bank.hip; capi.hip validates.
//
// An act is two launches.  mrl_cnn_bank_plan gathers the acted cells of every policy into that policy's sample list and cuts the
// lists into tiles of at most 32 samples; mrl_cnn_act_bank is mrl_cnn_act's body (cnn_act_body.hpp) over those tiles, each with
// its own policy's row of the bank as the parameter array.
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

#include "cnn_policy.hpp"

namespace mrl {

constexpr uint32_t kCnnBankMaxPolicies = 256, kCnnPlanThreads = 1024;
constexpr uint32_t kCnnPlanSingle = 2048;  // up to this many cells one workgroup plans; beyond, a workgroup per 1024 cells

struct CnnBankLayout {
    uint64_t count_at, start_at, table_at, lists_at, chunks_at, words;  // word offsets
    uint64_t max_tiles, chunk_ld;
};
constexpr CnnBankLayout cnn_bank_layout(uint64_t num_worlds, uint64_t num_players, uint64_t num_policies)
{
    const uint64_t M = num_worlds * num_players, Kp = (num_policies + 3u) & ~(uint64_t)3u, max_tiles = (M + kCnnTile - 1) / kCnnTile + num_policies;
    const uint64_t lists_at = 4 + 2 * Kp + 4 * max_tiles, chunks_at = lists_at + ((M + 3u) & ~(uint64_t)3u);
    const uint64_t chunks = (M + kCnnPlanThreads - 1) / kCnnPlanThreads, chunk_ld = Kp + 4;
    return CnnBankLayout{4, 4 + Kp, 4 + 2 * Kp, lists_at, chunks_at, chunks_at + chunks * chunk_ld, max_tiles, chunk_ld};
}

struct CnnBankArgs {
    CnnActArgs act;          // params: row 0 of the bank; players and num_seats as for mrl_cnn_act
    const int32_t *ids;      // (N, P)
    int32_t *ids_row;        // (N, P) or nullptr: k where the cell was acted, -1 elsewhere
    uint32_t *workspace;     // the layout above
    uint64_t stride;         // floats between two rows of the bank
    uint32_t num_policies;
};

// the plan and the act, two launches on `stream`
void launch_cnn_act_bank(const CnnBankArgs &args, hipStream_t stream);

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
