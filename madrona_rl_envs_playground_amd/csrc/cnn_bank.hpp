// A bank of K CNN policies and a policy per (world, seat) cell (C ABI: mrl_cnn_act_bank, mrl_cnn_bank_resample,
// mrl_rollout_cnn_bank in include/mrl_envs.h).  The kernels live in cnn_bank.hip; capi.hip validates.
//
// An act is two launches.  The plan (bank_plan.hpp, which has the workspace layout; one copy for both networks' banks) gathers
// the acted cells of every policy into that policy's sample list and cuts the lists into tiles of at most 32 samples;
// mrl_cnn_act_bank is mrl_cnn_act's body (cnn_act_body.hpp) over those tiles, each with its own policy's row of the bank as the
// parameter array.
#pragma once

#include "bank_plan.hpp"
#include "cnn_policy.hpp"

namespace mrl {

static_assert(kCnnTile == kBankTile, "the plan cuts tiles of the act's size");

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
