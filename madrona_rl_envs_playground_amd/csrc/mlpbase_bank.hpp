// A bank of K MLPBase policies and a policy per (world, seat) cell of the balance beam (C ABI: mrl_mlpbase_act_bank,
// mrl_mlpbase_bank_resample, mrl_rollout_mlpbase_bank in include/mrl_envs.h).  The kernel lives in
// mlpbase_bank.hip; capi.hip validates.
//
// An act is the plan (bank_plan.hpp: the CNN bank's, one copy, the same workspace words) and mrl_mlpbase_act_bank, which is
// mrl_mlpbase_act's body (mlpbase_act_body.hpp) over the plan's tiles, each with its own policy's row of the bank as the
// parameter array.  The resample is the CNN bank's kernel (cnn_bank.hpp), which reads DONE, the ids and the episodes only.
#pragma once

#include "bank_plan.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

static_assert(kMlpBaseTile == kBankTile, "the plan cuts tiles of the act's size");

struct MlpBaseBankArgs {
    MlpBaseActArgs act;      // params: row 0 of the bank; players and num_seats as for mrl_mlpbase_act
    const int32_t *ids;      // (N, P)
    int32_t *ids_row;        // (N, P) or nullptr: k where the cell was acted, -1 elsewhere
    uint32_t *workspace;     // bank_plan.hpp's layout
    uint64_t stride;         // floats between two rows of the bank
    uint32_t num_policies;
};

// the plan and the act on `stream`
void launch_mlpbase_act_bank(const MlpBaseBankArgs &args, hipStream_t stream);

}  // namespace mrl
