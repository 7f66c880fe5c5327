// A bank of K MLPBase policies and a policy per (world, seat) cell of the balance beam (C ABI: mrl_mlpbase_act_bank,
// mrl_mlpbase_bank_resample, mrl_rollout_mlpbase_bank in include/mrl_envs.h).  The kernel lives in
// mlpbase_bank.hip; capi_mappo.hip validates, with every bank's helpers (capi_bank.hip, capi_internal.hpp).
//
// An act is the plan (bank_plan.hpp: every bank's, one copy, the same workspace words) and mrl_mlpbase_act's body
// (mlpbase_act_body.hpp) over the plan's tiles, each under its own policy's row of the bank.  The resample is bank_plan.hpp's too.
#pragma once

#include "bank_plan.hpp"
#include "mlpbase_policy.hpp"

namespace mrl {

static_assert(kMlpBaseTile == kBankTile, "the plan cuts tiles of the act's size");

struct MlpBaseBankArgs {
    MlpBaseActArgs act;  // params: row 0 of the bank; players and num_seats as for mrl_mlpbase_act
    BankActArgs bank;
};

// the plan and the act on `stream`
void launch_mlpbase_act_bank(const MlpBaseBankArgs &args, hipStream_t stream);

}  // namespace mrl
