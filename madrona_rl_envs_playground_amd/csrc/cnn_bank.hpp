// A bank of K CNN policies and a policy per (world, seat) cell (C ABI: mrl_cnn_act_bank, mrl_cnn_bank_resample,
// mrl_rollout_cnn_bank in include/mrl_envs.h).  The kernel lives in cnn_bank.hip; capi_mappo.hip validates, with
// the helpers every bank shares (bank_refusal, bank_prepare, bank_resample, rollout_loop).
//
// An act is two launches: the plan (bank_plan.hpp, one copy for every bank, with the workspace layout, BankActArgs, bank_entry and
// the resample), then mrl_cnn_act's body (cnn_act_body.hpp) over the plan's tiles, each under its own policy's row of the bank.
#pragma once

#include "bank_plan.hpp"
#include "cnn_policy.hpp"

namespace mrl {

static_assert(kCnnTile == kBankTile, "the plan cuts tiles of the act's size");

struct CnnBankArgs {
    CnnActArgs act;  // params: row 0 of the bank; players and num_seats as for mrl_cnn_act
    BankActArgs bank;
};

// the plan and the act, two launches on `stream`
void launch_cnn_act_bank(const CnnBankArgs &args, hipStream_t stream);

}  // namespace mrl
