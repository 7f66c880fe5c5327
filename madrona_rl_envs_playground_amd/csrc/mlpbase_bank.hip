// mrl_mlpbase_act_bank: MAPPO's MLP actor-critic for the balance beam with a policy per (world, seat) cell, out of a bank of K
// parameter rows (include/mrl_envs.h).
//
//   the plan               bank_plan.hip, shared with the other banks: the acted cells of every policy gathered into that policy's
//                          list in ascending s, the lists cut into tiles of at most 32 cells of one policy.
//   mrl_mlpbase_act_bank   mrl_mlpbase_act's body.  Workgroup (t, net) leaves at once when t >= tiles; otherwise its up to 32 rows
//                          are lists[first .. first + rows) of the table's entry t and its parameters are row `policy` of the bank.
// No float atomics, no workgroup waits on another, no scratch.
#include "mlpbase_bank.hpp"
#include "mlpbase_act_body.hpp"

namespace mrl {

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mlpbase_act_bank(MlpBaseBankArgs b, BankLayout at)
{
    const uint32_t *__restrict__ ws = b.bank.workspace;
    if (!bank_has_tile(ws, blockIdx.x)) return;
    const uint32_t *__restrict__ tile = bank_entry(ws, at.table_at, blockIdx.x);
    mlpbase_act_body(b.act, BankTileMap{ws + at.lists_at + tile[1], tile[2]}, b.act.params + (size_t)tile[0] * b.bank.stride);
}

void launch_mlpbase_act_bank(const MlpBaseBankArgs &args, hipStream_t stream)
{
    allow_large_dynamic_lds<&mrl_mlpbase_act_bank>(kMlpFwdFloats * 4u);
    launch_act_bank<&mrl_mlpbase_act_bank>(args, kMlpBaseThreads, kMlpFwdFloats * 4u, stream);
}

}  // namespace mrl
