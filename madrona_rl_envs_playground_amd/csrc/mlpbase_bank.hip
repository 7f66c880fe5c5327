// mrl_mlpbase_act_bank: MAPPO's MLP actor-critic for the balance beam with a policy per (world, seat) cell, out of a bank of K
// parameter rows (include/mrl_envs.h).
//
//   the plan               bank_plan.hip, shared with the CNN's bank: the acted cells of every policy gathered into that policy's
//                          list in ascending s, the lists cut into tiles of at most 32 cells of one policy.
//   mrl_mlpbase_act_bank   mrl_mlpbase_act's body.  Workgroup (t, net) leaves at once when t >= tiles; otherwise its up to 32 rows
//                          are lists[first .. first + rows) of the table's entry t and its parameters are row `policy` of the bank.
// No float atomics, no workgroup waits on another, no scratch.
#include "mlpbase_bank.hpp"
#include "mlpbase_act_body.hpp"

namespace mrl {

__global__ void __launch_bounds__(kMlpBaseThreads) mrl_mlpbase_act_bank(MlpBaseBankArgs b, BankLayout at)
{
    const uint32_t *__restrict__ ws = b.workspace;
    if (blockIdx.x >= ws[0]) return;
    const uint32_t *__restrict__ entry = ws + at.table_at + 4u * (size_t)blockIdx.x;
    const uint32_t policy = entry[0], first = entry[1], rows = entry[2];
    mlpbase_act_body(b.act, BankTileMap{ws + at.lists_at + first, rows}, b.act.params + (size_t)policy * b.stride);
}

void launch_mlpbase_act_bank(const MlpBaseBankArgs &args, hipStream_t stream)
{
    const MlpBaseActArgs &a = args.act;
    const uint64_t cells = (uint64_t)a.num_worlds * a.P;
    if (cells == 0 || a.nets == 0) return;
    const BankLayout at = bank_layout(a.num_worlds, a.P, args.num_policies);
    launch_bank_plan(BankPlanArgs{args.ids, args.ids_row, args.workspace, (uint32_t)cells, a.P, a.players, args.num_policies, at}, stream);
    constexpr uint32_t bytes = kMlpFwdFloats * 4u;
    allow_large_dynamic_lds<&mrl_mlpbase_act_bank>(bytes);
    // acted <= N * num_seats, so tiles <= ceil(N num_seats / 32) + K <= at.max_tiles
    const uint64_t bound = ((uint64_t)a.num_worlds * a.num_seats + kMlpBaseTile - 1) / kMlpBaseTile + args.num_policies;
    const dim3 grid((uint32_t)bound, a.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_mlpbase_act_bank, grid, dim3(kMlpBaseThreads), bytes, stream, args, at);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
