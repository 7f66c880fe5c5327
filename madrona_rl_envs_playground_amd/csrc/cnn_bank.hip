// mrl_cnn_act_bank: MAPPO's CNN actor-critic with a policy per (world, seat) cell, out of a bank of K parameter rows
// (include/mrl_envs.h; the workspace layout is in bank_plan.hpp).
//
//   the plan            bank_plan.hip, shared with the MLP's bank: the acted cells of every policy gathered into that policy's
//                       list in ascending s, the lists cut into tiles of at most 32 cells of one policy.
//   mrl_cnn_act_bank    mrl_cnn_act's body.  Workgroup (t, net) leaves at once when t >= tiles; otherwise its up to 32 rows are
//                       lists[first .. first + rows) of the table's entry t and its parameters are row `policy` of the bank.
//   mrl_cnn_bank_resample   a lane per world: where DONE[n] != 0 the episode count goes up and the masked, non-negative cells of
//                       the world draw their next policy (it reads DONE, the ids and the episodes only: the MLP's bank runs it too).
// No float atomics, no scratch.
#include "cnn_bank.hpp"
#include "cnn_act_body.hpp"

namespace mrl {

__global__ void __launch_bounds__(kCnnThreads) mrl_cnn_act_bank(CnnBankArgs b, BankLayout at)
{
    const uint32_t *__restrict__ ws = b.workspace;
    if (blockIdx.x >= ws[0]) return;
    const uint32_t *__restrict__ entry = ws + at.table_at + 4u * (size_t)blockIdx.x;
    const uint32_t policy = entry[0], first = entry[1], rows = entry[2];
    cnn_act_body(b.act, BankTileMap{ws + at.lists_at + first, rows}, b.act.params + (size_t)policy * b.stride);
}

void launch_cnn_act_bank(const CnnBankArgs &args, hipStream_t stream)
{
    const CnnActArgs &a = args.act;
    const uint64_t cells = (uint64_t)a.num_worlds * a.P;
    if (cells == 0 || a.nets == 0) return;
    const BankLayout at = bank_layout(a.num_worlds, a.P, args.num_policies);
    launch_bank_plan(BankPlanArgs{args.ids, args.ids_row, args.workspace, (uint32_t)cells, a.P, a.players, args.num_policies, at}, stream);
    allow_large_dynamic_lds<&mrl_cnn_act_bank>(a.lds.total);
    // acted <= N * num_seats, so tiles <= ceil(N num_seats / 32) + K <= at.max_tiles
    const uint64_t bound = ((uint64_t)a.num_worlds * a.num_seats + kCnnTile - 1) / kCnnTile + args.num_policies;
    const dim3 grid((uint32_t)bound, a.nets == 3u ? 2u : 1u);
    hipLaunchKernelGGL(mrl_cnn_act_bank, grid, dim3(kCnnThreads), a.lds.total, stream, args, at);
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
