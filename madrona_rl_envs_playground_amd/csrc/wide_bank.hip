// mrl_agent_act_bank: the wide policy (CleanPPOAgent's actor and critic) with a policy per world for one seat of Hanabi or the
// balance beam, out of a bank of K parameter rows (include/mrl_envs.h).  On one stream:
//
//   mrl_wide_bank_ids      a lane per world: eff[n] = ids[n, player] where the world is computed (ACTIVE_AGENT[player, n] != 0, or
//                          always with MRL_AGENT_ALL_ROWS) or the id lies beyond the bank (so that the plan counts it), -1
//                          elsewhere; a world with a valid id that is not computed gets action 0, as the plain act writes it.
//   the plan               bank_plan.hip, shared with the other banks, over eff as N cells of one seat: every policy's worlds in
//                          ascending order, the lists cut into tiles of at most 32 worlds of one policy.
//   mrl_wide_layer x4      the layer kernel of wide_layer_body.hpp under the map WideBankTiles.  Workgroup (t, slab, net) leaves at once when t >= tiles; otherwise its rows are the
//                          list positions first .. first + rows of the table's entry t (layer 1 gathers the worlds through the
//                          lists) and its weights and bias are the layer's inside row `policy` of the bank.  Activations, logits
//                          and values are indexed by list position.
//   mrl_agent_head_bank    mrl_agent_head's body over the list positions [0, acted); it also writes ids_row.
// No float atomics, no workgroup waits on another, no scratch: the same inputs give the same bits on every run.
#include "wide_bank.hpp"
#include "wide_layer_body.hpp"

namespace mrl {

static_assert(kTileRows == (int)kBankTile, "the plan cuts tiles of the layer's size");

__global__ void __launch_bounds__(256) mrl_wide_bank_ids(WideInput active, const int32_t *__restrict__ ids, uint32_t P, uint32_t player,
                                                         uint32_t num_worlds, uint32_t all_rows, uint32_t num_policies,
                                                         int32_t *__restrict__ eff, int32_t *__restrict__ action, int64_t action_stride,
                                                         int32_t *__restrict__ ids_row)
{
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= num_worlds) return;
    const int32_t id = ids[(size_t)n * P + player];
    const bool computed = all_rows || wide_nonzero(active, (int64_t)n * active.row_stride);
    const bool valid = id >= 0 && (uint32_t)id < num_policies;
    eff[n] = computed || !valid ? id : -1;  // (an invalid id acts nowhere; one beyond the bank is counted wherever it stands)
    if (valid && !computed) {
        action[(int64_t)n * action_stride] = 0;
        if (ids_row) ids_row[n] = -1;
    }
}

// The plan's table as the layer kernel's map: workgroup x takes bank_entry's entry x -- (policy, first, rows, 0) -- and has no tile
// when x >= tiles (the grid is sized for max_tiles, the table too, so the entry read lies inside the workspace whatever it holds).
struct WideBankTiles {
    const uint32_t *plan;  // bank_plan.hpp's words
    uint64_t table_at;     // word offset of the tile table
    uint64_t stride;       // floats between two rows of the bank
    __device__ __forceinline__ const uint32_t *entry() const { return bank_entry(plan, table_at, blockIdx.x); }
    __device__ __forceinline__ uint32_t end(const WideLayerArgs &) const { return bank_has_tile(plan, blockIdx.x) ? entry()[1] + entry()[2] : 0u; }
    __device__ __forceinline__ uint32_t first() const { return entry()[1]; }
    __device__ __forceinline__ size_t shift() const { return (size_t)entry()[0] * stride; }
};

__global__ void __launch_bounds__(64) mrl_agent_head_bank(HeadArgs a, const int32_t *__restrict__ eff, int32_t *__restrict__ ids_row)
{
    const uint32_t j = blockIdx.x * 64u + threadIdx.x;
    if (j >= *a.count) return;
    const uint32_t w = a.rows[j];
    wide_head_body(a, j, w);
    if (ids_row) ids_row[w] = eff[w];
}

void launch_agent_act_bank(const WideBankArgs &args, hipStream_t stream)
{
    const AgentActArgs &g = args.act;
    const uint32_t N = g.num_worlds;
    if (N == 0) return;
    hipLaunchKernelGGL(mrl_wide_bank_ids, dim3((N + 255) / 256), dim3(256), 0, stream, g.active, args.ids, args.P, g.player, N,
                       g.flags & MRL_AGENT_ALL_ROWS ? 1u : 0u, args.num_policies, args.eff, g.action, g.action_stride, args.ids_row);
    MRL_HIP(hipGetLastError());

    const BankLayout at = bank_layout(N, 1, args.num_policies);
    launch_bank_plan(BankPlanArgs{args.eff, nullptr, args.plan, N, 1u, 1u, args.num_policies, at}, stream);
    const uint32_t *lists = args.plan + at.lists_at, *acted = args.plan + 1;

    WideForwardArgs fwd{};
    fwd.params = g.params, fwd.obs = g.obs, fwd.state = g.state;
    fwd.D = g.D, fwd.S = g.S, fwd.A = g.A, fwd.max_rows = N, fwd.nets = 2u;
    fwd.rows = lists, fwd.count = acted;
    for (uint32_t net = 0; net < 2; net++)
        for (uint32_t layer = 0; layer < 3; layer++) fwd.hidden[net][layer] = g.ws.hidden[layer & 1u] + (uint64_t)net * N * kWideHidden;
    fwd.logits = g.ws.logits, fwd.value = g.ws.value;
    // acted <= N, so tiles <= ceil(N / 32) + K = at.max_tiles
    for (uint32_t layer = 0; layer < 4; layer++)
        hipLaunchKernelGGL(mrl_wide_layer<WideBankTiles>, dim3((uint32_t)at.max_tiles, wide_layer_slabs(layer), 2u), dim3(kLayerThreads), 0,
                           stream, wide_layer_args(fwd, layer), WideBankTiles{args.plan, at.table_at, args.stride});
    MRL_HIP(hipGetLastError());

    HeadArgs head{};
    head.rows = lists, head.count = acted, head.logits = g.ws.logits, head.value = g.ws.value;
    head.mask = g.mask, head.action = g.action, head.action_stride = g.action_stride;
    head.has_record = 0u;
    head.row = 0u, head.flags = g.flags, head.A = g.A, head.num_worlds = N, head.player = g.player, head.step = g.step;
    head.seed = g.seed;
    hipLaunchKernelGGL(mrl_agent_head_bank, dim3((N + 63) / 64), dim3(64), 0, stream, head, args.eff, args.ids_row);
    MRL_HIP(hipGetLastError());
}

}  // namespace mrl
