// A bank of K wide policies (CleanPPOAgent's two 512-wide four-layer MLPs) and a policy per world for one seat of Hanabi or the
// balance beam (C ABI: mrl_agent_act_bank, mrl_agent_bank_resample, mrl_agent_bank_workspace_bytes in include/mrl_envs.h;
// DESIGN.md section 21).  The kernels live in wide_bank.hip; capi_wide.hip validates, with every bank's bank_refusal and bank_resample.
//
// An act is the effective ids (ids[n, player] where the world is computed, -1 elsewhere), the plan over them (bank_plan.hpp: the
// other banks' own, with P = 1 and N cells), mrl_wide_layer's body (wide_layer_body.hpp) over the plan's tiles, four launches,
// each tile (bank_entry's entry) under its own policy's row of the bank, and mrl_agent_head's body over the list positions
// [0, acted).  The resample is every bank's kernel (bank_plan.hpp), which reads DONE, the ids and the episodes only.
//
// THE WORKSPACE (include/mrl_envs.h repeats this: a test reads it back): mrl_agent_act's workspace first, wide_workspace_bytes(N)
// bytes, of which the activations, the logits and the values are used, indexed by position in the plan's lists; then eff, N int32
// in a region rounded up to 256 bytes; then bank_plan.hpp's words for N cells of one seat and K policies.
#pragma once

#include "bank_plan.hpp"
#include "wide_policy.hpp"

namespace mrl {

constexpr uint64_t wide_bank_eff_bytes(uint64_t n) { return (n * 4 + 255) / 256 * 256; }
constexpr uint64_t wide_bank_workspace_bytes(uint64_t n, uint64_t num_policies)
{
    return wide_workspace_bytes(n) + wide_bank_eff_bytes(n) + bank_layout(n, 1, num_policies).words * 4;
}

struct WideBankArgs {
    AgentActArgs act;     // params: row 0 of the bank; record null; ws: the front of the workspace
    const int32_t *ids;   // (N, P)
    int32_t *ids_row;     // (N) or nullptr: k where the world acted, -1 where it has a valid id and is not computed
    int32_t *eff;         // (N), in the workspace
    uint32_t *plan;       // bank_plan.hpp's words, in the workspace
    uint64_t stride;      // floats between two rows of the bank
    uint32_t P, num_policies;
};

// the effective ids, the plan, the four layers and the head on `stream`
void launch_agent_act_bank(const WideBankArgs &args, hipStream_t stream);

}  // namespace mrl
