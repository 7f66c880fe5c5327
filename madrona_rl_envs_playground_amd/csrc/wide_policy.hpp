// The collection phase of CleanPPOAgent on the device for Hanabi and the balance beam (C ABI: mrl_agent_act,
// mrl_agent_credit, mrl_gae_active in include/mrl_envs.h).  The kernels live in wide_policy.hip;
// capi_wide.hip validates the arguments and collects the simulator's tensors.
#pragma once

#include "common.hpp"

namespace mrl {

constexpr uint32_t kWideHidden = MRL_WIDE_HIDDEN;
constexpr uint32_t kWideMaxActions = MRL_WIDE_MAX_ACTIONS;

// one four-layer net: Linear(in, 512), Linear(512, 512), Linear(512, 512), Linear(512, out), each weight followed by its bias
constexpr uint64_t wide_net_params(uint64_t in, uint64_t out)
{
    return in * kWideHidden + kWideHidden + 2 * ((uint64_t)kWideHidden * kWideHidden + kWideHidden) + kWideHidden * out + out;
}

// The caller's workspace, in this order: the compacted world list (N uint32), its length (one uint32 in a 256-byte slot), two
// activation buffers of (2 nets, N, 512) floats that the layers alternate between, the logits (N, 64) and the values (N).
struct WideWorkspace {
    uint32_t *rows, *count;
    float *hidden[2];
    float *logits, *value;
};
constexpr uint64_t wide_rows_bytes(uint64_t n) { return (n * 4 + 255) / 256 * 256 + 256; }
constexpr uint64_t wide_workspace_bytes(uint64_t n)
{
    return wide_rows_bytes(n) + 2 * (2 * n * kWideHidden * 4) + n * kWideMaxActions * 4 + (n * 4 + 255) / 256 * 256;
}
inline WideWorkspace wide_workspace(void *base, uint64_t n)
{
    char *p = static_cast<char *>(base);
    WideWorkspace ws{};
    ws.rows = reinterpret_cast<uint32_t *>(p);
    ws.count = reinterpret_cast<uint32_t *>(p + wide_rows_bytes(n) - 256);
    p += wide_rows_bytes(n);
    ws.hidden[0] = reinterpret_cast<float *>(p);
    ws.hidden[1] = ws.hidden[0] + 2 * n * kWideHidden;
    ws.logits = ws.hidden[1] + 2 * n * kWideHidden;
    ws.value = ws.logits + n * kWideMaxActions;
    return ws;
}

// a row-strided view of one player's slice of a simulator tensor: element (w, k) at data + (w * row_stride + k) elements
struct WideInput {
    const void *data;
    int64_t row_stride;  // in elements
    uint32_t type;       // MRL_INT8 ...
};

// an element of a simulator tensor or of a record row, converted on load
__device__ __forceinline__ float wide_load(const void *p, uint32_t type, int64_t at)
{
    switch (type) {
    case MRL_INT8: return (float)static_cast<const int8_t *>(p)[at];
    case MRL_UINT8: return (float)static_cast<const uint8_t *>(p)[at];
    case MRL_INT32: return (float)static_cast<const int32_t *>(p)[at];
    case MRL_UINT32: return (float)static_cast<const uint32_t *>(p)[at];
    default: return static_cast<const float *>(p)[at];
    }
}

// The four mrl_wide_layer launches of one forward pass over the rows rows[0 .. *count): layer 1 gathers row rows[j] of `state`
// (critic, net 0) and `obs` (actor, net 1), layer l writes hidden[net][l - 1], layer 4 writes value (j) and logits (j, 64).  The
// grids are sized for max_rows; tiles past *count leave at once.  The act alternates between two buffers, so its hidden[net][2]
// is its hidden[net][0]; the update (wide_update.hip) keeps all three, which its backward pass reads.
struct WideForwardArgs {
    const float *params;
    WideInput obs, state;  // (rows, D), (rows, S)
    uint32_t D, S, A, max_rows, nets;  // nets = 1: the critic alone
    const uint32_t *rows, *count;
    float *hidden[2][3];
    float *logits, *value;
};
void launch_wide_forward(const WideForwardArgs &args, hipStream_t stream);

struct AgentActArgs {
    const float *params;
    WideInput obs, state, mask;  // (N, D), (N, S), (N, A)
    WideInput active;            // (N): row_stride is the stride between worlds
    int32_t *action;             // ACTION[player, :], stride action_stride
    int64_t action_stride;
    uint32_t D, S, A, num_worlds, player;
    const mrl_agent_record *record;  // host pointer or nullptr
    uint32_t row, step, flags;
    uint64_t seed;
    WideWorkspace ws;
};

void launch_agent_act(const AgentActArgs &args, hipStream_t stream);
void launch_agent_credit(const mrl_agent_record &record, const float *rewards, const int32_t *dones, uint32_t num_worlds,
                         hipStream_t stream);
void launch_gae_active(const mrl_agent_record &record, const float *next_value, const uint8_t *next_active, float gamma, float lambda,
                       float *advantages, float *returns, hipStream_t stream);

}  // namespace mrl
