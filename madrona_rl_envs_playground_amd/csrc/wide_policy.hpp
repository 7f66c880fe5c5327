// The collection phase of CleanPPOAgent on the device for Hanabi and the balance beam (C ABI: mrl_agent_act,
// mrl_agent_credit, mrl_gae_active in include/mrl_envs.h).  The kernels live in wide_policy.hip;
// capi.hip validates the arguments and collects the simulator's tensors.
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
