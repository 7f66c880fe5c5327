// The learning phase of CleanPPOAgent on the device for the wide policy (C ABI: mrl_agent_update in include/mrl_envs.h;
// DESIGN.md section 17).  The kernels live in wide_update.hip; the forward pass is wide_policy.hip's own mrl_wide_layer.
#pragma once

#include "wide_policy.hpp"

namespace mrl {

constexpr uint32_t kUpdateStats = 10;        // a stats row: mrl_ppo_update's eight columns, samples, status
constexpr uint32_t kUpdateHeadThreads = 256;  // samples per workgroup of the loss head, one partial stats row each

constexpr uint64_t update_pad(uint64_t bytes) { return (bytes + 255) / 256 * 256; }

// The caller's workspace for `n` = capacity samples and P parameters, every part a multiple of 256 bytes, in this order:
//   the sample list (n uint32) and one 256-byte slot of three words: B, the samples to compute (B, or 0 with a status), status
//   activations   (2 nets, 3 layers, n, 512) floats: what the forward pass leaves and the backward pass reads
//   d_hidden      (2 nets, 3 layers, n, 512) floats: dLoss / d(pre-activation) of every hidden layer
//   logits, d_logits (n, 64) floats each; value, d_value (n) floats each
//   (mean, std + 1e-8) of the advantages, one slot
//   the loss head's partial stats, (ceil(n / 256), 8) doubles
//   the gradient vector (P) that the weight-gradient kernel writes, the copy mrl_grad_reduce makes of it (P), and the
//   per-block sums of g^2 (ceil(P / 256))
struct UpdateWorkspace {
    uint32_t *rows, *words;  // words[0] = B, words[1] = live, words[2] = status
    float *act[2][3], *dh[2][3];
    float *logits, *d_logits, *value, *d_value, *mean_std;
    double *partial_stats;
    float *grad, *grad_sum, *sumsq;
};
constexpr uint64_t update_workspace_bytes(uint64_t n, uint64_t P)
{
    return wide_rows_bytes(n) + 2 * (6 * n * kWideHidden * 4) + 2 * (n * kWideMaxActions * 4) + 2 * update_pad(n * 4) + 256 +
           update_pad((n + kUpdateHeadThreads - 1) / kUpdateHeadThreads * 8 * 8) + 2 * update_pad(P * 4) + update_pad((P + 255) / 256 * 4);
}
inline UpdateWorkspace update_workspace(void *base, uint64_t n, uint64_t P)
{
    char *p = static_cast<char *>(base);
    UpdateWorkspace ws{};
    ws.rows = reinterpret_cast<uint32_t *>(p);
    ws.words = reinterpret_cast<uint32_t *>(p + wide_rows_bytes(n) - 256);
    p += wide_rows_bytes(n);
    float *f = reinterpret_cast<float *>(p);
    for (int net = 0; net < 2; net++)
        for (int layer = 0; layer < 3; layer++, f += n * kWideHidden) ws.act[net][layer] = f;
    for (int net = 0; net < 2; net++)
        for (int layer = 0; layer < 3; layer++, f += n * kWideHidden) ws.dh[net][layer] = f;
    ws.logits = f, f += n * kWideMaxActions;
    ws.d_logits = f, f += n * kWideMaxActions;
    p = reinterpret_cast<char *>(f);
    ws.value = reinterpret_cast<float *>(p), p += update_pad(n * 4);
    ws.d_value = reinterpret_cast<float *>(p), p += update_pad(n * 4);
    ws.mean_std = reinterpret_cast<float *>(p), p += 256;
    ws.partial_stats = reinterpret_cast<double *>(p), p += update_pad((n + kUpdateHeadThreads - 1) / kUpdateHeadThreads * 8 * 8);
    ws.grad = reinterpret_cast<float *>(p), p += update_pad(P * 4);
    ws.grad_sum = reinterpret_cast<float *>(p), p += update_pad(P * 4);
    ws.sumsq = reinterpret_cast<float *>(p);
    return ws;
}

struct AgentUpdateArgs {
    mrl_wide_policy policy;
    mrl_ppo_optimizer opt;
    mrl_agent_record record;
    uint32_t obs_type, state_type;
    const float *advantages, *returns;
    uint32_t epochs, capacity;
    mrl_ppo_config cfg;
    void *workspace;
    float *stats, *grads;
};

void launch_agent_update(const AgentUpdateArgs &args, hipStream_t stream);

}  // namespace mrl
