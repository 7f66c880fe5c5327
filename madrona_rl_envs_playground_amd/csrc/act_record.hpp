// What the act kernels of MAPPO's two actor-critics share (mrl_cnn_act and mrl_cnn_act_bank through cnn_act_body.hpp,
// mrl_mlpbase_act and mrl_mlpbase_act_bank through mlpbase_act_body.hpp; DESIGN.md sections 15, 18, 19 and 20): the arguments every act carries whatever its network,
// the map from a sample of the call to its (world, seat), and the tail that turns the head's outputs into the record's rows.
#pragma once

#include "common.hpp"
#include "random_policy.hpp"

namespace mrl {

// CnnActArgs and MlpBaseActArgs begin with this and add their own network's part (parameters, observations, REWARD, shapes)
struct ActArgs {
    const int32_t *done;       // DONE (N)
    int32_t *action;           // ACTION (P, N)
    // the record's rows for this call (nullptr: not written)
    int32_t *actions_row;                   // (N, P)
    float *logprobs_row, *values_row;       // (N, P)
    float *rewards_row, *dones_row;         // (N, P): rewards[row - 1]; dones[row] or next_done
    float *logits_row;                      // (N, P, actions)
    uint32_t P, num_worlds;
    uint32_t players, num_seats;            // the seat mask and its popcount
    uint32_t step, flags;
    uint32_t nets;                          // bit 0: the actor runs, bit 1: the critic runs
    uint64_t seed;
};

// the net a workgroup of an act runs: 0 the actor, 1 the critic (blockIdx.y chooses where both run)
__device__ __forceinline__ uint32_t act_net(const ActArgs &a) { return a.nets == 3u ? blockIdx.y : a.nets >> 1; }

// sample s of an act -> (world, seat): seat = the (s % num_seats)-th set bit of the mask
__device__ __forceinline__ void seat_sample(uint32_t players, uint32_t num_seats, uint32_t s, uint32_t &world, uint32_t &seat)
{
    world = s / num_seats;
    uint32_t idx = s - world * num_seats, mask = players;
    for (; idx > 0; idx--) mask &= mask - 1u;
    seat = (uint32_t)__ffs((int)mask) - 1u;
}

// The end of an act for the sample in the tile's row `tid` (lanes 0..31 of wave 0 call it, a sample each), given the head's
// outputs in LDS (row stride 8).  The critic's workgroup writes the value, the done flag and the reward (REWARD (P, N), int32 in
// the kitchens and float on the balance beam); the actor's draws the action (mrl_policy_act's rule) and writes it, its log-prob
// and the A logits.
template <int A, class Reward>
__device__ __forceinline__ void act_tail(const ActArgs &a, const float *outs, uint32_t net, uint32_t tid, uint32_t world, uint32_t seat,
                                         const Reward *__restrict__ reward)
{
    const size_t cell = (size_t)world * a.P + seat, agent = (size_t)seat * a.num_worlds + world;
    if (net) {
        if (a.values_row) a.values_row[cell] = outs[tid * 8u];
        if (a.dones_row) a.dones_row[cell] = a.done[world] != 0 ? 1.0f : 0.0f;
        if (a.rewards_row) a.rewards_row[cell] = (float)reward[agent];
        return;
    }
    float l[A];  // statically indexed throughout: stays in registers
#pragma unroll
    for (int i = 0; i < A; i++) l[i] = outs[tid * 8u + i];
    int action;
    float logprob;
    categorical_sample<A>(l, policy_hash(a.seed, a.step, world, seat), a.flags & MRL_POLICY_GREEDY, action, logprob);
    a.action[agent] = action;
    if (a.actions_row) a.actions_row[cell] = action;
    if (a.logprobs_row) a.logprobs_row[cell] = logprob;
    if (a.logits_row) {
#pragma unroll
        for (int i = 0; i < A; i++) a.logits_row[cell * A + i] = l[i];
    }
}

}  // namespace mrl
