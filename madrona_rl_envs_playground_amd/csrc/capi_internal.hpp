// What the files of the C API (capi*.hip) share: the guard around every call, the simulator checks, the rollout loop and the
// refusals that more than one learner raises.  Declarations; a definition lives in the file that owns it (named at each).
// Every capi*.hip includes this header and the kernel headers it launches, and none includes another .hip.  DESIGN.md section 24.
#pragma once
#include "common.hpp"

namespace mrl {

// empties the text behind mrl_last_error, which is thread-local and private to capi.hip
void clear_error();

template <typename Fn> static int guarded(Fn &&fn)
{
    try {
        clear_error();
        fn();
        return MRL_OK;
    } catch (const HipError &e) {
        return e.code;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return MRL_ERR_INVALID;
    }
}

// ---- the simulator and its stream (capi.hip) ----
int need(const mrl_sim *sim);
int need_healthy(const mrl_sim *sim);
int need_not_capturing(const mrl_sim *sim, void *hip_stream, const char *what);
bool capturing(void *hip_stream);
void completed_step(mrl_sim *sim, hipStream_t stream);
// the counter games complete a two-phase step with phase 2; the kitchen games, whose phase 2 does nothing, with phase 1
inline bool completes_in_phase1(const mrl_sim *sim) { return sim->game == MRL_GAME_OVERCOOKED || sim->game == MRL_GAME_SIMPLECOOKED; }

// The loop of every MAPPO rollout, on `stream` of the simulator's device: act(k, closing) for k = 0..T with the ordinary step, its
// statistics and after_step() behind every act but the closing one.
template <class Act, class AfterStep>
static void rollout_loop(mrl_sim *sim, uint32_t T, hipStream_t stream, Act act, AfterStep after_step)
{
    for (uint32_t k = 0; k <= T; k++) {
        const bool closing = k == T;
        act(k, closing);
        if (closing) break;
        sim->step(nullptr, stream);
        completed_step(sim, stream);
        after_step();
    }
}

// ---- the updates' common tail (capi_ppo.hip) ----
int update_refusal(const char *what, const char *sizer, uint64_t workspace_bytes, uint64_t need_bytes, const void *workspace_dev,
                   bool arrays_off, const char *arrays_rule, void *hip_stream);

// ---- the policy banks (capi_bank.hip) ----
int bank_refusal(const char *what, uint32_t num_worlds, uint32_t seats, uint32_t num_policies, uint64_t stride, uint64_t num_params,
                 const int32_t *ids_dev, void *workspace_dev, uint64_t workspace_bytes, uint64_t need_bytes, const char *sizer);

// A network family as a resample sees it: its games, a bit per MRL_GAME_* (`has`: what any other game is told), the slot of an
// observation tensor and the axis of its shape that holds the seats, the slot of DONE (`tensors`: the two by name).
struct BankFamily {
    uint32_t games;
    const char *has;
    int obs_slot, seat_axis, done_slot;
    const char *tensors;
};
// What mrl_*_bank_resample and the bank rollouts check of a resample on a simulator of `family`; fills `args`.
struct CnnResampleArgs;
int bank_resample_prepare(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
                          int32_t *episodes_dev, const char *what, CnnResampleArgs *args);
// the three public resamples behind their family
int bank_resample(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
                  int32_t *episodes_dev, void *hip_stream, const char *what);

}  // namespace mrl
