// The C API of MAPPO's two actor-critics (include/mrl_envs.h): the CNN of the kitchens and MLPBase of the balance beam -- act,
// rollout and update, each plain and over a policy bank -- and what every bank shares (bank_refusal, the resample).  A traits
// type per network (CnnNet, MlpBaseNet: the twins of _mappo._CNN and _MLPBASE) states once what differs; act, act_bank, rollout,
// rollout_bank and mappo_update are written once over it, and the entry points pass their own name.  DESIGN.md section 24.
#include "capi_internal.hpp"
#include "cnn_policy.hpp"
#include "cnn_bank.hpp"
#include "cnn_update.hpp"
#include "mlpbase_policy.hpp"
#include "mlpbase_bank.hpp"
#include "mlpbase_gru.hpp"
#include "mlpbase_update.hpp"

#include <type_traits>

// what mrl_mappo_workspace_bytes and mrl_mappo_update refuse alike: nullptr when the shape can run, else why not
static const char *mappo_shape_error(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size)
{
    if (hidden != mrl::kCnnHidden) return "hidden must be 64";
    if (width < 3 || height < 3 || channels == 0) return "the kitchen must be at least 3 x 3 with at least one channel";
    if ((uint64_t)width * height * channels > 65535u) return "the kitchen's LDS image does not fit one workgroup's 160 KiB";
    if (mrl::cnn_update_lds(width, height, channels).total > mrl::kCnnLdsLimit) return "the kitchen's LDS image does not fit one workgroup's 160 KiB";
    if (minibatch_size == 0) return "minibatch_size must be positive";
    return nullptr;
}

// what mrl_mappo_mlp_workspace_bytes and mrl_mappo_mlp_update refuse alike: nullptr when the shape can run, else why not
static const char *mappo_mlp_shape_error(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size)
{
    if (hidden != mrl::kMlpBaseHidden) return "hidden must be 64";
    if (layer_N < 1 || layer_N > mrl::kMlpBaseMaxLayerN) return "layer_N must be 1 or 2";
    if (obs_dim != mrl::kMlpBaseObs || num_actions != mrl::kMlpBaseActions) return "obs_dim must be 7 and num_actions 4";
    if (minibatch_size == 0) return "minibatch_size must be positive";
    return nullptr;
}

namespace mrl {

// What the acts and rollouts of MAPPO's two actor-critics (`what`: the entry point) check and fill alike, whatever the network.
static_assert(MRL_CNN_VALUE_ONLY == MRL_MLPBASE_VALUE_ONLY, "one closing-act bit for both networks");

// Behind the caller's own checks of the simulator's health and game: `out_of_scope` is why the network does not run on this
// simulator (a rank of an exchanged batch, say) or nullptr, and the stream must not be capturing.
static int act_scope_refusal(const char *what, const char *out_of_scope, void *hip_stream)
{
    if (out_of_scope) {
        mrl::set_error("%s: %s", what, out_of_scope);
        return MRL_ERR_INVALID;
    }
    if (mrl::capturing(hip_stream)) {
        mrl::set_error("%s: the row and the step number travel in kernel arguments, a captured call would replay them", what);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// the record's buffers every act writes; `own`: the network's own buffers are there too
template <class Record>
static int act_record_refusal(const char *what, const Record *record, bool own)
{
    if (record && (!record->actions || !record->logprobs || !record->values || !record->rewards || !record->dones || !record->next_done || !own)) {
        mrl::set_error("%s: the record needs every buffer but logits", what);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// An act's own flags (`only`: the name of its closing-act bit, for the message) and its row: the policy's flags join in, the
// closing act needs a record and row == num_steps, every other act row < num_steps.
template <class Record>
static int act_row_refusal(const char *what, const char *only, uint32_t &flags, uint32_t policy_flags, const Record *record, uint32_t row)
{
    if (flags & ~(uint32_t)(MRL_POLICY_GREEDY | MRL_CNN_VALUE_ONLY)) {
        mrl::set_error("%s: flags 0x%x: only MRL_POLICY_GREEDY and %s exist", what, flags, only);
        return MRL_ERR_INVALID;
    }
    flags |= policy_flags;  // MRL_POLICY_GREEDY may travel with the policy (the rollouts have no flags of their own)
    if (flags & MRL_CNN_VALUE_ONLY ? (!record || row != record->num_steps) : (record && row >= record->num_steps)) {
        mrl::set_error("%s: row %u of %u; %s needs a record and row == num_steps, every other act row < num_steps", what, row,
                       record ? record->num_steps : 0u, only);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// the rows of `record` an act at `row` writes (value_only: the closing act at row T); `actions`: the width of a row of logits
template <class Record>
static void record_rows(mrl::ActArgs &a, const Record *record, uint32_t row, bool value_only, uint32_t actions)
{
    a.actions_row = nullptr, a.logprobs_row = a.values_row = a.rewards_row = a.dones_row = a.logits_row = nullptr;
    a.nets = 1u;
    if (!record) return;
    const size_t cells = (size_t)a.num_worlds * a.P;
    a.nets = value_only ? 2u : 3u;
    a.values_row = record->values + row * cells;
    a.rewards_row = row ? record->rewards + (row - 1) * cells : nullptr;
    a.dones_row = value_only ? record->next_done : record->dones + row * cells;
    if (value_only) return;
    a.actions_row = record->actions + row * cells;
    a.logprobs_row = record->logprobs + row * cells;
    a.logits_row = record->logits ? record->logits + row * cells * actions : nullptr;
}

// the seat mask against the simulator's P seats, then the part of the arguments every act carries
static int act_seats(mrl::ActArgs &a, const char *what, mrl_sim *sim, uint32_t players, uint32_t P, const mrl_tensor_desc &done,
                     const mrl_tensor_desc &action)
{
    if (players == 0 || (P < 32 && (players >> P) != 0)) {
        mrl::set_error("%s: players = 0x%x must name at least one seat and none beyond the simulator's %u", what, players, P);
        return MRL_ERR_INVALID;
    }
    a.done = static_cast<const int32_t *>(done.data);
    a.action = static_cast<int32_t *>(action.data);
    a.P = P, a.num_worlds = sim->num_worlds;
    a.players = players, a.num_seats = (uint32_t)__builtin_popcount(players);
    return MRL_OK;
}

// Everything mrl_cnn_act and mrl_rollout_cnn check alike; fills `args` but for the observation pointer, the rows and the step.
static int cnn_prepare(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, void *hip_stream,
                       const char *what, mrl::CnnActArgs *args)
{
    // the two kitchens export the same slab, flags and slot ids (Simplecooked's ExportID is Overcooked's list); the kernels take
    // W, H, F and P at run time, so F = 5P + 10 and P = 1 need nothing of their own
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (sim->game != MRL_GAME_OVERCOOKED && sim->game != MRL_GAME_SIMPLECOOKED) {
        mrl::set_error("%s: game %d has no CNN policy (Overcooked and Simplecooked do)", what, sim->game);
        return MRL_ERR_INVALID;
    }
    const char *sharded = "this simulator is a rank of an exchanged batch (mrl_exchange_create); sharded simulators are out of scope";
    if (int rc = act_scope_refusal(what, sim->exchange.mine ? sharded : nullptr, hip_stream)) return rc;
    if (!policy || !policy->params_dev || policy->hidden != mrl::kCnnHidden || (policy->flags & ~(uint32_t)MRL_POLICY_GREEDY)) {
        mrl::set_error("%s: null policy or parameter array, hidden other than 64, or policy flags other than MRL_POLICY_GREEDY", what);
        return MRL_ERR_INVALID;
    }
    if (int rc = act_record_refusal(what, record, true)) return rc;
    mrl_tensor_desc obs{}, done{}, reward{}, action{};
    int rc = mrl::guarded([&] {
        if (!sim->tensor(MRL_OVERCOOKED_OBS_WORLD_MAJOR, &obs) || !sim->tensor(MRL_OVERCOOKED_DONE, &done) ||
            !sim->tensor(MRL_OVERCOOKED_REWARD, &reward) || !sim->tensor(MRL_OVERCOOKED_ACTION, &action))
            throw std::runtime_error("the simulator does not export OBS_WORLD_MAJOR / DONE / REWARD / ACTION");
    });
    if (rc) return rc;
    const uint32_t P = (uint32_t)obs.shape[1], H = (uint32_t)obs.shape[2], W = (uint32_t)obs.shape[3], F = (uint32_t)obs.shape[4];
    if (W < 3 || H < 3) {
        mrl::set_error("%s: a %u x %u kitchen has no 3 x 3 patch", what, W, H);
        return MRL_ERR_INVALID;
    }
    mrl::CnnActArgs &a = *args;
    a = mrl::CnnActArgs{};
    if (int rc = act_seats(a, what, sim, players, P, done, action)) return rc;
    const mrl::CnnLds lds = mrl::cnn_lds(W, H, F);
    if (lds.total > mrl::kCnnLdsLimit) {
        mrl::set_error("%s: a %u x %u kitchen with %u channels needs an LDS image of %u bytes per workgroup, the limit is %u", what, W, H, F,
                       lds.total, mrl::kCnnLdsLimit);
        return MRL_ERR_INVALID;
    }
    a.params = policy->params_dev;
    a.reward = static_cast<const int32_t *>(reward.data);
    a.W = W, a.H = H, a.F = F;
    a.lds = lds;
    return MRL_OK;
}

// Everything mrl_mlpbase_act and mrl_rollout_mlpbase check alike; fills `args` but for the rows, the seed, the step and the flags.
static int mlpbase_prepare(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record,
                           void *hip_stream, const char *what, mrl::MlpBaseActArgs *args)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (sim->game != MRL_GAME_BALANCE) {
        mrl::set_error("%s: game %d has no MLPBase policy (the balance beam does)", what, sim->game);
        return MRL_ERR_INVALID;
    }
    const char *prepared = "this simulator has been through mrl_exchange_create or mrl_prepare_graph_capture; sharded and captured "
                           "simulators are out of scope";
    if (int rc = act_scope_refusal(what, sim->exchange.mine || sim->capturable() ? prepared : nullptr, hip_stream)) return rc;
    if (!policy || !policy->params_dev || policy->hidden != mrl::kMlpBaseHidden || policy->layer_N < 1 ||
        policy->layer_N > mrl::kMlpBaseMaxLayerN || (policy->flags & ~(uint32_t)MRL_POLICY_GREEDY)) {
        mrl::set_error("%s: null policy or parameter array, hidden other than 64, layer_N other than 1 or 2, or policy flags other than "
                       "MRL_POLICY_GREEDY", what);
        return MRL_ERR_INVALID;
    }
    if (int rc = act_record_refusal(what, record, record && record->obs)) return rc;
    uintptr_t low_bits = reinterpret_cast<uintptr_t>(policy->params_dev);
    if (record)
        for (const void *p : {(const void *)record->actions, (const void *)record->logprobs, (const void *)record->values,
                              (const void *)record->rewards, (const void *)record->dones, (const void *)record->next_done,
                              (const void *)record->logits, (const void *)record->obs})
            low_bits |= reinterpret_cast<uintptr_t>(p);
    if (low_bits & 3u) {
        mrl::set_error("%s: the parameter array and the record's arrays must start on 4-byte boundaries", what);
        return MRL_ERR_INVALID;
    }
    mrl_tensor_desc obs{}, done{}, reward{}, action{};
    int rc = mrl::guarded([&] {
        if (!sim->tensor(MRL_BALANCE_OBSERVATION, &obs) || !sim->tensor(MRL_BALANCE_DONE, &done) || !sim->tensor(MRL_BALANCE_REWARD, &reward) ||
            !sim->tensor(MRL_BALANCE_ACTION, &action))
            throw std::runtime_error("the simulator does not export OBSERVATION / DONE / REWARD / ACTION");
        if (obs.shape[2] != (int64_t)mrl::kMlpBaseObs || obs.dtype != MRL_INT32 || reward.dtype != MRL_FLOAT32 || action.dtype != MRL_INT32)
            throw std::runtime_error("unexpected tensor layout (OBSERVATION int32 (P, N, 7), REWARD float32, ACTION int32)");
    });
    if (rc) return rc;
    mrl::MlpBaseActArgs &a = *args;
    a = mrl::MlpBaseActArgs{};
    if (int rc = act_seats(a, what, sim, players, (uint32_t)obs.shape[0], done, action)) return rc;
    a.params = policy->params_dev;
    a.obs = static_cast<const int32_t *>(obs.data);
    a.reward = static_cast<const float *>(reward.data);
    a.layer_N = policy->layer_N;
    return MRL_OK;
}

// the rows of `record` an act at `row` writes: record_rows', and the row of observations every act copies
static void mlpbase_rows(mrl::MlpBaseActArgs &a, const mrl_mlpbase_record *record, uint32_t row, bool value_only)
{
    record_rows(a, record, row, value_only, mrl::kMlpBaseActions);
    a.obs_row = record ? record->obs + row * (size_t)a.num_worlds * a.P * mrl::kMlpBaseObs : nullptr;
}

// the two networks as a resample sees them
static const BankFamily kCnnFamily{1u << MRL_GAME_OVERCOOKED | 1u << MRL_GAME_SIMPLECOOKED, "no CNN policy (Overcooked and Simplecooked do)",
                                   MRL_OVERCOOKED_OBS_WORLD_MAJOR, 1, MRL_OVERCOOKED_DONE, "OBS_WORLD_MAJOR / DONE"};
static const BankFamily kMlpBaseFamily{1u << MRL_GAME_BALANCE, "no MLPBase policy (the balance beam does)",
                                       MRL_BALANCE_OBSERVATION, 0, MRL_BALANCE_DONE, "OBSERVATION / DONE"};

// ---- the bank updates' own refusals ----

// What mrl_mappo_bank_update and mrl_mappo_mlp_bank_update (`what`) refuse of the bank itself, `num_params` being one policy's
// parameter count; the plain calls' refusals follow on `first`, the bank's arrays as an mrl_mappo_optimizer.
static int mappo_bank_refusal(const char *what, const mrl_mappo_bank_optimizer *opt, uint64_t num_params, mrl_mappo_optimizer *first)
{
    if (!opt) {
        mrl::set_error("%s: null optimizer", what);
        return MRL_ERR_INVALID;
    }
    if (opt->num_policies == 0 || opt->num_policies > mrl::kBankMaxPolicies || opt->num_members == 0 ||
        (uint64_t)opt->first_member + opt->num_members > opt->num_policies) {
        mrl::set_error("%s: members [%u, %u + %u) of a bank of %u policies: a bank holds 1 to %u and the call trains at least one of them", what,
                       opt->first_member, opt->first_member, opt->num_members, opt->num_policies, mrl::kBankMaxPolicies);
        return MRL_ERR_INVALID;
    }
    if ((opt->row_bytes & 3u) || opt->row_bytes / 4u < num_params) {
        mrl::set_error("%s: row_bytes %llu: the bank's rows must lie a multiple of 4 bytes and at least %llu floats apart", what,
                       (unsigned long long)opt->row_bytes, (unsigned long long)num_params);
        return MRL_ERR_INVALID;
    }
    *first = mrl_mappo_optimizer{opt->params_dev, opt->exp_avg, opt->exp_avg_sq, opt->step};
    return MRL_OK;
}

// the first trained member's rows of the bank's arrays, the ValueNorm state included, and the member dimension of the launches
static mrl::MappoMembers mappo_bank_members(const mrl_mappo_bank_optimizer &opt, mrl_mappo_optimizer *first, float **value_norm_state)
{
    const uint64_t stride = opt.row_bytes / 4u, at = opt.first_member * stride;
    first->params_dev += at, first->exp_avg += at, first->exp_avg_sq += at;
    if (*value_norm_state) *value_norm_state += 3u * opt.first_member;
    return mrl::MappoMembers{opt.num_members, stride};
}

// ---- one description per network ----

// The kitchens' CNN: it reads the int8 observation slab (the live one, or a slot of the rollout's ring), takes a workspace to
// act, and its bank calls accept ids_row / ids_record wherever they lie.
struct CnnNet {
    using Policy = mrl_cnn_policy;
    using Bank = mrl_cnn_bank;
    using Record = mrl_cnn_record;
    using Args = CnnActArgs;
    using BankArgs = CnnBankArgs;
    static constexpr auto prepare = cnn_prepare;
    static constexpr auto launch_act = launch_cnn_act;
    static constexpr auto launch_act_bank = launch_cnn_act_bank;
    static constexpr const char *kValueOnly = "MRL_CNN_VALUE_ONLY";
    static constexpr uint32_t kValueOnlyBit = MRL_CNN_VALUE_ONLY;
    static constexpr const char *kBankSizer = "mrl_cnn_bank_workspace_bytes";
    static constexpr uintptr_t kIdsMask = 0;  // ids_row and ids_record may lie anywhere
    static constexpr const BankFamily &kFamily = kCnnFamily;

    static void rows(Args &a, const Record *record, uint32_t row, bool value_only) { record_rows(a, record, row, value_only, kCnnActions); }
    // `slot`: the ring's slot of a rollout's act, or nullptr for the simulator's live slab
    static void observe(Args &a, mrl_sim *sim, const char *what, const int8_t *slot)
    {
        a.obs = slot ? slot : static_cast<const int8_t *>(sim->observation_source());
        if (!a.obs) throw std::runtime_error(std::string(what) + ": the simulator has no observation slab");
    }
    // what is wrong with an act's workspace, or nullptr
    static const char *workspace_error(const Args &a, void *workspace_dev, uint64_t workspace_bytes)
    {
        const bool fits = workspace_dev && !(reinterpret_cast<uintptr_t>(workspace_dev) & 15u) &&
                          workspace_bytes >= mrl_cnn_workspace_bytes(a.num_worlds, a.P);
        return fits ? nullptr : "the workspace is null, off a 16-byte boundary or smaller than mrl_cnn_workspace_bytes";
    }
    // what a rollout lacks, or nullptr
    static const char *rollout_lacks(const Record *record, void *ring) { return record && ring ? nullptr : "null record or observation ring"; }
    // mrl_rollout_cnn and mrl_rollout_cnn_bank: rollout_loop with the simulator writing slot k + 1 of the observation ring in step k;
    // act(k, slot k, closing) reads its slot.
    template <class Act, class AfterStep>
    static int loop(mrl_sim *sim, const char *what, uint32_t T, void *obs_ring_dev, void *hip_stream, Act act, AfterStep after_step)
    {
        DeviceGuard on(sim->device);
        return guarded([&] {
            hipStream_t stream = (hipStream_t)hip_stream;
            const uint64_t slot_bytes = sim->observation_bytes();
            uint8_t *ring = static_cast<uint8_t *>(obs_ring_dev);
            const void *current = sim->observation_source();
            if (!current || !slot_bytes) throw std::runtime_error(std::string(what) + ": the simulator has no observation slab");
            if (current != ring) MRL_HIP(hipMemcpyAsync(ring, current, slot_bytes, hipMemcpyDeviceToDevice, stream));
            const mrl_sim::ObservationRing before = sim->observation_ring();
            struct HandBack {  // also when a launch throws
                mrl_sim *sim;
                const mrl_sim::ObservationRing &ring;
                bool armed;
                ~HandBack()
                {
                    if (armed) sim->restore_observation_ring(ring);
                }
            } hand_back{sim, before, T > 0};
            if (T) sim->set_observation_ring(ring + slot_bytes, slot_bytes, T);  // step k writes slot k + 1
            rollout_loop(
                sim, T, stream, [&](uint32_t k, bool closing) { act(k, reinterpret_cast<const int8_t *>(ring + (size_t)k * slot_bytes), closing); },
                after_step);
            if (T) {
                // the output goes back to where it pointed, and that place receives slot T: the simulator's observations are then
                // what T mrl_step_with_actions calls would have left there, and the next act or rollout reads them
                hand_back.armed = false;
                sim->restore_observation_ring(before);
                void *home = const_cast<void *>(sim->observation_source());
                const uint8_t *last = ring + (size_t)T * slot_bytes;
                if (home != last) MRL_HIP(hipMemcpyAsync(home, last, slot_bytes, hipMemcpyDeviceToDevice, stream));
            }
        });
    }
    static Policy row0(const Bank &bank) { return Policy{bank.params_dev, bank.hidden, bank.flags}; }
    static uint64_t bank_num_params(const Bank &, const Args &a) { return mrl_cnn_policy_num_params(a.W, a.H, a.F, kCnnHidden, kCnnActions); }

    // the update
    using UpdatePolicy = mrl_mappo_policy;
    using Batch = mrl_mappo_batch;
    static constexpr bool kObsWords = false;
    static constexpr auto update_workspace_bytes = mrl_mappo_workspace_bytes;
    static constexpr const char *kSizer = "mrl_mappo_workspace_bytes", *kBankUpdateSizer = "mrl_mappo_bank_workspace_bytes";
    static const char *shape_error(const UpdatePolicy &p, uint32_t minibatch_size, char *described, size_t room)
    {
        snprintf(described, room, "width %u, height %u, channels %u, hidden %u", p.width, p.height, p.channels, p.hidden);
        return mappo_shape_error(p.width, p.height, p.channels, p.hidden, minibatch_size);
    }
    static uint64_t actor_params(const UpdatePolicy &p) { return cnn_net_params(p.width, p.height, p.channels, kCnnActions); }
    static uint64_t workspace_floats(const UpdatePolicy &p, uint32_t B, uint32_t K) { return mappo_workspace(actor_params(p), B, K).total; }
    static uint64_t num_params(const UpdatePolicy &p) { return mrl_cnn_policy_num_params(p.width, p.height, p.channels, p.hidden, kCnnActions); }
    template <class... Rest> static void launch_update(const UpdatePolicy &p, Rest &&...rest) { launch_mappo_update(p, rest...); }
};

// The balance beam's MLPBase: it reads the simulator's OBSERVATION tensor in place and copies it into the record (obs_row),
// acts without a workspace, and its bank calls refuse ids_row / ids_record off a 4-byte boundary.
struct MlpBaseNet {
    using Policy = mrl_mlpbase_policy;
    using Bank = mrl_mlpbase_bank;
    using Record = mrl_mlpbase_record;
    using Args = MlpBaseActArgs;
    using BankArgs = MlpBaseBankArgs;
    static constexpr auto prepare = mlpbase_prepare;
    static constexpr auto rows = mlpbase_rows;
    static constexpr auto launch_act = launch_mlpbase_act;
    static constexpr auto launch_act_bank = launch_mlpbase_act_bank;
    static constexpr const char *kValueOnly = "MRL_MLPBASE_VALUE_ONLY";
    static constexpr uint32_t kValueOnlyBit = MRL_MLPBASE_VALUE_ONLY;
    static constexpr const char *kBankSizer = "mrl_mlpbase_bank_workspace_bytes";
    static constexpr uintptr_t kIdsMask = 3u;  // ids_row and ids_record are refused off a 4-byte boundary
    static constexpr const BankFamily &kFamily = kMlpBaseFamily;

    static void observe(Args &, mrl_sim *, const char *, const int8_t *) {}
    static const char *workspace_error(const Args &, void *, uint64_t) { return nullptr; }
    static const char *rollout_lacks(const Record *record, void *) { return record ? nullptr : "null record"; }
    template <class Act, class AfterStep>
    static int loop(mrl_sim *sim, const char *, uint32_t T, void *, void *hip_stream, Act act, AfterStep after_step)
    {
        DeviceGuard on(sim->device);
        return guarded([&] {
            rollout_loop(sim, T, (hipStream_t)hip_stream, [&](uint32_t k, bool closing) { act(k, nullptr, closing); }, after_step);
        });
    }
    static Policy row0(const Bank &bank) { return Policy{bank.params_dev, bank.hidden, bank.layer_N, bank.flags}; }
    static uint64_t bank_num_params(const Bank &bank, const Args &)
    {
        return mrl_mlpbase_policy_num_params(kMlpBaseObs, kMlpBaseHidden, bank.layer_N, kMlpBaseActions);
    }

    // the update
    using UpdatePolicy = mrl_mlpbase_policy;
    using Batch = mrl_mappo_mlp_batch;
    static constexpr bool kObsWords = true;
    static constexpr auto update_workspace_bytes = mrl_mappo_mlp_workspace_bytes;
    static constexpr const char *kSizer = "mrl_mappo_mlp_workspace_bytes", *kBankUpdateSizer = "mrl_mappo_mlp_bank_workspace_bytes";
    static const char *shape_error(const UpdatePolicy &p, uint32_t minibatch_size, char *described, size_t room)
    {
        snprintf(described, room, "hidden %u, layer_N %u", p.hidden, p.layer_N);
        return mappo_mlp_shape_error(kMlpBaseObs, p.hidden, p.layer_N, kMlpBaseActions, minibatch_size);
    }
    static uint64_t actor_params(const UpdatePolicy &p) { return (uint64_t)mlpbase_net_params(p.layer_N, kMlpBaseActions); }
    static uint64_t workspace_floats(const UpdatePolicy &p, uint32_t B, uint32_t K) { return mappo_workspace(actor_params(p), B, K).total; }
    static uint64_t num_params(const UpdatePolicy &p) { return mrl_mlpbase_policy_num_params(kMlpBaseObs, p.hidden, p.layer_N, kMlpBaseActions); }
    template <class... Rest> static void launch_update(const UpdatePolicy &p, Rest &&...rest) { launch_mappo_mlp_update(p.layer_N, rest...); }
};

// The recurrent MLPBase as the update sees it (mrl_mappo_mlp_update with MRL_MLPBASE_RECURRENT): MlpBaseNet's refusals on the
// structs the extended ones begin with; the rows are chunk ids, the workspace and the launch the recurrent update's.
struct MlpBaseGruNet : MlpBaseNet {
    static uint64_t actor_params(const UpdatePolicy &p) { return (uint64_t)gru_net_params(p.layer_N, kMlpBaseActions); }
    static uint64_t num_params(const UpdatePolicy &p) { return (uint64_t)gru_net_params(p.layer_N, kMlpBaseActions) + gru_net_params(p.layer_N, 1); }
    static uint64_t workspace_floats(const UpdatePolicy &p, uint32_t Bc, uint32_t K) { return gru_update_workspace(p.layer_N, Bc, K).total; }
    // `batch` is the first member of the mrl_mappo_mlp_gru_batch that gru_update checked
    static void launch_update(const UpdatePolicy &p, const mrl_mappo_optimizer &opt, const Batch &batch, const int32_t *indices, uint32_t K,
                              uint32_t Bc, const mrl_mappo_config &cfg, float *value_norm_state, float *workspace, float *stats, float *grads,
                              hipStream_t stream, const MappoMembers &)
    {
        launch_mappo_gru_update(p.layer_N, opt, reinterpret_cast<const mrl_mappo_mlp_gru_batch &>(batch), indices, K, Bc, cfg, value_norm_state,
                                workspace, stats, grads, stream);
    }
};

// ---- act and rollout, plain and over a bank ----

// `why`, a check's verdict, refuses the call `what` unless it is nullptr
static int refusal(const char *what, const char *why)
{
    if (why) set_error("%s: %s", what, why);
    return why ? MRL_ERR_INVALID : MRL_OK;
}

// Everything the act and the rollout of a bank check alike: the network's own checks with row 0 of the bank as the policy, which
// fill args->act; then bank_refusal with the floats of one policy and the name of the network's sizer.  Fills args->bank but for
// the ids row.
template <class Net>
static int bank_prepare(const char *what, mrl_sim *sim, uint32_t players, const typename Net::Bank *bank, const int32_t *ids_dev,
                        const typename Net::Record *record, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream,
                        typename Net::BankArgs *args)
{
    if (int rc = refusal(what, bank ? nullptr : "null bank")) return rc;
    const typename Net::Policy row0 = Net::row0(*bank);
    if (int rc = Net::prepare(sim, players, &row0, record, hip_stream, what, &args->act)) return rc;
    const ActArgs &a = args->act;
    if (int rc = bank_refusal(what, a.num_worlds, a.P, bank->num_policies, bank->stride, Net::bank_num_params(*bank, args->act), ids_dev,
                              workspace_dev, workspace_bytes, mrl_cnn_bank_workspace_bytes(a.num_worlds, a.P, bank->num_policies), Net::kBankSizer))
        return rc;
    args->bank = BankActArgs{ids_dev, nullptr, static_cast<uint32_t *>(workspace_dev), bank->stride, bank->num_policies};
    return MRL_OK;
}

// what every act fills behind the checks: where it reads (observe), the record's rows it writes, its seed, step and flags
template <class Net>
static void fill(typename Net::Args &a, mrl_sim *sim, const char *what, const int8_t *slot, const typename Net::Record *record, uint32_t row,
                 uint64_t seed, uint32_t step, uint32_t flags)
{
    Net::observe(a, sim, what, slot);
    Net::rows(a, record, row, flags & Net::kValueOnlyBit);
    a.seed = seed, a.step = step, a.flags = flags;
}

template <class Net>
static int act(const char *what, mrl_sim *sim, uint32_t players, const typename Net::Policy *policy, const typename Net::Record *record,
               uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    typename Net::Args args{};
    if (int rc = Net::prepare(sim, players, policy, record, hip_stream, what, &args)) return rc;
    if (int rc = act_row_refusal(what, Net::kValueOnly, flags, policy->flags, record, row)) return rc;
    if (int rc = refusal(what, Net::workspace_error(args, workspace_dev, workspace_bytes))) return rc;
    DeviceGuard on(sim->device);
    return guarded([&] {
        fill<Net>(args, sim, what, nullptr, record, row, seed, step, flags);
        Net::launch_act(args, (hipStream_t)hip_stream);
    });
}

template <class Net>
static int act_bank(const char *what, mrl_sim *sim, uint32_t players, const typename Net::Bank *bank, const int32_t *ids_dev,
                    const typename Net::Record *record, int32_t *ids_row, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags,
                    void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    typename Net::BankArgs args{};
    if (int rc = bank_prepare<Net>(what, sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, &args)) return rc;
    if (int rc = act_row_refusal(what, Net::kValueOnly, flags, bank->flags, record, row)) return rc;
    if (int rc = refusal(what, reinterpret_cast<uintptr_t>(ids_row) & Net::kIdsMask ? "ids_row is off a 4-byte boundary" : nullptr)) return rc;
    args.bank.ids_row = ids_row;
    DeviceGuard on(sim->device);
    return guarded([&] {
        fill<Net>(args.act, sim, what, nullptr, record, row, seed, step, flags);
        Net::launch_act_bank(args, (hipStream_t)hip_stream);
    });
}

template <class Net>
static int rollout(const char *what, mrl_sim *sim, uint32_t players, const typename Net::Policy *policy, const typename Net::Record *record,
                   void *obs_ring_dev, uint64_t seed, uint32_t first_step, void *hip_stream)
{
    typename Net::Args args{};
    if (int rc = Net::prepare(sim, players, policy, record, hip_stream, what, &args)) return rc;
    if (int rc = refusal(what, Net::rollout_lacks(record, obs_ring_dev))) return rc;
    return Net::loop(
        sim, what, record->num_steps, obs_ring_dev, hip_stream,
        [&](uint32_t k, const int8_t *slot, bool closing) {
            fill<Net>(args, sim, what, slot, record, k, seed, first_step + k, policy->flags | (closing ? Net::kValueOnlyBit : 0u));
            Net::launch_act(args, (hipStream_t)hip_stream);
        },
        [] {});
}

// ---- the recurrent MLPBase: mrl_mlpbase_act and mrl_rollout_mlpbase with MRL_MLPBASE_RECURRENT in the policy's flags ----

// Everything the recurrent act and rollout check alike: mrl_mlpbase_act's own checks on the base structs (the bit taken out:
// to every other caller of mlpbase_prepare, the banks included, it stays an unknown policy flag), then the state and h0 arrays.
static int gru_prepare(mrl_sim *sim, uint32_t players, const mrl_mlpbase_gru_policy *policy, const mrl_mlpbase_gru_record *record,
                       void *hip_stream, const char *what, MlpBaseGruActArgs *args, mrl_mlpbase_policy *plain)
{
    *plain = policy->base;
    plain->flags &= ~(uint32_t)MRL_MLPBASE_RECURRENT;
    if (int rc = mlpbase_prepare(sim, players, plain, record ? &record->base : nullptr, hip_stream, what, &args->act)) return rc;
    if (!policy->h_actor || !policy->h_critic || ((reinterpret_cast<uintptr_t>(policy->h_actor) | reinterpret_cast<uintptr_t>(policy->h_critic)) & 3u))
        return refusal(what, "a recurrent policy needs h_actor and h_critic, each on a 4-byte boundary");
    if (record) {
        if (record->chunk_length == 0 || record->base.num_steps % record->chunk_length != 0)
            return refusal(what, "a recurrent record needs chunk_length >= 1 that divides num_steps");
        if (!record->h0_actor || !record->h0_critic ||
            ((reinterpret_cast<uintptr_t>(record->h0_actor) | reinterpret_cast<uintptr_t>(record->h0_critic)) & 3u))
            return refusal(what, "a recurrent record needs h0_actor and h0_critic, each on a 4-byte boundary");
    }
    args->h[0] = policy->h_actor, args->h[1] = policy->h_critic;
    return MRL_OK;
}

// what a recurrent act fills behind the checks: the plain act's rows, seed, step and flags, then the h0 rows and the write-back
static void gru_fill(MlpBaseGruActArgs &g, const mrl_mlpbase_gru_record *record, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags)
{
    const bool value_only = flags & MRL_MLPBASE_VALUE_ONLY;
    mlpbase_rows(g.act, record ? &record->base : nullptr, row, value_only);
    g.act.seed = seed, g.act.step = step, g.act.flags = flags;
    g.write_state = value_only ? 0u : 1u;
    g.h0_row[0] = g.h0_row[1] = nullptr;
    if (record && !value_only && row % record->chunk_length == 0) {
        const size_t at = (size_t)(row / record->chunk_length) * g.act.num_worlds * g.act.P * kMlpBaseHidden;
        g.h0_row[0] = record->h0_actor + at, g.h0_row[1] = record->h0_critic + at;
    }
}

static int gru_act(const char *what, mrl_sim *sim, uint32_t players, const mrl_mlpbase_gru_policy *policy, const mrl_mlpbase_gru_record *record,
                   uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *hip_stream)
{
    MlpBaseGruActArgs args{};
    mrl_mlpbase_policy plain{};
    if (int rc = gru_prepare(sim, players, policy, record, hip_stream, what, &args, &plain)) return rc;
    if (int rc = act_row_refusal(what, MlpBaseNet::kValueOnly, flags, plain.flags, record ? &record->base : nullptr, row)) return rc;
    DeviceGuard on(sim->device);
    return guarded([&] {
        gru_fill(args, record, row, seed, step, flags);
        launch_mlpbase_gru_act(args, (hipStream_t)hip_stream);
    });
}

static int gru_rollout(const char *what, mrl_sim *sim, uint32_t players, const mrl_mlpbase_gru_policy *policy, const mrl_mlpbase_gru_record *record,
                       uint64_t seed, uint32_t first_step, void *hip_stream)
{
    MlpBaseGruActArgs args{};
    mrl_mlpbase_policy plain{};
    if (int rc = gru_prepare(sim, players, policy, record, hip_stream, what, &args, &plain)) return rc;
    if (int rc = refusal(what, record ? nullptr : "null record")) return rc;
    DeviceGuard on(sim->device);
    return guarded([&] {
        rollout_loop(
            sim, record->base.num_steps, (hipStream_t)hip_stream,
            [&](uint32_t k, bool closing) {
                gru_fill(args, record, k, seed, first_step + k, plain.flags | (closing ? (uint32_t)MRL_MLPBASE_VALUE_ONLY : 0u));
                launch_mlpbase_gru_act(args, (hipStream_t)hip_stream);
            },
            [] {});
    });
}

template <class Net>
static int rollout_bank(const char *what, mrl_sim *sim, uint32_t players, const typename Net::Bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                        const mrl_cnn_resample *resample, const typename Net::Record *record, int32_t *ids_record, void *obs_ring_dev,
                        uint64_t seed, uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    typename Net::BankArgs args{};
    if (int rc = bank_prepare<Net>(what, sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, &args)) return rc;
    if (int rc = refusal(what, Net::rollout_lacks(record, obs_ring_dev))) return rc;
    if (int rc = refusal(what, reinterpret_cast<uintptr_t>(ids_record) & Net::kIdsMask ? "ids_record is off a 4-byte boundary" : nullptr)) return rc;
    CnnResampleArgs again{};
    if (resample)
        if (int rc = bank_resample_prepare(sim, Net::kFamily, players, resample, ids_dev, episodes_dev, what, &again)) return rc;
    const size_t cells = (size_t)args.act.num_worlds * args.act.P;
    return Net::loop(
        sim, what, record->num_steps, obs_ring_dev, hip_stream,
        [&](uint32_t k, const int8_t *slot, bool closing) {
            fill<Net>(args.act, sim, what, slot, record, k, seed, first_step + k, bank->flags | (closing ? Net::kValueOnlyBit : 0u));
            args.bank.ids_row = ids_record ? ids_record + (size_t)k * cells : nullptr;
            Net::launch_act_bank(args, (hipStream_t)hip_stream);
        },
        [&] {
            if (resample) launch_cnn_bank_resample(again, (hipStream_t)hip_stream);
        });
}

// ---- the update, plain and over a bank ----

// One body for mrl_mappo_update, mrl_mappo_mlp_update (Opt: mrl_mappo_optimizer) and their bank forms (mrl_mappo_bank_optimizer).
// A bank's own refusals come first and hand on the bank's arrays as an optimizer, `first`; behind the common refusals `first`
// moves to the first trained member's rows and the launches get their member dimension.  Of the network: Net::shape_error
// returns why the shape cannot run, or nullptr, and describes the shape for the message; Net::actor_params is the actor's
// parameter count; Net::kObsWords: the batch's observations are 4-byte words, to be checked with the other arrays.
template <class Net, class Opt>
static int mappo_update(const char *what, const typename Net::UpdatePolicy *policy, const Opt *bank_or_opt, const typename Net::Batch *batch,
                        const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                        float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null,
                        int gpu_id, void *hip_stream)
{
    constexpr bool kBank = std::is_same<Opt, mrl_mappo_bank_optimizer>::value;
    mrl_mappo_optimizer first{};
    const mrl_mappo_optimizer *opt = &first;
    uint32_t members = 1;  // the workspace must hold that many plain ones
    if constexpr (kBank) {
        if (int rc = mappo_bank_refusal(what, bank_or_opt, policy ? Net::num_params(*policy) : 0, &first)) return rc;
        members = bank_or_opt->num_members;
    } else {
        opt = bank_or_opt;
    }
    if (!policy || !opt || !batch || (!indices_dev && num_minibatches) || !cfg || !workspace_dev) {  // (no rows: no index array)
        mrl::set_error("%s: null policy, optimizer, batch, index array, configuration or workspace", what);
        return MRL_ERR_INVALID;
    }
    if (!policy->params_dev || !opt->params_dev || !opt->exp_avg || !opt->exp_avg_sq || !batch->obs || !batch->actions || !batch->logprobs ||
        !batch->value_preds || !batch->returns || !batch->advantages) {
        mrl::set_error("%s: null parameter, moment or batch array", what);
        return MRL_ERR_INVALID;
    }
    if (policy->params_dev != opt->params_dev) {
        mrl::set_error("%s: the policy's and the optimizer's params_dev must be the same array", what);
        return MRL_ERR_INVALID;
    }
    if (cfg->flags & ~mrl::kMappoKnownFlags) {
        mrl::set_error("%s: flags 0x%x: only the four MRL_MAPPO_* bits exist", what, cfg->flags);
        return MRL_ERR_INVALID;
    }
    if ((cfg->flags & MRL_MAPPO_VALUENORM) && !value_norm_state) {
        mrl::set_error("%s: MRL_MAPPO_VALUENORM needs value_norm_state", what);
        return MRL_ERR_INVALID;
    }
    char described[96];
    const char *why = Net::shape_error(*policy, minibatch_size, described, sizeof described);
    if (why || batch->size == 0) {
        mrl::set_error("%s: %s (%s, minibatch_size %u, batch size %u)", what, why ? why : "the batch must hold at least one sample", described,
                       minibatch_size, batch->size);
        return MRL_ERR_INVALID;
    }
    const uint64_t need_bytes = members * Net::workspace_floats(*policy, minibatch_size, num_minibatches) * sizeof(float);
    const void *words[] = {opt->params_dev, opt->exp_avg, opt->exp_avg_sq, Net::kObsWords ? batch->obs : nullptr, batch->actions, batch->logprobs,
                           batch->value_preds, batch->returns, batch->advantages, indices_dev, value_norm_state, stats_dev_or_null,
                           grads_dev_or_null};
    uintptr_t low_bits = 0;
    for (const void *p : words) low_bits |= reinterpret_cast<uintptr_t>(p) & 3u;
    if (int rc = update_refusal(what, kBank ? Net::kBankUpdateSizer : Net::kSizer, workspace_bytes, need_bytes, workspace_dev, low_bits,
                                "the float and int32 arrays must start on 4-byte boundaries", hip_stream))
        return rc;
    MappoMembers launch_members = kMappoOneMember;
    if constexpr (kBank) launch_members = mappo_bank_members(*bank_or_opt, &first, &value_norm_state);
    DeviceGuard on(gpu_id);
    return guarded([&] {
        Net::launch_update(*policy, *opt, *batch, indices_dev, num_minibatches, minibatch_size, *cfg, value_norm_state,
                           static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream, launch_members);
    });
}

// mrl_mappo_mlp_update with MRL_MLPBASE_RECURRENT: what the extended batch adds is checked here, the rest by mappo_update on the
// structs the extended ones begin with (the policy's state pointers are not read: every chunk starts from the batch's h0)
static int gru_update(const char *what, const mrl_mlpbase_gru_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_mlp_gru_batch *batch,
                      const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                      float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null,
                      int gpu_id, void *hip_stream)
{
    if (batch) {
        const uintptr_t low_bits = reinterpret_cast<uintptr_t>(batch->h0_actor) | reinterpret_cast<uintptr_t>(batch->h0_critic) |
                                   reinterpret_cast<uintptr_t>(batch->dones);
        if (!batch->h0_actor || !batch->h0_critic || !batch->dones || (low_bits & 3u))
            return refusal(what, "a recurrent batch needs h0_actor, h0_critic and dones, each on a 4-byte boundary");
        if (batch->chunk_length == 0 || batch->chunk_length > kGruMaxChunk) {
            set_error("%s: chunk_length %u: the update runs chunks of 1 to %u steps", what, batch->chunk_length, kGruMaxChunk);
            return MRL_ERR_INVALID;
        }
        const uint64_t row = (uint64_t)batch->chunk_length * batch->num_worlds * batch->num_seats;
        if (row == 0 || batch->base.size % row != 0) {
            set_error("%s: a batch of %u samples is not a whole number of rows of %u-step chunks of %u worlds and %u seats", what,
                      batch->base.size, batch->chunk_length, batch->num_worlds, batch->num_seats);
            return MRL_ERR_INVALID;
        }
        if (minibatch_size > batch->base.size / batch->chunk_length) {  // (so that Bc L, a row's samples, is at most the batch's size)
            set_error("%s: minibatch_size %u: a row holds chunk ids, and the batch has %u chunks", what, minibatch_size,
                      batch->base.size / batch->chunk_length);
            return MRL_ERR_INVALID;
        }
    }
    mrl_mlpbase_policy plain{};
    if (policy) plain = policy->base;
    return mappo_update<MlpBaseGruNet>(what, policy ? &plain : nullptr, opt, batch ? &batch->base : nullptr, indices_dev, num_minibatches,
                                       minibatch_size, cfg, value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null,
                                       grads_dev_or_null, gpu_id, hip_stream);
}

// mrl_mappo_bank_workspace_bytes and mrl_mappo_mlp_bank_workspace_bytes (`what`): the plain update's workspace, once per member
template <class Net>
static int bank_workspace_bytes(const char *what, uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3, uint32_t minibatch_size,
                                uint32_t num_minibatches, uint32_t num_members, uint64_t *out)
{
    if (num_members == 0 || num_members > kBankMaxPolicies) {
        set_error("%s: %u members: a call trains 1 to %u", what, num_members, kBankMaxPolicies);
        return MRL_ERR_INVALID;
    }
    if (int rc = Net::update_workspace_bytes(s0, s1, s2, s3, minibatch_size, num_minibatches, out)) return rc;
    *out *= num_members;
    return MRL_OK;
}

}  // namespace mrl

using mrl::CnnNet;
using mrl::MlpBaseNet;

extern "C" {

uint64_t mrl_cnn_policy_num_params(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t num_actions)
{
    if (hidden != mrl::kCnnHidden || num_actions != mrl::kCnnActions || width < 3 || height < 3 || channels == 0) return 0;
    return mrl::cnn_net_params(width, height, channels, num_actions) + mrl::cnn_net_params(width, height, channels, 1);
}

uint64_t mrl_cnn_workspace_bytes(uint32_t num_worlds, uint32_t num_players) { return mrl::kCnnWorkspaceBytes; }

uint64_t mrl_mlpbase_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions)
{
    // the recurrent shape: layer_N + MRL_MLPBASE_GRU_LAYERS
    const uint32_t gru = layer_N - MRL_MLPBASE_GRU_LAYERS;
    if (obs_dim == mrl::kMlpBaseObs && hidden == mrl::kMlpBaseHidden && gru >= 1 && gru <= mrl::kMlpBaseMaxLayerN && num_actions == mrl::kMlpBaseActions)
        return (uint64_t)mrl::gru_net_params(gru, num_actions) + mrl::gru_net_params(gru, 1);
    if (obs_dim != mrl::kMlpBaseObs || hidden != mrl::kMlpBaseHidden || layer_N < 1 || layer_N > mrl::kMlpBaseMaxLayerN ||
        num_actions != mrl::kMlpBaseActions)
        return 0;
    return (uint64_t)mrl::mlpbase_net_params(layer_N, num_actions) + mrl::mlpbase_net_params(layer_N, 1);
}

uint64_t mrl_cnn_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_players, uint32_t num_policies)
{
    if (num_policies == 0 || num_policies > mrl::kBankMaxPolicies) return 0;
    return mrl::bank_layout(num_worlds, num_players, num_policies).words * sizeof(uint32_t);
}

uint64_t mrl_mlpbase_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_policies)
{
    return mrl_cnn_bank_workspace_bytes(num_worlds, 2, num_policies);  // the balance beam seats two
}

int mrl_mappo_workspace_bytes(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size,
                              uint32_t num_minibatches, uint64_t *out)
{
    const char *why = out ? mappo_shape_error(width, height, channels, hidden, minibatch_size) : "null output pointer";
    if (why) {
        mrl::set_error("mrl_mappo_workspace_bytes: %s (width %u, height %u, channels %u, hidden %u, minibatch_size %u)", why, width, height,
                       channels, hidden, minibatch_size);
        return MRL_ERR_INVALID;
    }
    *out = mrl::mappo_workspace(mrl::cnn_net_params(width, height, channels, mrl::kCnnActions), minibatch_size, num_minibatches).total *
           sizeof(float);
    return MRL_OK;
}

int mrl_mappo_mlp_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                  uint32_t num_minibatches, uint64_t *out)
{
    // the recurrent shape: layer_N + MRL_MLPBASE_GRU_LAYERS
    const uint32_t gru = layer_N - MRL_MLPBASE_GRU_LAYERS;
    if (out && gru >= 1 && gru <= mrl::kMlpBaseMaxLayerN && !mappo_mlp_shape_error(obs_dim, hidden, gru, num_actions, minibatch_size)) {
        *out = mrl::gru_update_workspace(gru, minibatch_size, num_minibatches).total * sizeof(float);
        return MRL_OK;
    }
    const char *why = out ? mappo_mlp_shape_error(obs_dim, hidden, layer_N, num_actions, minibatch_size) : "null output pointer";
    if (why) {
        mrl::set_error("mrl_mappo_mlp_workspace_bytes: %s (obs_dim %u, hidden %u, layer_N %u, num_actions %u, minibatch_size %u)", why, obs_dim,
                       hidden, layer_N, num_actions, minibatch_size);
        return MRL_ERR_INVALID;
    }
    *out = mrl::mappo_workspace(mrl::mlpbase_net_params(layer_N, num_actions), minibatch_size, num_minibatches).total * sizeof(float);
    return MRL_OK;
}

int mrl_cnn_act(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, uint32_t row, uint64_t seed,
                uint32_t step, uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    return mrl::act<CnnNet>("mrl_cnn_act", sim, players, policy, record, row, seed, step, flags, workspace_dev, workspace_bytes, hip_stream);
}

int mrl_mlpbase_act(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record, uint32_t row,
                    uint64_t seed, uint32_t step, uint32_t flags, void *hip_stream)
{
    if (policy && (policy->flags & MRL_MLPBASE_RECURRENT))
        return mrl::gru_act("mrl_mlpbase_act", sim, players, reinterpret_cast<const mrl_mlpbase_gru_policy *>(policy),
                            reinterpret_cast<const mrl_mlpbase_gru_record *>(record), row, seed, step, flags, hip_stream);
    return mrl::act<MlpBaseNet>("mrl_mlpbase_act", sim, players, policy, record, row, seed, step, flags, nullptr, 0, hip_stream);
}

int mrl_cnn_act_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, const int32_t *ids_dev, const mrl_cnn_record *record,
                     int32_t *ids_row, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev,
                     uint64_t workspace_bytes, void *hip_stream)
{
    return mrl::act_bank<CnnNet>("mrl_cnn_act_bank", sim, players, bank, ids_dev, record, ids_row, row, seed, step, flags, workspace_dev,
                                 workspace_bytes, hip_stream);
}

int mrl_mlpbase_act_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, const int32_t *ids_dev,
                         const mrl_mlpbase_record *record, int32_t *ids_row, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags,
                         void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    return mrl::act_bank<MlpBaseNet>("mrl_mlpbase_act_bank", sim, players, bank, ids_dev, record, ids_row, row, seed, step, flags, workspace_dev,
                                     workspace_bytes, hip_stream);
}

int mrl_rollout_cnn(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, void *obs_ring_dev,
                    uint64_t seed, uint32_t first_step, void *hip_stream)
{
    return mrl::rollout<CnnNet>("mrl_rollout_cnn", sim, players, policy, record, obs_ring_dev, seed, first_step, hip_stream);
}

int mrl_rollout_mlpbase(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record, uint64_t seed,
                        uint32_t first_step, void *hip_stream)
{
    if (policy && (policy->flags & MRL_MLPBASE_RECURRENT))
        return mrl::gru_rollout("mrl_rollout_mlpbase", sim, players, reinterpret_cast<const mrl_mlpbase_gru_policy *>(policy),
                                reinterpret_cast<const mrl_mlpbase_gru_record *>(record), seed, first_step, hip_stream);
    return mrl::rollout<MlpBaseNet>("mrl_rollout_mlpbase", sim, players, policy, record, nullptr, seed, first_step, hip_stream);
}

int mrl_rollout_cnn_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                         const mrl_cnn_resample *resample, const mrl_cnn_record *record, int32_t *ids_record, void *obs_ring_dev, uint64_t seed,
                         uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    return mrl::rollout_bank<CnnNet>("mrl_rollout_cnn_bank", sim, players, bank, ids_dev, episodes_dev, resample, record, ids_record, obs_ring_dev,
                                     seed, first_step, workspace_dev, workspace_bytes, hip_stream);
}

int mrl_rollout_mlpbase_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                             const mrl_cnn_resample *resample, const mrl_mlpbase_record *record, int32_t *ids_record, uint64_t seed,
                             uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    return mrl::rollout_bank<MlpBaseNet>("mrl_rollout_mlpbase_bank", sim, players, bank, ids_dev, episodes_dev, resample, record, ids_record,
                                         nullptr, seed, first_step, workspace_dev, workspace_bytes, hip_stream);
}

int mrl_cnn_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                          void *hip_stream)
{
    return mrl::bank_resample(sim, mrl::kCnnFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_cnn_bank_resample");
}

int mrl_mlpbase_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                              void *hip_stream)
{
    return mrl::bank_resample(sim, mrl::kMlpBaseFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_mlpbase_bank_resample");
}

int mrl_mappo_update(const mrl_mappo_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_batch *batch, const int32_t *indices_dev,
                     uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg, float *value_norm_state, void *workspace_dev,
                     uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    return mrl::mappo_update<CnnNet>("mrl_mappo_update", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg, value_norm_state,
                                     workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, gpu_id, hip_stream);
}

int mrl_mappo_bank_update(const mrl_mappo_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_batch *batch, const int32_t *indices_dev,
                          uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg, float *value_norm_state, void *workspace_dev,
                          uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    return mrl::mappo_update<CnnNet>("mrl_mappo_bank_update", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg,
                                     value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, gpu_id, hip_stream);
}

int mrl_mappo_mlp_update(const mrl_mlpbase_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_mlp_batch *batch, const int32_t *indices_dev,
                         uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg, float *value_norm_state, void *workspace_dev,
                         uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    if (policy && (policy->flags & MRL_MLPBASE_RECURRENT))
        return mrl::gru_update("mrl_mappo_mlp_update", reinterpret_cast<const mrl_mlpbase_gru_policy *>(policy), opt,
                               reinterpret_cast<const mrl_mappo_mlp_gru_batch *>(batch), indices_dev, num_minibatches, minibatch_size, cfg,
                               value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, gpu_id, hip_stream);
    return mrl::mappo_update<MlpBaseNet>("mrl_mappo_mlp_update", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg,
                                         value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, gpu_id, hip_stream);
}

int mrl_mappo_mlp_bank_update(const mrl_mlpbase_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_mlp_batch *batch,
                              const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                              float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                              float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    if (policy && (policy->flags & MRL_MLPBASE_RECURRENT))
        return mrl::refusal("mrl_mappo_mlp_bank_update", "a bank update does not take a recurrent policy (MRL_MLPBASE_RECURRENT)");
    return mrl::mappo_update<MlpBaseNet>("mrl_mappo_mlp_bank_update", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg,
                                         value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, gpu_id, hip_stream);
}

int mrl_mappo_bank_workspace_bytes(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size,
                                   uint32_t num_minibatches, uint32_t num_members, uint64_t *out)
{
    return mrl::bank_workspace_bytes<CnnNet>("mrl_mappo_bank_workspace_bytes", width, height, channels, hidden, minibatch_size, num_minibatches,
                                             num_members, out);
}

int mrl_mappo_mlp_bank_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                       uint32_t num_minibatches, uint32_t num_members, uint64_t *out)
{
    return mrl::bank_workspace_bytes<MlpBaseNet>("mrl_mappo_mlp_bank_workspace_bytes", obs_dim, hidden, layer_N, num_actions, minibatch_size,
                                                 num_minibatches, num_members, out);
}

}  // extern "C"
