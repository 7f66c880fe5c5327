// The C API of the wide agent (include/mrl_envs.h, mrl_agent_*): act, credit, GAE over active steps, the update, and the bank
// act with its resample.  It acts per player on its own tensors, so it shares bank_refusal and BankFamily with MAPPO's two
// networks (capi_internal.hpp) and nothing else.
#include "capi_internal.hpp"
#include "wide_policy.hpp"
#include "wide_bank.hpp"
#include "wide_update.hpp"

using mrl::guarded;
using mrl::update_refusal;

extern "C" {

uint64_t mrl_wide_policy_num_params(uint32_t obs_dim, uint32_t state_dim, uint32_t num_actions)
{
    return mrl::wide_net_params(state_dim, 1) + mrl::wide_net_params(obs_dim, num_actions);
}

uint64_t mrl_agent_workspace_bytes(uint32_t num_worlds) { return mrl::wide_workspace_bytes(num_worlds); }

static bool agent_record_complete(const mrl_agent_record *r)
{
    return r->obs && r->states && r->action_masks && r->active && r->actions && r->logprobs && r->values && r->dones && r->rewards &&
           r->last_active && r->new_game && r->next_done && r->running_rewards && r->totals && r->next_value && r->next_active &&
           r->first_step;
}

// player p's (N, width) slice of a (P, N, width) tensor, or its (N) slice of a (P, N) one
static mrl::WideInput agent_slice(const mrl_tensor_desc &d, uint32_t player)
{
    const int64_t bytes = d.dtype == MRL_INT8 || d.dtype == MRL_UINT8 ? 1 : 4;
    mrl::WideInput in{};
    in.data = static_cast<const char *>(d.data) + (int64_t)player * d.strides[0] * bytes;
    in.row_stride = d.strides[1];
    in.type = (uint32_t)d.dtype;
    return in;
}

// Everything mrl_agent_act and mrl_agent_act_bank check alike of the simulator, the seat and the policy's shape (`policy`: for the
// bank its row 0); fills `args` but for the record, the row, the step, the flags, the seed and the workspace; *seats: the
// simulator's seats.
static int agent_prepare(mrl_sim *sim, uint32_t player, const mrl_wide_policy *policy, void *workspace_dev, void *hip_stream, const char *what,
                         mrl::AgentActArgs *out, uint32_t *seats = nullptr)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, what)) return rc;
    if (sim->game != MRL_GAME_HANABI && sim->game != MRL_GAME_BALANCE) {
        mrl::set_error("%s: game %d has no wide-policy agent (Hanabi and the balance beam do)", what, sim->game);
        return MRL_ERR_INVALID;
    }
    if (sim->exchange.mine) {
        mrl::set_error("%s: this simulator is a rank of an exchanged batch (mrl_exchange_create); sharded simulators are out of scope", what);
        return MRL_ERR_INVALID;
    }
    if (!policy || !policy->params_dev || !workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) {
        mrl::set_error("%s: null policy or parameter array, or a workspace that is null or off a 16-byte boundary", what);
        return MRL_ERR_INVALID;
    }
    if (policy->num_actions == 0 || policy->num_actions > MRL_WIDE_MAX_ACTIONS || policy->obs_dim == 0 || policy->state_dim == 0) {
        mrl::set_error("%s: need 1 <= num_actions <= %d and obs_dim, state_dim >= 1; got num_actions %u, obs_dim %u, state_dim %u", what,
                       MRL_WIDE_MAX_ACTIONS, policy->num_actions, policy->obs_dim, policy->state_dim);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    int rc = MRL_OK;
    int g = guarded([&] {
        mrl_tensor_desc active{}, action{}, obs{}, mask{}, state{};
        // (the slot numbers are the same for both games: MRL_HANABI_* == MRL_BALANCE_* up to REWARD; the balance beam's state is its observation)
        if (!sim->tensor(MRL_HANABI_ACTIVE_AGENT, &active) || !sim->tensor(MRL_HANABI_ACTION, &action) ||
            !sim->tensor(MRL_HANABI_OBSERVATION, &obs) || !sim->tensor(MRL_HANABI_ACTION_MASK, &mask) ||
            !sim->tensor(sim->game == MRL_GAME_HANABI ? MRL_HANABI_STATE : MRL_BALANCE_OBSERVATION, &state))
            throw std::runtime_error(std::string(what) + ": the simulator does not export ACTIVE_AGENT / ACTION / OBSERVATION / ACTION_MASK / STATE");
        if (player >= (uint64_t)obs.shape[0] || policy->obs_dim > (uint64_t)obs.shape[2] || policy->state_dim > (uint64_t)state.shape[2] ||
            policy->num_actions > (uint64_t)mask.shape[2]) {
            mrl::set_error("%s: player %u of %lld; obs_dim %u, state_dim %u, num_actions %u against rows of %lld, %lld, %lld", what, player,
                           (long long)obs.shape[0], policy->obs_dim, policy->state_dim, policy->num_actions, (long long)obs.shape[2],
                           (long long)state.shape[2], (long long)mask.shape[2]);
            rc = MRL_ERR_INVALID;
            return;
        }
        if (obs.strides[2] != 1 || state.strides[2] != 1 || mask.strides[2] != 1 || action.dtype != MRL_INT32 || active.ndim != 2)
            throw std::runtime_error(std::string(what) + ": unexpected tensor layout (rows must be dense, ACTION int32, ACTIVE_AGENT (P, N))");
        mrl::AgentActArgs &args = *out;
        args = mrl::AgentActArgs{};
        args.params = policy->params_dev;
        args.obs = agent_slice(obs, player), args.state = agent_slice(state, player), args.mask = agent_slice(mask, player);
        args.active = agent_slice(active, player);
        args.action = static_cast<int32_t *>(action.data) + (int64_t)player * action.strides[0];
        args.action_stride = action.strides[1];
        args.D = policy->obs_dim, args.S = policy->state_dim, args.A = policy->num_actions;
        args.num_worlds = sim->num_worlds, args.player = player;
        if (seats) *seats = (uint32_t)obs.shape[0];
    });
    return g != MRL_OK ? g : rc;
}

int mrl_agent_act(mrl_sim *sim, uint32_t player, const mrl_wide_policy *policy, const mrl_agent_record *record, uint32_t row,
                  uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev, void *hip_stream)
{
    mrl::AgentActArgs args{};
    if (int rc = agent_prepare(sim, player, policy, workspace_dev, hip_stream, "mrl_agent_act", &args)) return rc;
    if ((flags & MRL_AGENT_VALUE_ONLY) && !record) {
        mrl::set_error("mrl_agent_act: MRL_AGENT_VALUE_ONLY writes next_value and next_active of a record; none was given");
        return MRL_ERR_INVALID;
    }
    if (record && (!agent_record_complete(record) || record->num_worlds != sim->num_worlds ||
                   (!(flags & MRL_AGENT_VALUE_ONLY) && row >= record->num_steps))) {
        mrl::set_error("mrl_agent_act: the record needs every buffer but logits, num_worlds = %u (got %u) and row < num_steps (row %u of %u)",
                       sim->num_worlds, record->num_worlds, row, record->num_steps);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        args.record = record, args.row = row, args.step = step, args.flags = flags, args.seed = seed;
        args.ws = mrl::wide_workspace(workspace_dev, sim->num_worlds);
        mrl::launch_agent_act(args, (hipStream_t)hip_stream);
    });
}

int mrl_agent_credit(const mrl_agent_record *record, const float *rewards_dev, const int32_t *dones_dev, uint32_t num_worlds, int gpu_id,
                     void *hip_stream)
{
    if (!record || !rewards_dev || !dones_dev || !agent_record_complete(record) || record->num_worlds != num_worlds) {
        mrl::set_error("mrl_agent_credit: null record, buffer, reward or done array, or num_worlds other than the record's");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] { mrl::launch_agent_credit(*record, rewards_dev, dones_dev, num_worlds, (hipStream_t)hip_stream); });
}

int mrl_gae_active(const mrl_agent_record *record, const float *next_value, const uint8_t *next_active, float gamma, float lambda,
                   float *advantages, float *returns, int gpu_id, void *hip_stream)
{
    if (!record || !next_value || !next_active || !advantages || !returns || !agent_record_complete(record)) {
        mrl::set_error("mrl_gae_active: null record, buffer or array");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_gae_active(*record, next_value, next_active, gamma, lambda, advantages, returns, (hipStream_t)hip_stream);
    });
}

static const char *agent_update_shape_error(uint32_t obs_dim, uint32_t state_dim, uint32_t num_actions, uint32_t capacity)
{
    if (num_actions == 0 || num_actions > MRL_WIDE_MAX_ACTIONS || obs_dim == 0 || state_dim == 0)
        return "need 1 <= num_actions <= 64 and obs_dim, state_dim >= 1";
    if (capacity == 0 || capacity >= (1u << 24)) return "need 1 <= capacity < 2^24 (the sample count travels through a float)";
    return nullptr;
}

int mrl_agent_update_workspace_bytes(uint32_t obs_dim, uint32_t state_dim, uint32_t num_actions, uint32_t capacity, uint64_t *out)
{
    const char *why = out ? agent_update_shape_error(obs_dim, state_dim, num_actions, capacity) : "need an output pointer";
    if (why) {
        mrl::set_error("mrl_agent_update_workspace_bytes: %s; got obs_dim %u, state_dim %u, num_actions %u, capacity %u", why, obs_dim,
                       state_dim, num_actions, capacity);
        return MRL_ERR_INVALID;
    }
    *out = mrl::update_workspace_bytes(capacity, mrl_wide_policy_num_params(obs_dim, state_dim, num_actions));
    return MRL_OK;
}

int mrl_agent_update(const mrl_wide_policy *policy, const mrl_ppo_optimizer *opt, const mrl_agent_record *record, uint32_t obs_type,
                     uint32_t state_type, const float *advantages, const float *returns, uint32_t epochs, const mrl_ppo_config *cfg,
                     uint32_t capacity, void *workspace_dev, uint64_t workspace_bytes, float *stats_or_null, float *grads_or_null,
                     int gpu_id, void *hip_stream)
{
    if (!policy || !opt || !record || !cfg || !advantages || !returns || !workspace_dev) {
        mrl::set_error("mrl_agent_update: null policy, optimizer, record, configuration, advantages, returns or workspace");
        return MRL_ERR_INVALID;
    }
    if (!opt->params_dev || !opt->exp_avg || !opt->exp_avg_sq || !record->obs || !record->states || !record->action_masks ||
        !record->active || !record->actions || !record->logprobs || !record->values) {
        mrl::set_error("mrl_agent_update: null parameter or moment array, or a record without obs, states, action_masks, active, "
                       "actions, logprobs or values");
        return MRL_ERR_INVALID;
    }
    const uint64_t cells = (uint64_t)record->num_steps * record->num_worlds;
    if (cells >= (1u << 24)) {
        mrl::set_error("mrl_agent_update: a record of %llu cells; the sample count travels through a float, so T N must stay below 2^24",
                       (unsigned long long)cells);
        return MRL_ERR_INVALID;
    }
    const char *why = agent_update_shape_error(policy->obs_dim, policy->state_dim, policy->num_actions, capacity);
    if (why || capacity > cells) {
        mrl::set_error("mrl_agent_update: %s; got obs_dim %u, state_dim %u, num_actions %u, capacity %u for a record of %llu cells",
                       why ? why : "capacity must not exceed T N", policy->obs_dim, policy->state_dim, policy->num_actions, capacity,
                       (unsigned long long)cells);
        return MRL_ERR_INVALID;
    }
    if (cfg->flags & ~(uint32_t)(MRL_PPO_NORM_ADV | MRL_PPO_CLIP_VLOSS)) {
        mrl::set_error("mrl_agent_update: unknown flag bits 0x%x", cfg->flags & ~(uint32_t)(MRL_PPO_NORM_ADV | MRL_PPO_CLIP_VLOSS));
        return MRL_ERR_INVALID;
    }
    if (obs_type > MRL_UINT32 || state_type > MRL_UINT32) {
        mrl::set_error("mrl_agent_update: element types must be MRL_INT8, MRL_UINT8, MRL_INT32, MRL_FLOAT32 or MRL_UINT32; got %u and %u",
                       obs_type, state_type);
        return MRL_ERR_INVALID;
    }
    uintptr_t floats = 0;
    for (const void *p : {(const void *)opt->params_dev, (const void *)opt->exp_avg, (const void *)opt->exp_avg_sq,
                          (const void *)record->logprobs, (const void *)record->values, (const void *)record->actions,
                          (const void *)advantages, (const void *)returns, (const void *)stats_or_null, (const void *)grads_or_null})
        floats |= reinterpret_cast<uintptr_t>(p);
    if (obs_type != MRL_INT8 && obs_type != MRL_UINT8) floats |= reinterpret_cast<uintptr_t>(record->obs);
    if (state_type != MRL_INT8 && state_type != MRL_UINT8) floats |= reinterpret_cast<uintptr_t>(record->states);
    const uint64_t need_bytes = mrl::update_workspace_bytes(capacity, mrl_wide_policy_num_params(policy->obs_dim, policy->state_dim, policy->num_actions));
    if (int rc = update_refusal("mrl_agent_update", "mrl_agent_update_workspace_bytes", workspace_bytes, need_bytes, workspace_dev,
                                floats & 3u, "float and int32 arrays must start on a 4-byte boundary", hip_stream))
        return rc;
    if (opt->num_members) {
        mrl::set_error("mrl_agent_update: opt->num_members is %u; the wide policy has no bank update (mrl_ppo_update takes members), "
                       "pass 0", opt->num_members);
        return MRL_ERR_INVALID;
    }
    if (epochs == 0) return MRL_OK;
    mrl::AgentUpdateArgs args{};
    args.policy = *policy, args.opt = *opt, args.record = *record, args.cfg = *cfg;
    args.obs_type = obs_type, args.state_type = state_type;
    args.advantages = advantages, args.returns = returns;
    args.epochs = epochs, args.capacity = capacity;
    args.workspace = workspace_dev, args.stats = stats_or_null, args.grads = grads_or_null;
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] { mrl::launch_agent_update(args, (hipStream_t)hip_stream); });
}

// (the slot numbers are the same for both games)
static const mrl::BankFamily kWideFamily{1u << MRL_GAME_HANABI | 1u << MRL_GAME_BALANCE, "no wide-policy agent (Hanabi and the balance beam do)",
                                         MRL_HANABI_OBSERVATION, 0, MRL_HANABI_DONE, "OBSERVATION / DONE"};

int mrl_agent_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                            void *hip_stream)
{
    return mrl::bank_resample(sim, kWideFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_agent_bank_resample");
}

int mrl_agent_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_policies, uint64_t *out)
{
    if (!out || num_policies == 0 || num_policies > mrl::kBankMaxPolicies) {
        mrl::set_error("mrl_agent_bank_workspace_bytes: null output pointer, or a bank of %u policies (a bank holds 1 to %u)", num_policies,
                       mrl::kBankMaxPolicies);
        return MRL_ERR_INVALID;
    }
    *out = mrl::wide_bank_workspace_bytes(num_worlds, num_policies);
    return MRL_OK;
}

int mrl_agent_act_bank(mrl_sim *sim, uint32_t player, const mrl_wide_bank *bank, const int32_t *ids_dev, int32_t *ids_row, uint64_t seed,
                       uint32_t step, uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    const char *what = "mrl_agent_act_bank";
    if (!bank) {
        mrl::set_error("%s: null bank", what);
        return MRL_ERR_INVALID;
    }
    const mrl_wide_policy row0{bank->params_dev, bank->obs_dim, bank->state_dim, bank->num_actions};
    mrl::WideBankArgs args{};
    if (int rc = agent_prepare(sim, player, &row0, workspace_dev, hip_stream, what, &args.act, &args.P)) return rc;
    if (flags & ~(uint32_t)(MRL_POLICY_GREEDY | MRL_AGENT_ALL_ROWS)) {
        mrl::set_error("%s: flags 0x%x; the bank act takes MRL_POLICY_GREEDY and MRL_AGENT_ALL_ROWS (there is no record, so no "
                       "MRL_AGENT_VALUE_ONLY: train a member through mrl_agent_act on its row)", what, flags);
        return MRL_ERR_INVALID;
    }
    const uint32_t K = bank->num_policies, N = sim->num_worlds;
    // (one seat acts in a call: N cells)
    if (int rc = mrl::bank_refusal(what, N, 1, K, bank->stride, mrl_wide_policy_num_params(bank->obs_dim, bank->state_dim, bank->num_actions),
                                   ids_dev, workspace_dev, workspace_bytes, mrl::wide_bank_workspace_bytes(N, K),
                                   "mrl_agent_bank_workspace_bytes"))
        return rc;
    if (reinterpret_cast<uintptr_t>(ids_row) & 3u) {
        mrl::set_error("%s: ids_row is off a 4-byte boundary", what);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        char *base = static_cast<char *>(workspace_dev);
        args.act.record = nullptr, args.act.row = 0, args.act.step = step, args.act.flags = flags, args.act.seed = seed;
        args.act.ws = mrl::wide_workspace(base, N);
        args.eff = reinterpret_cast<int32_t *>(base + mrl::wide_workspace_bytes(N));
        args.plan = reinterpret_cast<uint32_t *>(base + mrl::wide_workspace_bytes(N) + mrl::wide_bank_eff_bytes(N));
        args.ids = ids_dev, args.ids_row = ids_row;
        args.stride = bank->stride, args.num_policies = K;
        mrl::launch_agent_act_bank(args, (hipStream_t)hip_stream);
    });
}

}  // extern "C"
