// What the three policy banks (CNN, MLPBase, wide) share in the C API: the refusals of a bank act and the resample behind the
// three mrl_*_bank_resample calls and the bank rollouts (declared in capi_internal.hpp).
#include "capi_internal.hpp"
#include "bank_plan.hpp"

namespace mrl {

// What every bank act refuses behind its own network's checks: the bank's size and stride (`num_params`: the floats of one
// policy), the ids, the cells of a call (`seats` per world; the plan numbers them) and the workspace of `need_bytes`, which is
// what `sizer` returns.
int bank_refusal(const char *what, uint32_t num_worlds, uint32_t seats, uint32_t num_policies, uint64_t stride, uint64_t num_params,
                 const int32_t *ids_dev, void *workspace_dev, uint64_t workspace_bytes, uint64_t need_bytes, const char *sizer)
{
    if (num_policies == 0 || num_policies > mrl::kBankMaxPolicies) {
        mrl::set_error("%s: a bank holds 1 to %u policies, not %u", what, mrl::kBankMaxPolicies, num_policies);
        return MRL_ERR_INVALID;
    }
    if (stride < num_params) {
        mrl::set_error("%s: the bank's stride of %llu floats is below the policy's %llu parameters", what, (unsigned long long)stride,
                       (unsigned long long)num_params);
        return MRL_ERR_INVALID;
    }
    if (!ids_dev || (reinterpret_cast<uintptr_t>(ids_dev) & 3u)) {
        mrl::set_error("%s: ids is null or off a 4-byte boundary", what);
        return MRL_ERR_INVALID;
    }
    if ((uint64_t)num_worlds * seats > 0x7fffffffull) {
        mrl::set_error("%s: %u worlds of %u seats are more cells than the plan numbers", what, num_worlds, seats);
        return MRL_ERR_INVALID;
    }
    if (!workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u) || workspace_bytes < need_bytes) {
        mrl::set_error("%s: the workspace is null, off a 16-byte boundary or smaller than %s = %llu bytes", what, sizer,
                       (unsigned long long)need_bytes);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// the descriptor of a resample, whichever network's bank it serves
static int resample_desc_refusal(const mrl_cnn_resample *resample, const char *what)
{
    if (!resample || !resample->first_id || !resample->num_ids ||
        (resample->mode != MRL_CNN_RESAMPLE_ROBIN && resample->mode != MRL_CNN_RESAMPLE_RANDOM)) {
        mrl::set_error("%s: null resample, first_id or num_ids, or a mode other than MRL_CNN_RESAMPLE_ROBIN and MRL_CNN_RESAMPLE_RANDOM", what);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// the seat mask and the seats' ranges of a resample on a simulator of P seats whose DONE is `done`; fills `args` but for ids and
// episodes
static int resample_fill(mrl_sim *sim, uint32_t players, uint32_t P, const mrl_tensor_desc &done, const mrl_cnn_resample *resample,
                         const char *what, mrl::CnnResampleArgs *args)
{
    if (players == 0 || P > 32 || (P < 32 && (players >> P) != 0)) {
        mrl::set_error("%s: players = 0x%x must name at least one seat and none beyond the simulator's %u", what, players, P);
        return MRL_ERR_INVALID;
    }
    mrl::CnnResampleArgs &a = *args;
    a = mrl::CnnResampleArgs{};
    for (uint32_t p = 0; p < P; p++) {
        if (!((players >> p) & 1u)) continue;
        const uint32_t first = resample->first_id[p], num = resample->num_ids[p];
        if (num == 0 || first > mrl::kBankMaxPolicies || num > mrl::kBankMaxPolicies || first + num > mrl::kBankMaxPolicies) {
            mrl::set_error("%s: seat %u draws from [%u, %u + %u): a range is 1 to 256 ids and ends at 256 at the latest", what, p, first, first, num);
            return MRL_ERR_INVALID;
        }
        a.first[p] = (uint16_t)first, a.num[p] = (uint16_t)num;
    }
    a.done = static_cast<const int32_t *>(done.data);
    a.seed = resample->seed;
    a.num_worlds = sim->num_worlds, a.P = P, a.players = players, a.mode = resample->mode;
    return MRL_OK;
}

// What mrl_*_bank_resample and the bank rollouts check of a resample on a simulator of `family`; fills `args`.
int bank_resample_prepare(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
                          int32_t *episodes_dev, const char *what, mrl::CnnResampleArgs *args)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if ((uint32_t)sim->game > 31u || !((family.games >> sim->game) & 1u)) {
        mrl::set_error("%s: game %d has %s", what, sim->game, family.has);
        return MRL_ERR_INVALID;
    }
    if (int rc = resample_desc_refusal(resample, what)) return rc;
    mrl_tensor_desc obs{}, done{};
    int rc = mrl::guarded([&] {
        if (!sim->tensor(family.obs_slot, &obs) || !sim->tensor(family.done_slot, &done))
            throw std::runtime_error(std::string("the simulator does not export ") + family.tensors);
    });
    if (rc) return rc;
    if (int rc2 = resample_fill(sim, players, (uint32_t)obs.shape[family.seat_axis], done, resample, what, args)) return rc2;
    if (!ids_dev || !episodes_dev || ((reinterpret_cast<uintptr_t>(ids_dev) | reinterpret_cast<uintptr_t>(episodes_dev)) & 3u)) {
        mrl::set_error("%s: a resample's ids or episodes is null or off a 4-byte boundary", what);
        return MRL_ERR_INVALID;
    }
    args->ids = ids_dev, args->episodes = episodes_dev;
    return MRL_OK;
}

// the three public resamples behind their family
int bank_resample(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
                  int32_t *episodes_dev, void *hip_stream, const char *what)
{
    mrl::CnnResampleArgs args{};
    if (int rc = bank_resample_prepare(sim, family, players, resample, ids_dev, episodes_dev, what, &args)) return rc;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] { mrl::launch_cnn_bank_resample(args, (hipStream_t)hip_stream); });
}

}  // namespace mrl
