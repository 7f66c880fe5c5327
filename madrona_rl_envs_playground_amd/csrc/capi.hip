// extern "C" entry points of libmrl_envs.so (include/mrl_envs.h).
#include "common.hpp"
#include "episode_scan.hpp"
#include "episode_stats.hpp"
#include "policy_rollout.hpp"
#include "ppo_update.hpp"
#include "wide_policy.hpp"
#include "wide_bank.hpp"
#include "wide_update.hpp"
#include "cnn_policy.hpp"
#include "cnn_bank.hpp"
#include "cnn_update.hpp"
#include "mlpbase_policy.hpp"
#include "mlpbase_bank.hpp"
#include "mlpbase_update.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <exception>
#include <map>
#include <mutex>
#include <string>

namespace mrl {

static thread_local char g_error[512] = "";

// mrl_debug_set: the knobs tests and measurement tools may turn (the library reads no environment variable)
static const char *const kDebugKeys[] = {
    "overcooked.wpw",        // worlds per wave (0 = chosen by the library)
    "overcooked.whole_max",  // largest single-pass observation tile, bytes
    "overcooked.lds_max",    // LDS budget per workgroup, bytes
    "overcooked.share_max_players",  // experiment: up to how many players the four waves of a workgroup share one world of a large layout
    "overcooked.share_private",  // 1: waves that share a world keep a private copy of its state each (step_body) instead of one per workgroup (team_body)
    "overcooked.no_share",   // 1: never let the waves of a workgroup share one world
    "overcooked.lds_pad",    // experiment: extra LDS bytes per workgroup (limits how many are resident per CU)
    "overcooked.no_fixed",   // 1: never use the kernels specialised for one layout size
    "overcooked.no_direct",  // 1: the single-pass encode looks for its dynamic cells (cell -> player map + ballot compaction) instead of
                             // taking them from the player lanes and the holder-cell table
    "overcooked.whole_store",   // single-pass stream-out stores: 0 by slab size and group alignment (default), 1 write-through, 2 plain
    "overcooked.store_policy",  // multi-pass stream-out stores: 0 by slab size (default), 1 sc1 write-through, 2 plain, 3 nt
    "overcooked.wide_rollout",  // 1: the multi-step launches keep the single step's group size (default: twice as wide where it fits)
    "overcooked.writeback",  // cell words the single step writes back: 0 by batch size and layout (default), 1 every word, 2 only the words that changed
    "overcooked.groups",     // groups of worlds a wave steps one after the other in the single step of the standard layouts: 0 by batch size, 1, 2
    "overcooked.shared_consts",  // 1: constants through the workgroup-shared LDS block + barrier even where a private copy would do
    "overcooked.variant",    // 0: the library's choice; 1: force the generic (lane = world) transition
    "hanabi.variant",        // cap on the encoder variant (0 = the generic encoders)
    "hanabi.pairing",        // phase A of the single-launch step: 4 (default) four leader waves step their own and wave w + 4's worlds with all
                             // 64 lanes, 1 the pairs are (2k, 2k + 1), 0 every wave steps its own 32 worlds
    "hanabi.no_persistent",  // 1: mrl_rollout_random as one launch per step
    "cartpole.no_persistent",
    "cartpole.persistent_max",  // largest batch mrl_rollout_random runs as ONE persistent launch (above: one single-launch step per step)
    "cartpole.variant",      // arithmetic of the transition: 0 the library's default, 1 typed and rounded as the reference writes it (four double
                             // divisions), 2 the same float roundings around fused double intermediates and reciprocals, 3 = 2 with sin/cos
                             // evaluated without range reduction while |theta| <= pi/4 (the default), 4 float throughout (csrc/cartpole.hip)
    "fused_step",            // mrl_step of Hanabi / Cartpole as ONE launch with the in-kernel look-back (episode_scan.hpp) or as
                             // phase 1 + phase 2 launches: 0 the library's choice, 1 one launch where the kernel exists, 2 always two
    "fused_heal_test",       // m > 0: in the single-launch step, workgroups whose index is a multiple of m act as if dispatched late, so
                             // that higher workgroups take the recount path of the healing look-back (tests)
    "inject_scan_timeout",   // 1: the simulator's SCAN_TIMEOUT alarm is raised right after construction (tests of the error path)
    "ablate",                // diagnostic build only: phase ablation mask
    "stamps",                // diagnostic build only: in-kernel time stamps
};
static std::mutex g_debug_mutex;
static std::map<std::string, int64_t> g_debug;

int64_t debug_get(const char *key, int64_t fallback)
{
    std::lock_guard<std::mutex> lock(g_debug_mutex);
    auto it = g_debug.find(key);
    return it == g_debug.end() ? fallback : it->second;
}

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

void bind_device(int gpu_id)
{
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count == 0) {
        set_error("no HIP device available (%s); this engine has no CPU execution mode",
                  err == hipSuccess ? "device count is 0" : hipGetErrorString(err));
        throw HipError{MRL_ERR_DEVICE};
    }
    if (gpu_id < 0 || gpu_id >= count) {
        set_error("gpu_id %d out of range (%d device(s))", gpu_id, count);
        throw HipError{MRL_ERR_INVALID};
    }
    MRL_HIP(hipSetDevice(gpu_id));
    hipDeviceProp_t prop;
    MRL_HIP(hipGetDeviceProperties(&prop, gpu_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libmrl_envs.so carries gfx950 (MI355X) code objects only", gpu_id,
                  prop.gcnArchName);
        throw HipError{MRL_ERR_DEVICE};
    }
}

template <typename Fn> static int guarded(Fn &&fn)
{
    try {
        g_error[0] = '\0';
        fn();
        return MRL_OK;
    } catch (const HipError &e) {
        return e.code;
    } catch (const std::exception &e) {
        set_error("%s", e.what());
        return MRL_ERR_INVALID;
    }
}

static int need(const mrl_sim *sim)
{
    if (!sim) {
        set_error("null simulator handle");
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

// Entry of every call that advances the simulation: a bounded in-kernel wait that expired in an
// earlier call (SCAN_TIMEOUT, episode_scan.hpp) left the episode numbering unspecified -- refuse to go on.
static int need_healthy(const mrl_sim *sim)
{
    if (int rc = need(sim)) return rc;
    if (sim->scan_timed_out()) {
        set_error("an in-kernel wait of an earlier step expired (SCAN_TIMEOUT): episode numbers of this simulator are "
                  "unspecified from that step on; destroy it and create a new one");
        return MRL_ERR_DEVICE;
    }
    return MRL_OK;
}

// Hanabi, Cartpole and the balance beam keep launch-to-launch state on the HOST by default (which half of the
// double-buffered episode counter is current, the epoch tag of the single-launch step): their launches bake it into kernel
// arguments, so a captured launch replayed later would run with stale values (repeated episode seeds, a look-back that
// accepts the previous replay's counts).  They refuse to be captured until mrl_prepare_graph_capture has moved that state
// into device memory, where every step advances it itself.  Overcooked and Simplecooked have no such state.
static int need_not_capturing(const mrl_sim *sim, void *hip_stream, const char *what)
{
    if (sim->capturable() || !hip_stream) return MRL_OK;
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)hip_stream, &status) != hipSuccess) {
        (void)hipGetLastError();
        return MRL_OK;
    }
    if (status == hipStreamCaptureStatusNone) return MRL_OK;
    set_error("%s: this game's launches carry host-side episode-counter state and cannot be captured in a HIP graph as they are; "
              "call mrl_prepare_graph_capture on the simulator first (outside the capture)", what);
    return MRL_ERR_INVALID;
}

static bool capturing(void *hip_stream)
{
    if (!hip_stream) return false;  // (asking about the NULL stream would itself break another stream's capture)
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)hip_stream, &status) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return status != hipStreamCaptureStatusNone;
}

// Behind every completed step (include/mrl_envs.h, mrl_enable_episode_stats): the general update launch, on the step's stream
static void completed_step(mrl_sim *sim, hipStream_t stream)
{
    if (!sim->stats) return;
    if (!sim->stats_taken) sim->stats->update(stream);
    sim->stats_taken = false;
}
// the counter games complete a two-phase step with phase 2; the kitchen games, whose phase 2 does nothing, with phase 1
static bool completes_in_phase1(const mrl_sim *sim) { return sim->game == MRL_GAME_OVERCOOKED || sim->game == MRL_GAME_SIMPLECOOKED; }

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

// mrl_rollout_cnn and mrl_rollout_cnn_bank: rollout_loop with the simulator writing slot k + 1 of the observation ring in step k;
// act(k, slot k, closing) reads its slot.
template <class Act, class AfterStep>
static int cnn_rollout_loop(mrl_sim *sim, const char *what, uint32_t T, void *obs_ring_dev, void *hip_stream, Act act, AfterStep after_step)
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

// ---- roofline.peak_measured of bench.py: float4 streams over caller buffers ----
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int kMode>
__global__ void __launch_bounds__(256) mrl_probe_stream_kernel(f32x4 *__restrict__ dst, const f32x4 *__restrict__ src, size_t chunks)
{
    // every workgroup streams through ONE contiguous range (like a wave of the step kernels writing its group's
    // slab): 4 x 4 KB in flight per workgroup and trip
    const size_t per_block = (chunks + gridDim.x - 1) / gridDim.x;
    const size_t first = (size_t)blockIdx.x * per_block, last = first + per_block < chunks ? first + per_block : chunks;
    const f32x4 fill = {1.f, 2.f, 3.f, 4.f};
    size_t i = first + threadIdx.x;
    for (; i + 3 * 256 < last; i += 4 * 256) {
        f32x4 a = fill, b = fill, c = fill, d = fill;
        if (kMode == 0) {
            a = src[i];
            b = src[i + 256];
            c = src[i + 512];
            d = src[i + 768];
        }
        if (kMode == 2) {  // write-through, like the observation stores of the step kernels
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i), "v"(a) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i + 256), "v"(b) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i + 512), "v"(c) : "memory");
            asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(dst + i + 768), "v"(d) : "memory");
        } else {
            dst[i] = a;
            dst[i + 256] = b;
            dst[i + 512] = c;
            dst[i + 768] = d;
        }
    }
    for (; i < last; i += 256) dst[i] = kMode == 0 ? src[i] : fill;
}

// Modes 3 / 4: the bytes and stores of mode 2 in TWO passes inside one launch.  The first pass stores the aligned
// kBlockBytes blocks (64 / 128) of a fixed pseudo-random quarter of the block indices, the second pass the rest -- what a
// step kernel does when it sends the blocks that cannot change ahead of the others.  Asks whether two halves of a
// 128-byte line that reach the L2 at different times cost more than the line written at once.
template <int kBlockBytes>
__global__ void __launch_bounds__(256) mrl_probe_stream_two_pass_kernel(f32x4 *__restrict__ dst, size_t chunks)
{
    const size_t per_block = (chunks + gridDim.x - 1) / gridDim.x;
    const size_t first = (size_t)blockIdx.x * per_block, last = first + per_block < chunks ? first + per_block : chunks;
    const f32x4 fill = {1.f, 2.f, 3.f, 4.f};
    constexpr int kShift = kBlockBytes == 64 ? 2 : 3;  // 16-byte chunks per block
    for (int pass = 0; pass < 2; pass++) {
        for (size_t i = first + threadIdx.x; i < last; i += 256) {
            const bool early = (((uint32_t)(i >> kShift) * 2654435761u) >> 30) == 0u;
            if (early == (pass == 0)) asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(dst + i), "v"(fill) : "memory");
        }
    }
}

// What every bank act refuses behind its own network's checks: the bank's size and stride (`num_params`: the floats of one
// policy), the ids, the cells of a call (`seats` per world; the plan numbers them) and the workspace of `need_bytes`, which is
// what `sizer` returns.
static int bank_refusal(const char *what, uint32_t num_worlds, uint32_t seats, uint32_t num_policies, uint64_t stride, uint64_t num_params,
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

// Everything the act and the rollout of a MAPPO bank (CnnBankArgs, MlpBaseBankArgs) check alike: prepare(), the network's own
// checks with row 0 of the bank as the policy, which fills args->act; then bank_refusal with num_params(), the floats of one
// policy, and `sizer`, the name of the entry point's own workspace function.  Fills args->bank but for the ids row.
template <class Bank, class Args, class Prepare, class NumParams>
static int bank_prepare(const char *what, const char *sizer, const Bank *bank, const int32_t *ids_dev, void *workspace_dev, uint64_t workspace_bytes, Args *args,
                        Prepare prepare, NumParams num_params)
{
    if (!bank) {
        set_error("%s: null bank", what);
        return MRL_ERR_INVALID;
    }
    if (int rc = prepare()) return rc;
    const ActArgs &a = args->act;
    if (int rc = bank_refusal(what, a.num_worlds, a.P, bank->num_policies, bank->stride, num_params(), ids_dev, workspace_dev, workspace_bytes,
                              mrl_cnn_bank_workspace_bytes(a.num_worlds, a.P, bank->num_policies), sizer))
        return rc;
    args->bank = BankActArgs{ids_dev, nullptr, static_cast<uint32_t *>(workspace_dev), bank->stride, bank->num_policies};
    return MRL_OK;
}

}  // namespace mrl

using mrl::guarded;

extern "C" {

int mrl_abi_version(void) { return MRL_ABI_VERSION; }

#ifndef MRL_SOURCE_HASH
#error "build through csrc/Makefile: it passes -DMRL_SOURCE_HASH (the hash of the sources, see the Makefile)"
#endif
// "MRL_SOURCE_HASH=" in front so that the value can also be found in the file without loading it (_lib.embedded_hash)
static const char g_build_hash[] = "MRL_SOURCE_HASH=" MRL_SOURCE_HASH;
const char *mrl_build_hash(void) { return g_build_hash + sizeof("MRL_SOURCE_HASH=") - 1; }
const char *mrl_last_error(void) { return mrl::g_error; }

int mrl_overcooked_create(const mrl_overcooked_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_overcooked(cfg, gpu_id, num_worlds); });
}

int mrl_simplecooked_create(const mrl_overcooked_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_simplecooked(cfg, gpu_id, num_worlds); });
}

int mrl_hanabi_create(const mrl_hanabi_config *cfg, int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_hanabi(cfg, gpu_id, num_worlds); });
}

int mrl_cartpole_create(int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_cartpole(gpu_id, num_worlds); });
}

int mrl_balance_create(int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_balance(gpu_id, num_worlds); });
}

int mrl_acrobot_create(int gpu_id, uint32_t num_worlds, mrl_sim **out)
{
    if (!out) return MRL_ERR_INVALID;
    *out = nullptr;
    mrl::DeviceGuard on(gpu_id);  // the caller's current device is restored on return
    return guarded([&] { *out = mrl::create_acrobot(gpu_id, num_worlds); });
}

int mrl_step(mrl_sim *sim, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step")) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->step(nullptr, (hipStream_t)hip_stream);
        mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_step_with_actions(mrl_sim *sim, const int32_t *actions_dev, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_with_actions")) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->step(actions_dev, (hipStream_t)hip_stream);
        mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_step_many(mrl_sim *const *sims, uint32_t count, const int32_t *const *actions_dev_or_null, void *hip_stream)
{
    if (!sims && count) {
        mrl::set_error("mrl_step_many: null simulator list");
        return MRL_ERR_INVALID;
    }
    for (uint32_t k = 0; k < count; k++)
        if (int rc = mrl::need_healthy(sims[k])) return rc;
    if (count == 0) return MRL_OK;
    mrl::DeviceGuard on(sims[0]->device);
    return guarded([&] {
        mrl::step_many_overcooked(sims, count, actions_dev_or_null, (hipStream_t)hip_stream);
        for (uint32_t k = 0; k < count; k++) mrl::completed_step(sims[k], (hipStream_t)hip_stream);
    });
}

int mrl_step_with_actions_i64(mrl_sim *sim, const int64_t *actions_dev, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (!actions_dev) {
        mrl::set_error("mrl_step_with_actions_i64: null action array");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    int rc = MRL_OK;
    const int g = guarded([&] {
        if (!sim->step_i64(reinterpret_cast<const long long *>(actions_dev), (hipStream_t)hip_stream)) {
            mrl::set_error("mrl_step_with_actions_i64: not available for game %d; convert to int32 and use mrl_step_with_actions", sim->game);
            rc = MRL_ERR_INVALID;
        } else {
            mrl::completed_step(sim, (hipStream_t)hip_stream);
        }
    });
    return g != MRL_OK ? g : rc;
}

int mrl_step_phase1(mrl_sim *sim, const int32_t *actions_dev_or_null, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_phase1")) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->phase1(actions_dev_or_null, (hipStream_t)hip_stream);
        sim->publish_shard_count((hipStream_t)hip_stream);
        if (mrl::completes_in_phase1(sim)) mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_step_phase2(mrl_sim *sim, const uint32_t *episode_base_dev, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_phase2")) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->phase2(episode_base_dev, (hipStream_t)hip_stream);
        if (!mrl::completes_in_phase1(sim)) mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_step_phase2_gathered(mrl_sim *sim, const uint32_t *counts_dev, uint32_t num_ranks, uint32_t rank, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_phase2_gathered")) return rc;
    if (!counts_dev || num_ranks == 0 || num_ranks > 1024 || rank >= num_ranks) {
        mrl::set_error("mrl_step_phase2_gathered: need the gathered counts, 1..1024 ranks and rank < num_ranks (got %u of %u)", rank, num_ranks);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->phase2_gathered(counts_dev, num_ranks, rank, (hipStream_t)hip_stream);
        if (!mrl::completes_in_phase1(sim)) mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_exchange_create(mrl_sim *sim, uint32_t num_ranks, uint32_t rank, uint8_t *ipc_handle_out)
{
    if (int rc = mrl::need(sim)) return rc;
    static_assert(sizeof(hipIpcMemHandle_t) == MRL_IPC_HANDLE_BYTES, "MRL_IPC_HANDLE_BYTES is hipIpcMemHandle_t's size");
    if (!ipc_handle_out || num_ranks == 0 || num_ranks > MRL_MAX_RANKS || rank >= num_ranks) {
        mrl::set_error("mrl_exchange_create: need a handle buffer, 1..%d ranks and rank < num_ranks (got %u of %u)", MRL_MAX_RANKS, rank, num_ranks);
        return MRL_ERR_INVALID;
    }
    if (sim->exchange.mine) {
        mrl::set_error("mrl_exchange_create: this simulator already has a mailbox");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        mrl::ShardExchange &x = sim->exchange;
        const size_t bytes = sizeof(unsigned long long) * mrl::kMailSlots * MRL_MAX_RANKS;
        void *block = nullptr;
        // fine-grained: the peers' stores must become visible to a kernel of this device that is already running
        if (hipExtMallocWithFlags(&block, bytes, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            MRL_HIP(hipMalloc(&block, bytes));
        }
        x.mine = static_cast<unsigned long long *>(block);
        MRL_HIP(hipMemset(x.mine, 0, bytes));
        MRL_HIP(hipDeviceSynchronize());
        hipIpcMemHandle_t handle;
        MRL_HIP(hipIpcGetMemHandle(&handle, x.mine));
        memcpy(ipc_handle_out, &handle, sizeof(handle));
        x.num_ranks = num_ranks;
        x.rank = rank;
        x.step = 0;
    });
}

int mrl_exchange_connect(mrl_sim *sim, const uint8_t *ipc_handles_of_all_ranks)
{
    if (int rc = mrl::need(sim)) return rc;
    mrl::ShardExchange &x = sim->exchange;
    if (!ipc_handles_of_all_ranks || !x.mine || x.connected) {
        mrl::set_error("mrl_exchange_connect: call mrl_exchange_create first, once, and pass the handles of all ranks");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        for (uint32_t p = 0; p < x.num_ranks; p++) {
            if (p == x.rank) {
                x.peer[p] = x.mine;  // (a process cannot open its own handle)
                continue;
            }
            hipIpcMemHandle_t handle;
            memcpy(&handle, ipc_handles_of_all_ranks + (size_t)p * sizeof(handle), sizeof(handle));
            void *mapped = nullptr;
            MRL_HIP(hipIpcOpenMemHandle(&mapped, handle, hipIpcMemLazyEnablePeerAccess));
            x.peer[p] = static_cast<unsigned long long *>(mapped);
        }
        x.connected = true;
    });
}

int mrl_step_exchanged(mrl_sim *sim, const int32_t *actions_dev_or_null, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_exchanged")) return rc;
    if (!sim->exchange.connected) {
        mrl::set_error("mrl_step_exchanged: no connected mailbox (mrl_exchange_create, mrl_exchange_connect)");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        mrl::ShardExchange &x = sim->exchange;
        x.step += 1;  // this step's tag: the words of step k live in slot k % kMailSlots
        x.publishing = true;
        struct Done {
            mrl::ShardExchange &x;
            ~Done() { x.publishing = false; }
        } done{x};
        sim->step_exchanged(actions_dev_or_null, (hipStream_t)hip_stream);
        mrl::completed_step(sim, (hipStream_t)hip_stream);
    });
}

int mrl_set_observation_output(mrl_sim *sim, void *obs_dev_or_null, uint64_t bytes)
{
    if (int rc = mrl::need(sim)) return rc;
    const uint64_t want = sim->observation_bytes();
    if (want == 0) {
        mrl::set_error("mrl_set_observation_output: game %d writes no redirectable observation slab (Overcooked and Simplecooked do)", sim->game);
        return MRL_ERR_INVALID;
    }
    if (obs_dev_or_null && bytes != want) {
        mrl::set_error("mrl_set_observation_output: need a device buffer of exactly %llu bytes (N x P x H x W x F int8), got %llu at %p",
                       (unsigned long long)want, (unsigned long long)bytes, obs_dev_or_null);
        return MRL_ERR_INVALID;
    }
    return guarded([&] { sim->set_observation_output(obs_dev_or_null); });
}

int mrl_set_observation_ring(mrl_sim *sim, void *base_dev_or_null, uint64_t slot_stride_bytes, uint32_t num_slots)
{
    if (int rc = mrl::need(sim)) return rc;
    const uint64_t want = sim->observation_bytes();
    if (want == 0) {
        mrl::set_error("mrl_set_observation_ring: game %d writes no redirectable observation slab (Overcooked and Simplecooked do)", sim->game);
        return MRL_ERR_INVALID;
    }
    if (base_dev_or_null && (num_slots == 0 || slot_stride_bytes < want)) {
        mrl::set_error("mrl_set_observation_ring: need at least one slot and a slot stride >= %llu bytes (N x P x H x W x F int8); got stride "
                       "%llu, %u slot(s) at %p",
                       (unsigned long long)want, (unsigned long long)slot_stride_bytes, num_slots, base_dev_or_null);
        return MRL_ERR_INVALID;
    }
    return guarded([&] { sim->set_observation_ring(base_dev_or_null, slot_stride_bytes, num_slots); });
}

int mrl_prepare_graph_capture(mrl_sim *sim, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] { sim->prepare_graph_capture((hipStream_t)hip_stream); });
}

int mrl_enable_episode_stats(mrl_sim *sim, void *hip_stream)
{
    if (int rc = mrl::need(sim)) return rc;
    if (sim->stats) return MRL_OK;
    if (mrl::capturing(hip_stream)) {
        mrl::set_error("mrl_enable_episode_stats: the call allocates and cannot run on a capturing stream; enable the statistics "
                       "before the capture");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        auto *stats = new mrl::EpisodeStats();
        try {
            stats->init(sim, (hipStream_t)hip_stream);
        } catch (...) {
            delete stats;
            throw;
        }
        sim->stats = stats;
    });
}

int mrl_clear_episode_totals(mrl_sim *sim, void *hip_stream)
{
    if (int rc = mrl::need(sim)) return rc;
    if (!sim->stats) {
        mrl::set_error("mrl_clear_episode_totals: call mrl_enable_episode_stats first");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] { sim->stats->clear_totals((hipStream_t)hip_stream); });
}

int mrl_set_episode_counter(mrl_sim *sim, uint32_t next_episode, void *hip_stream)
{
    if (int rc = mrl::need(sim)) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] { sim->set_episode_counter(next_episode, (hipStream_t)hip_stream); });
}

int mrl_reseed_shard(mrl_sim *sim, uint32_t world_offset, uint32_t num_worlds_total, void *hip_stream)
{
    if (int rc = mrl::need(sim)) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->reseed_shard(world_offset, num_worlds_total, (hipStream_t)hip_stream);
        sim->reseeded = true;
        if (sim->stats) sim->stats->clear_running(nullptr, (hipStream_t)hip_stream);
    });
}

int mrl_reset_worlds(mrl_sim *sim, const uint8_t *mask_dev_or_null, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_reset_worlds")) return rc;
    const bool numbered = sim->game == MRL_GAME_HANABI || sim->game == MRL_GAME_CARTPOLE || sim->game == MRL_GAME_BALANCE ||
                          sim->game == MRL_GAME_ACROBOT;
    if (numbered && (sim->reseeded || sim->exchange.mine)) {
        mrl::set_error("mrl_reset_worlds: this simulator is a shard of a larger batch (mrl_reseed_shard / mrl_exchange_create); "
                       "numbering restarted episodes across ranks is not supported");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        sim->reset_worlds(mask_dev_or_null, (hipStream_t)hip_stream);
        // a forced restart is not a finished episode: the running values go, LAST_* and TOTALS stay
        if (sim->stats) sim->stats->clear_running(mask_dev_or_null, (hipStream_t)hip_stream);
    });
}

int mrl_step_sequence(mrl_sim *sim, const int32_t *actions_dev, uint32_t num_steps, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_step_sequence")) return rc;
    mrl::DeviceGuard on(sim->device);
    if (!actions_dev && num_steps) {
        mrl::set_error("mrl_step_sequence: null action array");
        return MRL_ERR_INVALID;
    }
    return guarded([&] {
        if (!sim->stats) {
            sim->step_sequence(actions_dev, num_steps, (hipStream_t)hip_stream);
            return;
        }
        // K steps equal K single calls: with statistics each is a launch of its own with the update behind it
        for (uint32_t k = 0; k < num_steps; k++) {
            sim->step(actions_dev + (size_t)k * sim->action_elems(), (hipStream_t)hip_stream);
            mrl::completed_step(sim, (hipStream_t)hip_stream);
        }
    });
}

int mrl_rollout_random(mrl_sim *sim, uint32_t num_steps, uint64_t seed, uint32_t first_step, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_rollout_random")) return rc;
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        if (!sim->stats) {
            sim->rollout_random(num_steps, seed, first_step, (hipStream_t)hip_stream);
            return;
        }
        for (uint32_t k = 0; k < num_steps; k++) {
            sim->rollout_random(1, seed, first_step + k, (hipStream_t)hip_stream);
            mrl::completed_step(sim, (hipStream_t)hip_stream);
        }
    });
}

uint64_t mrl_mlp_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions)
{
    return mrl::mlp_net_params(obs_dim, hidden, 1) + mrl::mlp_net_params(obs_dim, hidden, num_actions);
}

int mrl_rollout_policy(mrl_sim *sim, const mrl_mlp_policy *policy, const mrl_rollout_buffers *buffers, uint64_t seed,
                       uint32_t first_step, void *hip_stream)
{
    if (int rc = mrl::need_healthy(sim)) return rc;
    if (int rc = mrl::need_not_capturing(sim, hip_stream, "mrl_rollout_policy")) return rc;
    if (sim->game != MRL_GAME_CARTPOLE && sim->game != MRL_GAME_ACROBOT) {
        mrl::set_error("mrl_rollout_policy: game %d has no policy rollout (Cartpole and Acrobot do)", sim->game);
        return MRL_ERR_INVALID;
    }
    if (sim->exchange.mine) {
        mrl::set_error("mrl_rollout_policy: this simulator is a rank of an exchanged batch (mrl_exchange_create); its step needs the other ranks");
        return MRL_ERR_INVALID;
    }
    if (!policy || !buffers || !policy->params_dev) {
        mrl::set_error("mrl_rollout_policy: null policy, parameter array or buffer description");
        return MRL_ERR_INVALID;
    }
    const uint32_t actions = sim->game == MRL_GAME_CARTPOLE ? 2u : 3u;
    const bool raw = policy->obs_dim == 4 && policy->obs_mode == MRL_OBS_RAW;
    const bool gym = policy->obs_dim == 6 && policy->obs_mode == MRL_OBS_ACROBOT_GYM && sim->game == MRL_GAME_ACROBOT;
    if (policy->hidden != mrl::kPolicyHidden || policy->num_actions != actions || !(raw || gym)) {
        mrl::set_error("mrl_rollout_policy: need hidden = 64, num_actions = %u and (obs_dim, obs_mode) = (4, MRL_OBS_RAW)%s for game %d; got "
                       "hidden %u, num_actions %u, obs_dim %u, obs_mode %u", actions,
                       sim->game == MRL_GAME_ACROBOT ? " or (6, MRL_OBS_ACROBOT_GYM)" : "", sim->game, policy->hidden,
                       policy->num_actions, policy->obs_dim, policy->obs_mode);
        return MRL_ERR_INVALID;
    }
    const mrl_rollout_buffers &b = *buffers;
    const uint32_t T = b.num_steps;
    if (!b.next_obs || !b.next_value || !b.next_done ||
        (T && (!b.obs || !b.actions || !b.logprobs || !b.values || !b.rewards || !b.dones))) {
        mrl::set_error("mrl_rollout_policy: null rollout buffer");
        return MRL_ERR_INVALID;
    }
    const uintptr_t row_align = policy->obs_dim == 4 ? 15u : 7u;  // the observation rows are stored 16 / 8 bytes at a time
    if ((reinterpret_cast<uintptr_t>(b.obs) | reinterpret_cast<uintptr_t>(b.next_obs)) & row_align) {
        mrl::set_error("mrl_rollout_policy: obs and next_obs must start on a %u-byte boundary", (unsigned)row_align + 1u);
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return guarded([&] {
        hipStream_t stream = (hipStream_t)hip_stream;
        mrl_tensor_desc state{}, reset{}, reward{}, action{};
        // (the slot numbers are the same for both games: MRL_CARTPOLE_* == MRL_ACROBOT_*)
        if (!sim->tensor(MRL_CARTPOLE_STATE, &state) || !sim->tensor(MRL_CARTPOLE_RESET, &reset) ||
            !sim->tensor(MRL_CARTPOLE_REWARD, &reward) || !sim->tensor(MRL_CARTPOLE_ACTION, &action))
            throw std::runtime_error("mrl_rollout_policy: the simulator does not export STATE / RESET / REWARD / ACTION");
        const size_t N = sim->num_worlds, D = policy->obs_dim;
        mrl::PolicyActArgs args{};
        args.params = policy->params_dev;
        args.state = static_cast<const float *>(state.data);
        args.reset = static_cast<const int32_t *>(reset.data);
        args.reward = static_cast<const float *>(reward.data);
        args.action_tensor = static_cast<int32_t *>(action.data);
        args.seed = seed;
        args.num_worlds = sim->num_worlds;
        args.flags = policy->flags;
        for (uint32_t k = 0; k <= T; k++) {
            const bool closing = k == T;
            args.obs_row = closing ? b.next_obs : b.obs + k * N * D;
            args.done_row = closing ? b.next_done : b.dones + k * N;
            args.value_row = closing ? b.next_value : b.values + k * N;
            args.reward_row = k ? b.rewards + (k - 1) * N : nullptr;
            args.action_row = closing ? nullptr : b.actions + k * N;
            args.logprob_row = closing ? nullptr : b.logprobs + k * N;
            args.step = first_step + k;
            mrl::launch_policy_act(*policy, args, stream);
            if (closing) break;
            sim->step(nullptr, stream);
            mrl::completed_step(sim, stream);
        }
    });
}

int mrl_gae(const float *rewards, const float *values, const float *dones, const float *next_value, const float *next_done,
            uint32_t num_steps, uint32_t num_worlds, float gamma, float lambda, float *advantages, float *returns, int gpu_id,
            void *hip_stream)
{
    if (!next_value || !next_done || (num_steps && (!rewards || !values || !dones || !advantages || !returns))) {
        mrl::set_error("mrl_gae: null array");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_gae(rewards, values, dones, next_value, next_done, num_steps, num_worlds, gamma, lambda, advantages, returns,
                        (hipStream_t)hip_stream);
    });
}

// what mrl_ppo_update and mrl_mappo_update (`what`) refuse alike, after their own checks: a workspace smaller than `sizer` asks
// for, arrays or a workspace off their boundaries (`arrays_rule` says which arrays, `arrays_off` whether one of them is), and a
// capturing stream
static int update_refusal(const char *what, const char *sizer, uint64_t workspace_bytes, uint64_t need_bytes, const void *workspace_dev,
                          bool arrays_off, const char *arrays_rule, void *hip_stream)
{
    if (workspace_bytes < need_bytes) {
        mrl::set_error("%s: workspace of %llu bytes, %s asks for %llu", what, (unsigned long long)workspace_bytes, sizer,
                       (unsigned long long)need_bytes);
        return MRL_ERR_INVALID;
    }
    if (arrays_off || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u)) {
        mrl::set_error("%s: %s and the workspace on a 16-byte one", what, arrays_rule);
        return MRL_ERR_INVALID;
    }
    if (mrl::capturing(hip_stream)) {
        mrl::set_error("%s: the Adam step number travels in kernel arguments, so the call cannot be captured in a HIP graph: a replay "
                       "would repeat the same step's bias correction", what);
        return MRL_ERR_INVALID;
    }
    return MRL_OK;
}

static bool ppo_shape_ok(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions)
{
    return hidden == mrl::kPolicyHidden && ((obs_dim == 4 && (num_actions == 2 || num_actions == 3)) || (obs_dim == 6 && num_actions == 3));
}

int mrl_ppo_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t num_actions, uint32_t minibatch_size,
                            uint32_t num_minibatches, uint64_t *out)
{
    if (!out || !ppo_shape_ok(obs_dim, hidden, num_actions) || minibatch_size == 0) {
        mrl::set_error("mrl_ppo_workspace_bytes: need an output pointer, hidden = 64, (obs_dim, num_actions) one of (4, 2), (4, 3), "
                       "(6, 3) and minibatch_size > 0; got hidden %u, obs_dim %u, num_actions %u, minibatch_size %u", hidden, obs_dim,
                       num_actions, minibatch_size);
        return MRL_ERR_INVALID;
    }
    const uint64_t params = mrl_mlp_policy_num_params(obs_dim, hidden, num_actions);
    *out = mrl::ppo_workspace(params, minibatch_size, num_minibatches).total * sizeof(float);
    return MRL_OK;
}

int mrl_ppo_update(const mrl_mlp_policy *shape, const mrl_ppo_optimizer *opt, const mrl_ppo_batch *batch,
                   const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_ppo_config *cfg,
                   void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null, float *grads_dev_or_null, int gpu_id,
                   void *hip_stream)
{
    if (!shape || !opt || !batch || !indices_dev || !cfg || !workspace_dev) {
        mrl::set_error("mrl_ppo_update: null shape, optimizer, batch, index array, configuration or workspace");
        return MRL_ERR_INVALID;
    }
    if (!opt->params_dev || !opt->exp_avg || !opt->exp_avg_sq || !batch->obs || !batch->actions || !batch->logprobs ||
        !batch->advantages || !batch->returns || !batch->values) {
        mrl::set_error("mrl_ppo_update: null parameter, moment or batch array");
        return MRL_ERR_INVALID;
    }
    if (!ppo_shape_ok(shape->obs_dim, shape->hidden, shape->num_actions)) {
        mrl::set_error("mrl_ppo_update: need hidden = 64 and (obs_dim, num_actions) one of (4, 2), (4, 3), (6, 3); got hidden %u, "
                       "obs_dim %u, num_actions %u", shape->hidden, shape->obs_dim, shape->num_actions);
        return MRL_ERR_INVALID;
    }
    if (minibatch_size == 0 || batch->size == 0 || (minibatch_size < 2 && (cfg->flags & MRL_PPO_NORM_ADV))) {
        mrl::set_error("mrl_ppo_update: need minibatch_size > 0 (> 1 with MRL_PPO_NORM_ADV: the unbiased std of one sample does not "
                       "exist) and a batch of at least one sample; got minibatch_size %u, batch size %u", minibatch_size, batch->size);
        return MRL_ERR_INVALID;
    }
    const uint64_t params = mrl_mlp_policy_num_params(shape->obs_dim, shape->hidden, shape->num_actions);
    const uint64_t need_bytes = mrl::ppo_workspace(params, minibatch_size, num_minibatches).total * sizeof(float);
    const bool wide_rows = shape->obs_dim == 4;  // the observation rows are loaded 16 / 8 bytes at a time
    if (int rc = update_refusal("mrl_ppo_update", "mrl_ppo_workspace_bytes", workspace_bytes, need_bytes, workspace_dev,
                                reinterpret_cast<uintptr_t>(batch->obs) & (wide_rows ? 15u : 7u),
                                wide_rows ? "obs must start on a 16-byte boundary" : "obs must start on a 8-byte boundary", hip_stream))
        return rc;
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_ppo_update(*shape, *opt, *batch, indices_dev, num_minibatches, minibatch_size, *cfg,
                               static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream);
    });
}

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

uint64_t mrl_cnn_policy_num_params(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t num_actions)
{
    if (hidden != mrl::kCnnHidden || num_actions != mrl::kCnnActions || width < 3 || height < 3 || channels == 0) return 0;
    return mrl::cnn_net_params(width, height, channels, num_actions) + mrl::cnn_net_params(width, height, channels, 1);
}

uint64_t mrl_cnn_workspace_bytes(uint32_t num_worlds, uint32_t num_players) { return mrl::kCnnWorkspaceBytes; }

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

extern "C++" {
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
}  // extern "C++"

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

int mrl_cnn_act(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, uint32_t row, uint64_t seed,
                uint32_t step, uint32_t flags, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    mrl::CnnActArgs args{};
    if (int rc = cnn_prepare(sim, players, policy, record, hip_stream, "mrl_cnn_act", &args)) return rc;
    if (int rc = act_row_refusal("mrl_cnn_act", "MRL_CNN_VALUE_ONLY", flags, policy->flags, record, row)) return rc;
    const bool value_only = flags & MRL_CNN_VALUE_ONLY;
    if (!workspace_dev || (reinterpret_cast<uintptr_t>(workspace_dev) & 15u) ||
        workspace_bytes < mrl_cnn_workspace_bytes(sim->num_worlds, args.P)) {
        mrl::set_error("mrl_cnn_act: the workspace is null, off a 16-byte boundary or smaller than mrl_cnn_workspace_bytes");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        args.obs = static_cast<const int8_t *>(sim->observation_source());
        if (!args.obs) throw std::runtime_error("mrl_cnn_act: the simulator has no observation slab");
        record_rows(args, record, row, value_only, mrl::kCnnActions);
        args.seed = seed, args.step = step, args.flags = flags;
        mrl::launch_cnn_act(args, (hipStream_t)hip_stream);
    });
}

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

// What mrl_mappo_update and mrl_mappo_mlp_update (`what`; `sizer`: its workspace function) refuse alike.  The network's own part
// comes from the caller once the pointers are known to be there: shape(described) returns why the shape cannot run, or nullptr,
// and describes the shape for the message; actor_params() is the actor's parameter count; obs_words: the batch's observations
// are 4-byte words, to be checked with the other arrays.  members: the workspace must hold that many plain ones (the bank updates).
extern "C++" {
template <class Policy, class Batch, class Shape, class ActorParams>
static int mappo_update_refusal(const char *what, const char *sizer, const Policy *policy, const mrl_mappo_optimizer *opt, const Batch *batch,
                                const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                                float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                                float *grads_dev_or_null, void *hip_stream, bool obs_words, Shape shape, ActorParams actor_params,
                                uint32_t members = 1)
{
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
    const char *why = shape(described, sizeof described);
    if (why || batch->size == 0) {
        mrl::set_error("%s: %s (%s, minibatch_size %u, batch size %u)", what, why ? why : "the batch must hold at least one sample", described,
                       minibatch_size, batch->size);
        return MRL_ERR_INVALID;
    }
    const uint64_t need_bytes = members * mrl::mappo_workspace(actor_params(), minibatch_size, num_minibatches).total * sizeof(float);
    const void *words[] = {opt->params_dev, opt->exp_avg, opt->exp_avg_sq, obs_words ? batch->obs : nullptr, batch->actions, batch->logprobs,
                           batch->value_preds, batch->returns, batch->advantages, indices_dev, value_norm_state, stats_dev_or_null,
                           grads_dev_or_null};
    uintptr_t low_bits = 0;
    for (const void *p : words) low_bits |= reinterpret_cast<uintptr_t>(p) & 3u;
    return update_refusal(what, sizer, workspace_bytes, need_bytes, workspace_dev, low_bits,
                          "the float and int32 arrays must start on 4-byte boundaries", hip_stream);
}

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
}  // extern "C++"

int mrl_mappo_update(const mrl_mappo_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_batch *batch,
                     const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                     float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                     float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    if (int rc = mappo_update_refusal(
            "mrl_mappo_update", "mrl_mappo_workspace_bytes", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg, value_norm_state,
            workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, hip_stream, false,
            [&](char *described, size_t room) {
                snprintf(described, room, "width %u, height %u, channels %u, hidden %u", policy->width, policy->height, policy->channels,
                         policy->hidden);
                return mappo_shape_error(policy->width, policy->height, policy->channels, policy->hidden, minibatch_size);
            },
            [&] { return mrl::cnn_net_params(policy->width, policy->height, policy->channels, mrl::kCnnActions); }))
        return rc;
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_mappo_update(*policy, *opt, *batch, indices_dev, num_minibatches, minibatch_size, *cfg, value_norm_state,
                                 static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream);
    });
}

int mrl_mappo_bank_workspace_bytes(uint32_t width, uint32_t height, uint32_t channels, uint32_t hidden, uint32_t minibatch_size,
                                   uint32_t num_minibatches, uint32_t num_members, uint64_t *out)
{
    if (num_members == 0 || num_members > mrl::kBankMaxPolicies) {
        mrl::set_error("mrl_mappo_bank_workspace_bytes: %u members: a call trains 1 to %u", num_members, mrl::kBankMaxPolicies);
        return MRL_ERR_INVALID;
    }
    if (int rc = mrl_mappo_workspace_bytes(width, height, channels, hidden, minibatch_size, num_minibatches, out)) return rc;
    *out *= num_members;
    return MRL_OK;
}

int mrl_mappo_bank_update(const mrl_mappo_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_batch *batch,
                          const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                          float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                          float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    const char *what = "mrl_mappo_bank_update";
    mrl_mappo_optimizer first{};
    const uint64_t num_params = policy ? mrl_cnn_policy_num_params(policy->width, policy->height, policy->channels, policy->hidden, mrl::kCnnActions) : 0;
    if (int rc = mappo_bank_refusal(what, opt, num_params, &first)) return rc;
    if (int rc = mappo_update_refusal(
            what, "mrl_mappo_bank_workspace_bytes", policy, &first, batch, indices_dev, num_minibatches, minibatch_size, cfg, value_norm_state,
            workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, hip_stream, false,
            [&](char *described, size_t room) {
                snprintf(described, room, "width %u, height %u, channels %u, hidden %u", policy->width, policy->height, policy->channels,
                         policy->hidden);
                return mappo_shape_error(policy->width, policy->height, policy->channels, policy->hidden, minibatch_size);
            },
            [&] { return mrl::cnn_net_params(policy->width, policy->height, policy->channels, mrl::kCnnActions); }, opt->num_members))
        return rc;
    const mrl::MappoMembers members = mappo_bank_members(*opt, &first, &value_norm_state);
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_mappo_update(*policy, first, *batch, indices_dev, num_minibatches, minibatch_size, *cfg, value_norm_state,
                                 static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream, members);
    });
}

int mrl_rollout_cnn(mrl_sim *sim, uint32_t players, const mrl_cnn_policy *policy, const mrl_cnn_record *record, void *obs_ring_dev,
                    uint64_t seed, uint32_t first_step, void *hip_stream)
{
    mrl::CnnActArgs args{};
    if (int rc = cnn_prepare(sim, players, policy, record, hip_stream, "mrl_rollout_cnn", &args)) return rc;
    if (!record || !obs_ring_dev) {
        mrl::set_error("mrl_rollout_cnn: null record or observation ring");
        return MRL_ERR_INVALID;
    }
    args.seed = seed;
    return mrl::cnn_rollout_loop(
        sim, "mrl_rollout_cnn", record->num_steps, obs_ring_dev, hip_stream,
        [&](uint32_t k, const int8_t *obs, bool closing) {
            args.obs = obs;
            record_rows(args, record, k, closing, mrl::kCnnActions);
            args.step = first_step + k;
            args.flags = policy->flags | (closing ? (uint32_t)MRL_CNN_VALUE_ONLY : 0u);
            mrl::launch_cnn_act(args, (hipStream_t)hip_stream);
        },
        [] {});
}

// ---- the policy banks: what the three networks' banks (CNN, MLPBase, wide) check, fill and launch alike ----

uint64_t mrl_cnn_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_players, uint32_t num_policies)
{
    if (num_policies == 0 || num_policies > mrl::kBankMaxPolicies) return 0;
    return mrl::bank_layout(num_worlds, num_players, num_policies).words * sizeof(uint32_t);
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

// A network family as a resample sees it: its games, a bit per MRL_GAME_* (`has`: what any other game is told), the slot of an
// observation tensor and the axis of its shape that holds the seats, the slot of DONE (`tensors`: the two by name).
struct BankFamily {
    uint32_t games;
    const char *has;
    int obs_slot, seat_axis, done_slot;
    const char *tensors;
};
static const BankFamily kCnnFamily{1u << MRL_GAME_OVERCOOKED | 1u << MRL_GAME_SIMPLECOOKED, "no CNN policy (Overcooked and Simplecooked do)",
                                   MRL_OVERCOOKED_OBS_WORLD_MAJOR, 1, MRL_OVERCOOKED_DONE, "OBS_WORLD_MAJOR / DONE"};
static const BankFamily kMlpBaseFamily{1u << MRL_GAME_BALANCE, "no MLPBase policy (the balance beam does)",
                                       MRL_BALANCE_OBSERVATION, 0, MRL_BALANCE_DONE, "OBSERVATION / DONE"};
// (the slot numbers are the same for both games)
static const BankFamily kWideFamily{1u << MRL_GAME_HANABI | 1u << MRL_GAME_BALANCE, "no wide-policy agent (Hanabi and the balance beam do)",
                                    MRL_HANABI_OBSERVATION, 0, MRL_HANABI_DONE, "OBSERVATION / DONE"};

// What mrl_*_bank_resample and the bank rollouts check of a resample on a simulator of `family`; fills `args`.
static int bank_resample_prepare(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
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
static int bank_resample(mrl_sim *sim, const BankFamily &family, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev,
                         int32_t *episodes_dev, void *hip_stream, const char *what)
{
    mrl::CnnResampleArgs args{};
    if (int rc = bank_resample_prepare(sim, family, players, resample, ids_dev, episodes_dev, what, &args)) return rc;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] { mrl::launch_cnn_bank_resample(args, (hipStream_t)hip_stream); });
}

int mrl_cnn_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                          void *hip_stream)
{
    return bank_resample(sim, kCnnFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_cnn_bank_resample");
}

int mrl_mlpbase_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                              void *hip_stream)
{
    return bank_resample(sim, kMlpBaseFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_mlpbase_bank_resample");
}

int mrl_agent_bank_resample(mrl_sim *sim, uint32_t players, const mrl_cnn_resample *resample, int32_t *ids_dev, int32_t *episodes_dev,
                            void *hip_stream)
{
    return bank_resample(sim, kWideFamily, players, resample, ids_dev, episodes_dev, hip_stream, "mrl_agent_bank_resample");
}

// Everything mrl_cnn_act_bank and mrl_rollout_cnn_bank check alike (cnn_prepare's checks and the bank's own); fills `args` but
// for the observation pointer, the rows, the ids row, the seed, the step and the flags.
static int cnn_bank_prepare(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, const int32_t *ids_dev, const mrl_cnn_record *record,
                            void *workspace_dev, uint64_t workspace_bytes, void *hip_stream, const char *what, mrl::CnnBankArgs *args)
{
    return mrl::bank_prepare(
        what, "mrl_cnn_bank_workspace_bytes", bank, ids_dev, workspace_dev, workspace_bytes, args,
        [&] {
            const mrl_cnn_policy row0{bank->params_dev, bank->hidden, bank->flags};
            return cnn_prepare(sim, players, &row0, record, hip_stream, what, &args->act);
        },
        [&] { return mrl_cnn_policy_num_params(args->act.W, args->act.H, args->act.F, mrl::kCnnHidden, mrl::kCnnActions); });
}

int mrl_cnn_act_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, const int32_t *ids_dev, const mrl_cnn_record *record,
                     int32_t *ids_row, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags, void *workspace_dev,
                     uint64_t workspace_bytes, void *hip_stream)
{
    mrl::CnnBankArgs args{};
    if (int rc = cnn_bank_prepare(sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, "mrl_cnn_act_bank", &args))
        return rc;
    if (int rc = act_row_refusal("mrl_cnn_act_bank", "MRL_CNN_VALUE_ONLY", flags, bank->flags, record, row)) return rc;
    const bool value_only = flags & MRL_CNN_VALUE_ONLY;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        args.act.obs = static_cast<const int8_t *>(sim->observation_source());
        if (!args.act.obs) throw std::runtime_error("mrl_cnn_act_bank: the simulator has no observation slab");
        record_rows(args.act, record, row, value_only, mrl::kCnnActions);
        args.act.seed = seed, args.act.step = step, args.act.flags = flags;
        args.bank.ids_row = ids_row;
        mrl::launch_cnn_act_bank(args, (hipStream_t)hip_stream);
    });
}

int mrl_rollout_cnn_bank(mrl_sim *sim, uint32_t players, const mrl_cnn_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                         const mrl_cnn_resample *resample, const mrl_cnn_record *record, int32_t *ids_record, void *obs_ring_dev, uint64_t seed,
                         uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    const char *what = "mrl_rollout_cnn_bank";
    mrl::CnnBankArgs args{};
    if (int rc = cnn_bank_prepare(sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, what, &args)) return rc;
    if (!record || !obs_ring_dev) {
        mrl::set_error("%s: null record or observation ring", what);
        return MRL_ERR_INVALID;
    }
    mrl::CnnResampleArgs again{};
    if (resample)
        if (int rc = bank_resample_prepare(sim, kCnnFamily, players, resample, ids_dev, episodes_dev, what, &again)) return rc;
    args.act.seed = seed;
    const size_t cells = (size_t)args.act.num_worlds * args.act.P;
    return mrl::cnn_rollout_loop(
        sim, what, record->num_steps, obs_ring_dev, hip_stream,
        [&](uint32_t k, const int8_t *obs, bool closing) {
            args.act.obs = obs;
            record_rows(args.act, record, k, closing, mrl::kCnnActions);
            args.act.step = first_step + k;
            args.act.flags = bank->flags | (closing ? (uint32_t)MRL_CNN_VALUE_ONLY : 0u);
            args.bank.ids_row = ids_record ? ids_record + (size_t)k * cells : nullptr;
            mrl::launch_cnn_act_bank(args, (hipStream_t)hip_stream);
        },
        [&] {
            if (resample) mrl::launch_cnn_bank_resample(again, (hipStream_t)hip_stream);
        });
}

uint64_t mrl_mlpbase_policy_num_params(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions)
{
    if (obs_dim != mrl::kMlpBaseObs || hidden != mrl::kMlpBaseHidden || layer_N < 1 || layer_N > mrl::kMlpBaseMaxLayerN ||
        num_actions != mrl::kMlpBaseActions)
        return 0;
    return (uint64_t)mrl::mlpbase_net_params(layer_N, num_actions) + mrl::mlpbase_net_params(layer_N, 1);
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

int mrl_mlpbase_act(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record, uint32_t row,
                    uint64_t seed, uint32_t step, uint32_t flags, void *hip_stream)
{
    mrl::MlpBaseActArgs args{};
    if (int rc = mlpbase_prepare(sim, players, policy, record, hip_stream, "mrl_mlpbase_act", &args)) return rc;
    if (int rc = act_row_refusal("mrl_mlpbase_act", "MRL_MLPBASE_VALUE_ONLY", flags, policy->flags, record, row)) return rc;
    const bool value_only = flags & MRL_MLPBASE_VALUE_ONLY;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        mlpbase_rows(args, record, row, value_only);
        args.seed = seed, args.step = step, args.flags = flags;
        mrl::launch_mlpbase_act(args, (hipStream_t)hip_stream);
    });
}

int mrl_rollout_mlpbase(mrl_sim *sim, uint32_t players, const mrl_mlpbase_policy *policy, const mrl_mlpbase_record *record, uint64_t seed,
                        uint32_t first_step, void *hip_stream)
{
    mrl::MlpBaseActArgs args{};
    if (int rc = mlpbase_prepare(sim, players, policy, record, hip_stream, "mrl_rollout_mlpbase", &args)) return rc;
    if (!record) {
        mrl::set_error("mrl_rollout_mlpbase: null record");
        return MRL_ERR_INVALID;
    }
    args.seed = seed;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        mrl::rollout_loop(
            sim, record->num_steps, (hipStream_t)hip_stream,
            [&](uint32_t k, bool closing) {
                mlpbase_rows(args, record, k, closing);
                args.step = first_step + k;
                args.flags = policy->flags | (closing ? (uint32_t)MRL_MLPBASE_VALUE_ONLY : 0u);
                mrl::launch_mlpbase_act(args, (hipStream_t)hip_stream);
            },
            [] {});
    });
}

// Everything mrl_mlpbase_act_bank and mrl_rollout_mlpbase_bank check alike (mlpbase_prepare's checks and the bank's own); fills
// `args` but for the rows, the ids row, the seed, the step and the flags.
static int mlpbase_bank_prepare(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, const int32_t *ids_dev,
                                const mrl_mlpbase_record *record, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream,
                                const char *what, mrl::MlpBaseBankArgs *args)
{
    return mrl::bank_prepare(
        what, "mrl_mlpbase_bank_workspace_bytes", bank, ids_dev, workspace_dev, workspace_bytes, args,
        [&] {
            const mrl_mlpbase_policy row0{bank->params_dev, bank->hidden, bank->layer_N, bank->flags};
            return mlpbase_prepare(sim, players, &row0, record, hip_stream, what, &args->act);
        },
        [&] { return mrl_mlpbase_policy_num_params(mrl::kMlpBaseObs, mrl::kMlpBaseHidden, bank->layer_N, mrl::kMlpBaseActions); });
}

uint64_t mrl_mlpbase_bank_workspace_bytes(uint32_t num_worlds, uint32_t num_policies)
{
    return mrl_cnn_bank_workspace_bytes(num_worlds, 2, num_policies);  // the balance beam seats two
}

int mrl_mlpbase_act_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, const int32_t *ids_dev,
                         const mrl_mlpbase_record *record, int32_t *ids_row, uint32_t row, uint64_t seed, uint32_t step, uint32_t flags,
                         void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    mrl::MlpBaseBankArgs args{};
    if (int rc = mlpbase_bank_prepare(sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, "mrl_mlpbase_act_bank",
                                      &args))
        return rc;
    if (int rc = act_row_refusal("mrl_mlpbase_act_bank", "MRL_MLPBASE_VALUE_ONLY", flags, bank->flags, record, row)) return rc;
    if (reinterpret_cast<uintptr_t>(ids_row) & 3u) {
        mrl::set_error("mrl_mlpbase_act_bank: ids_row is off a 4-byte boundary");
        return MRL_ERR_INVALID;
    }
    const bool value_only = flags & MRL_MLPBASE_VALUE_ONLY;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        mlpbase_rows(args.act, record, row, value_only);
        args.act.seed = seed, args.act.step = step, args.act.flags = flags;
        args.bank.ids_row = ids_row;
        mrl::launch_mlpbase_act_bank(args, (hipStream_t)hip_stream);
    });
}

int mrl_rollout_mlpbase_bank(mrl_sim *sim, uint32_t players, const mrl_mlpbase_bank *bank, int32_t *ids_dev, int32_t *episodes_dev,
                             const mrl_cnn_resample *resample, const mrl_mlpbase_record *record, int32_t *ids_record, uint64_t seed,
                             uint32_t first_step, void *workspace_dev, uint64_t workspace_bytes, void *hip_stream)
{
    const char *what = "mrl_rollout_mlpbase_bank";
    mrl::MlpBaseBankArgs args{};
    if (int rc = mlpbase_bank_prepare(sim, players, bank, ids_dev, record, workspace_dev, workspace_bytes, hip_stream, what, &args)) return rc;
    if (!record) {
        mrl::set_error("%s: null record", what);
        return MRL_ERR_INVALID;
    }
    if (reinterpret_cast<uintptr_t>(ids_record) & 3u) {
        mrl::set_error("%s: ids_record is off a 4-byte boundary", what);
        return MRL_ERR_INVALID;
    }
    mrl::CnnResampleArgs again{};
    if (resample)
        if (int rc = bank_resample_prepare(sim, kMlpBaseFamily, players, resample, ids_dev, episodes_dev, what, &again)) return rc;
    args.act.seed = seed;
    const size_t cells = (size_t)args.act.num_worlds * args.act.P;
    mrl::DeviceGuard on(sim->device);
    return mrl::guarded([&] {
        mrl::rollout_loop(
            sim, record->num_steps, (hipStream_t)hip_stream,
            [&](uint32_t k, bool closing) {
                mlpbase_rows(args.act, record, k, closing);
                args.act.step = first_step + k;
                args.act.flags = bank->flags | (closing ? (uint32_t)MRL_MLPBASE_VALUE_ONLY : 0u);
                args.bank.ids_row = ids_record ? ids_record + (size_t)k * cells : nullptr;
                mrl::launch_mlpbase_act_bank(args, (hipStream_t)hip_stream);
            },
            [&] {
                if (resample) mrl::launch_cnn_bank_resample(again, (hipStream_t)hip_stream);
            });
    });
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

// what mrl_mappo_mlp_workspace_bytes and mrl_mappo_mlp_update refuse alike: nullptr when the shape can run, else why not
static const char *mappo_mlp_shape_error(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size)
{
    if (hidden != mrl::kMlpBaseHidden) return "hidden must be 64";
    if (layer_N < 1 || layer_N > mrl::kMlpBaseMaxLayerN) return "layer_N must be 1 or 2";
    if (obs_dim != mrl::kMlpBaseObs || num_actions != mrl::kMlpBaseActions) return "obs_dim must be 7 and num_actions 4";
    if (minibatch_size == 0) return "minibatch_size must be positive";
    return nullptr;
}

int mrl_mappo_mlp_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                  uint32_t num_minibatches, uint64_t *out)
{
    const char *why = out ? mappo_mlp_shape_error(obs_dim, hidden, layer_N, num_actions, minibatch_size) : "null output pointer";
    if (why) {
        mrl::set_error("mrl_mappo_mlp_workspace_bytes: %s (obs_dim %u, hidden %u, layer_N %u, num_actions %u, minibatch_size %u)", why, obs_dim,
                       hidden, layer_N, num_actions, minibatch_size);
        return MRL_ERR_INVALID;
    }
    *out = mrl::mappo_workspace(mrl::mlpbase_net_params(layer_N, num_actions), minibatch_size, num_minibatches).total * sizeof(float);
    return MRL_OK;
}

int mrl_mappo_mlp_update(const mrl_mlpbase_policy *policy, const mrl_mappo_optimizer *opt, const mrl_mappo_mlp_batch *batch,
                         const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                         float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                         float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    if (int rc = mappo_update_refusal(
            "mrl_mappo_mlp_update", "mrl_mappo_mlp_workspace_bytes", policy, opt, batch, indices_dev, num_minibatches, minibatch_size, cfg,
            value_norm_state, workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, hip_stream, true,
            [&](char *described, size_t room) {
                snprintf(described, room, "hidden %u, layer_N %u", policy->hidden, policy->layer_N);
                return mappo_mlp_shape_error(mrl::kMlpBaseObs, policy->hidden, policy->layer_N, mrl::kMlpBaseActions, minibatch_size);
            },
            [&] { return (uint64_t)mrl::mlpbase_net_params(policy->layer_N, mrl::kMlpBaseActions); }))
        return rc;
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_mappo_mlp_update(policy->layer_N, *opt, *batch, indices_dev, num_minibatches, minibatch_size, *cfg, value_norm_state,
                                     static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream);
    });
}

int mrl_mappo_mlp_bank_workspace_bytes(uint32_t obs_dim, uint32_t hidden, uint32_t layer_N, uint32_t num_actions, uint32_t minibatch_size,
                                       uint32_t num_minibatches, uint32_t num_members, uint64_t *out)
{
    if (num_members == 0 || num_members > mrl::kBankMaxPolicies) {
        mrl::set_error("mrl_mappo_mlp_bank_workspace_bytes: %u members: a call trains 1 to %u", num_members, mrl::kBankMaxPolicies);
        return MRL_ERR_INVALID;
    }
    if (int rc = mrl_mappo_mlp_workspace_bytes(obs_dim, hidden, layer_N, num_actions, minibatch_size, num_minibatches, out)) return rc;
    *out *= num_members;
    return MRL_OK;
}

int mrl_mappo_mlp_bank_update(const mrl_mlpbase_policy *policy, const mrl_mappo_bank_optimizer *opt, const mrl_mappo_mlp_batch *batch,
                              const int32_t *indices_dev, uint32_t num_minibatches, uint32_t minibatch_size, const mrl_mappo_config *cfg,
                              float *value_norm_state, void *workspace_dev, uint64_t workspace_bytes, float *stats_dev_or_null,
                              float *grads_dev_or_null, int gpu_id, void *hip_stream)
{
    const char *what = "mrl_mappo_mlp_bank_update";
    mrl_mappo_optimizer first{};
    const uint64_t num_params = policy ? mrl_mlpbase_policy_num_params(mrl::kMlpBaseObs, policy->hidden, policy->layer_N, mrl::kMlpBaseActions) : 0;
    if (int rc = mappo_bank_refusal(what, opt, num_params, &first)) return rc;
    if (int rc = mappo_update_refusal(
            what, "mrl_mappo_mlp_bank_workspace_bytes", policy, &first, batch, indices_dev, num_minibatches, minibatch_size, cfg, value_norm_state,
            workspace_dev, workspace_bytes, stats_dev_or_null, grads_dev_or_null, hip_stream, true,
            [&](char *described, size_t room) {
                snprintf(described, room, "hidden %u, layer_N %u", policy->hidden, policy->layer_N);
                return mappo_mlp_shape_error(mrl::kMlpBaseObs, policy->hidden, policy->layer_N, mrl::kMlpBaseActions, minibatch_size);
            },
            [&] { return (uint64_t)mrl::mlpbase_net_params(policy->layer_N, mrl::kMlpBaseActions); }, opt->num_members))
        return rc;
    const mrl::MappoMembers members = mappo_bank_members(*opt, &first, &value_norm_state);
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        mrl::launch_mappo_mlp_update(policy->layer_N, first, *batch, indices_dev, num_minibatches, minibatch_size, *cfg, value_norm_state,
                                     static_cast<float *>(workspace_dev), stats_dev_or_null, grads_dev_or_null, (hipStream_t)hip_stream, members);
    });
}

int mrl_tensor(mrl_sim *sim, int slot, mrl_tensor_desc *out)
{
    if (int rc = mrl::need(sim)) return rc;
    mrl::DeviceGuard on(sim->device);
    if (!out) return MRL_ERR_INVALID;
    int rc = MRL_OK;
    int g = guarded([&] {
        memset(out, 0, sizeof(*out));
        if (!sim->tensor(slot, out) && !(sim->stats && sim->stats->tensor(slot, out))) {
            mrl::set_error("tensor slot %d is not exported by game %d", slot, sim->game);
            rc = MRL_ERR_SLOT;
        }
    });
    return g != MRL_OK ? g : rc;
}

int mrl_game(const mrl_sim *sim) { return sim ? sim->game : 0; }
uint32_t mrl_num_worlds(const mrl_sim *sim) { return sim ? sim->num_worlds : 0; }
const char *mrl_kernel_name(const mrl_sim *sim) { return sim ? sim->kernel_name() : ""; }
const char *mrl_rollout_kernel_name(const mrl_sim *sim) { return sim ? sim->rollout_kernel_name() : ""; }
uint64_t mrl_bytes_per_world_step(const mrl_sim *sim) { return sim ? sim->bytes_per_world_step() : 0; }

void mrl_destroy(mrl_sim *sim)
{
    if (!sim) return;
    mrl::DeviceGuard on(sim->device);
    (void)hipDeviceSynchronize();
    delete sim;
}

int mrl_launch_shape(const mrl_sim *sim, uint32_t out[4])
{
    if (!sim || !out) return MRL_ERR_INVALID;
    sim->launch_shape(out);
    return MRL_OK;
}

int mrl_scan_timed_out(const mrl_sim *sim) { return sim && sim->scan_timed_out() ? 1 : 0; }

int mrl_debug_set(const char *key, int64_t value)
{
    if (!key) {  // forget everything
        std::lock_guard<std::mutex> lock(mrl::g_debug_mutex);
        mrl::g_debug.clear();
        return MRL_OK;
    }
    for (const char *known : mrl::kDebugKeys)
        if (strcmp(known, key) == 0) {
            std::lock_guard<std::mutex> lock(mrl::g_debug_mutex);
            mrl::g_debug[key] = value;
            return MRL_OK;
        }
    mrl::set_error("mrl_debug_set: unknown key '%s'", key);
    return MRL_ERR_INVALID;
}

int mrl_probe_stream(void *dst_dev, const void *src_dev, uint64_t bytes, int mode, int gpu_id, void *hip_stream)
{
    if (!dst_dev || (mode == 0 && !src_dev) || mode < 0 || mode > 4 || bytes < 16 || (bytes & 15u) ||
        (reinterpret_cast<uintptr_t>(dst_dev) & 15u) || (reinterpret_cast<uintptr_t>(src_dev) & 15u)) {
        mrl::set_error("mrl_probe_stream: need 16-byte aligned device buffers, a multiple of 16 bytes and mode 0..4");
        return MRL_ERR_INVALID;
    }
    mrl::DeviceGuard on(gpu_id);
    return guarded([&] {
        const size_t chunks = bytes / 16;
        const unsigned grid = (unsigned)std::min<size_t>((chunks + 1023) / 1024, 256 * 32);
        auto *dst = static_cast<mrl::f32x4 *>(dst_dev);
        auto *src = static_cast<const mrl::f32x4 *>(src_dev);
        hipStream_t stream = (hipStream_t)hip_stream;
        if (mode == 0)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<0>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 1)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<1>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 2)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_kernel<2>), dim3(grid), dim3(256), 0, stream, dst, src, chunks);
        else if (mode == 3)
            hipLaunchKernelGGL((mrl::mrl_probe_stream_two_pass_kernel<64>), dim3(grid), dim3(256), 0, stream, dst, chunks);
        else
            hipLaunchKernelGGL((mrl::mrl_probe_stream_two_pass_kernel<128>), dim3(grid), dim3(256), 0, stream, dst, chunks);
        MRL_HIP(hipGetLastError());
    });
}

}  // extern "C"
