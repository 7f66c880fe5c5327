// Host side of what the two kitchen simulators share (OvercookedSim in overcooked.hip, SimplecookedSim in
// simplecooked.hip; the device side is grid_common.hpp): reading a layout out of the config, the tables the kernels
// index by group, and KitchenSim -- the exported tensors, the observation ring with its staging, the reset of chosen
// worlds.  Host-only code; the two fill kernels it needs live in world_reset.hip.
#pragma once

#include "common.hpp"
#include "grid_common.hpp"
#include "world_reset.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace mrl {
// world_reset.hip; on the null stream.  fill_ids: world_id[i] = i % n, row_id[i] = i / n for i < rows * n
void fill_ids(int32_t *world_id, int32_t *row_id, uint32_t rows, uint32_t n);
void fill_i32(int32_t *dst, int32_t value, size_t count);
}  // namespace mrl

namespace mrl_kitchen {

// The TerrainT values the two games agree on (each game's own enum T_* names the rest, which they number differently).
enum : uint32_t { kAir = 0, kPot = 1, kCounter = 2 };

// What differs between the games' config checks: the limits and what the messages cite.
struct Rules {
    const char *game;         // prefix of every message
    int64_t max_cells;
    const char *cells_why;
    int64_t max_players;
    const char *players_why;
    const char *neighbours;   // where the reference's step indexes neighbours without bounds checks
};

struct Kitchen {
    int64_t H = 0, W = 0, P = 0, C = 0;
    uint32_t num_pots = 0;
    uint8_t terrain[256] = {};  // TerrainT per cell
    uint8_t pots[256] = {};     // cells holding a pot, ascending
    uint8_t start[64] = {};     // start cell of each player
};

// The checked layout of a config; sets the error and throws HipError{MRL_ERR_INVALID} on the first thing wrong.
inline Kitchen read_config(const mrl_overcooked_config *cfg, uint32_t num_worlds, const Rules &r)
{
    const auto invalid = [] { return mrl::HipError{MRL_ERR_INVALID}; };
    if (!cfg || !cfg->terrain || !cfg->start_player_x || !cfg->start_player_y || !cfg->recipe_values || !cfg->recipe_times) {
        mrl::set_error("%s: null config field", r.game);
        throw invalid();
    }
    Kitchen k;
    const int64_t H = k.H = cfg->height, W = k.W = cfg->width, P = k.P = cfg->num_players;
    if (H < 3 || W < 3 || H * W > r.max_cells) {
        mrl::set_error("%s: height*width must be 9..%lld (%s), got %lldx%lld", r.game, (long long)r.max_cells, r.cells_why, (long long)H,
                       (long long)W);
        throw invalid();
    }
    if (P < 1 || P > r.max_players) {
        mrl::set_error("%s: num_players must be 1..%lld (%s), got %lld", r.game, (long long)r.max_players, r.players_why, (long long)P);
        throw invalid();
    }
    if (num_worlds == 0) {
        mrl::set_error("%s: num_worlds must be > 0", r.game);
        throw invalid();
    }
    k.C = H * W;
    for (int64_t c = 0; c < k.C; c++) {
        const int64_t t = cfg->terrain[c];
        if (t < 0 || t > 6) {
            mrl::set_error("%s: terrain[%lld] = %lld is not a TerrainT value", r.game, (long long)c, (long long)t);
            throw invalid();
        }
        const int64_t x = c % W, y = c / W;
        if (t == kAir && (x == 0 || y == 0 || x == W - 1 || y == H - 1)) {
            mrl::set_error("%s: walkable cell on the grid border at (%lld,%lld); the step indexes neighbours without bounds checks (%s)",
                           r.game, (long long)x, (long long)y, r.neighbours);
            throw invalid();
        }
        k.terrain[c] = (uint8_t)t;
        if (t == kPot) k.pots[k.num_pots++] = (uint8_t)c;
    }
    for (int64_t q = 0; q < P; q++) {
        const int64_t x = cfg->start_player_x[q], y = cfg->start_player_y[q];
        if (x < 1 || y < 1 || x >= W - 1 || y >= H - 1) {
            mrl::set_error("%s: start position of player %lld (%lld,%lld) is not an interior cell", r.game, (long long)q, (long long)x,
                           (long long)y);
            throw invalid();
        }
        k.start[q] = (uint8_t)(y * W + x);
    }
    return k;
}

// The direct encode (patch_direct in overcooked.hip) needs no search for what is dynamic: players only ever stand on
// AIR cells and objects only ever lie on HOLDER cells -- counters and pots next to a walkable cell, which a player can
// face.  The holder cells in ascending order, each as cell | is_pot << 8.
inline std::vector<uint32_t> holder_cells(const Kitchen &k)
{
    std::vector<uint32_t> holders;
    for (int64_t c = 0; c < k.C; c++) {
        const uint32_t t = k.terrain[c];
        if (t != kCounter && t != kPot) continue;
        const int64_t x = c % k.W, y = c / k.W;
        const bool faced = (x > 0 && k.terrain[c - 1] == kAir) || (x + 1 < k.W && k.terrain[c + 1] == kAir) ||
                           (y > 0 && k.terrain[c - k.W] == kAir) || (y + 1 < k.H && k.terrain[c + k.W] == kAir);
        if (faced) holders.push_back((uint32_t)c | (t == kPot ? 0x100u : 0u));
    }
    return holders;
}

// ... which also wants every player to start on a walkable cell
inline bool starts_walkable(const Kitchen &k)
{
    bool ok = true;
    for (int64_t q = 0; q < k.P; q++) ok = ok && k.terrain[k.start[q]] == kAir;
    return ok;
}

// The holder cells of a group of `gw` worlds as the kernels read them, entry [round * 64 + lane]: tile offset of the
// cell's viewer-0 row | cell index in the group << 16 | 1 << 30 | is_pot << 31.  Round 0 keeps lanes [0, gw * P) for
// the players.  F: bytes of an observation row.  Never empty.
inline std::vector<uint32_t> hold_table(const Kitchen &k, const std::vector<uint32_t> &holders, uint32_t gw, uint32_t F)
{
    const uint32_t P = (uint32_t)k.P, C = (uint32_t)k.C, block_bytes = P * C * F;
    std::vector<uint32_t> tab;
    const uint32_t free0 = (uint32_t)mrl_grid::kWave - std::min<uint32_t>((uint32_t)mrl_grid::kWave, gw * P);
    uint32_t s = 0;
    for (uint32_t l = 0; l < gw; l++)
        for (const uint32_t h : holders) {
            const uint32_t c = h & 0xFFu;
            const uint32_t slot = s < free0 ? gw * P + s : (uint32_t)mrl_grid::kWave + (s - free0);
            if (tab.size() <= slot) tab.resize(slot + 1, 0u);
            tab[slot] = (l * block_bytes + c * F) | ((l * C + c) << 16) | (1u << 30) | ((h >> 8) << 31);
            s++;
        }
    if (tab.empty()) tab.resize(1, 0u);
    return tab;
}

// Per observation row of a group of `gw` worlds (row = world, viewer, cell): the tile offset of its terrain one-hot
// byte (channel 5P + t - 1), 0 = none -- no terrain byte sits at offset 0.  `no_byte`: bit t set for the terrain
// values without a visible byte (AIR in both games).
inline std::vector<uint16_t> terrain_offsets(const Kitchen &k, uint32_t gw, uint32_t F, uint32_t no_byte)
{
    const uint32_t P = (uint32_t)k.P, C = (uint32_t)k.C, rows = P * C;
    std::vector<uint16_t> off((size_t)gw * rows, 0);
    for (uint32_t l = 0; l < gw; l++)
        for (uint32_t v = 0; v < P; v++)
            for (uint32_t c = 0; c < C; c++) {
                const uint32_t t = k.terrain[c];
                if (!((no_byte >> t) & 1u)) off[l * rows + v * C + c] = (uint16_t)((l * rows + v * C + c) * F + 5 * P + t - 1);
            }
    return off;
}

// Store flavour of the single-pass stream-out (grid_common.hpp, stream_store_rsrc): write-through, except where a
// group's slab is not whole 128-byte lines AND either the slab is larger than the 256 MiB Infinity Cache or the launch
// is a multi-step one -- then ordinary stores, which the L2 merges.  (The multi-step launches rewrite the same lines
// step after step and do better with ordinary stores for such groups at every size: asymmetric_advantages 32768 worlds
// 10.6 -> 9.3 us per step, 65536 21.2 -> 18.6, coordination_ring 6.61 -> 6.44; the single step inside the cache does
// not: coordination_ring 10.5 vs 12.0, asymmetric_advantages 15.6 vs 17.3.)
// mrl_debug_set overcooked.whole_store: 0 = that rule, 1 = write-through, 2 = plain.
inline bool plain_store(uint32_t num_worlds, uint32_t block_bytes, uint32_t group_worlds, bool multi_step)
{
    const int64_t knob = mrl::debug_get("overcooked.whole_store", 0);
    const uint64_t slab = (uint64_t)num_worlds * block_bytes;
    const bool whole_lines = ((uint64_t)group_worlds * block_bytes) % 64u == 0;  // (64: Simplecooked random0's 8000-byte groups, half a 128-byte line off, do not care)
    return knob ? knob == 2 : (!whole_lines && (multi_step || slab > (256ull << 20)));
}

// a host table's copy in device memory, owned by the arena
template <typename T> T *upload(mrl::DeviceArena &arena, const T *data, size_t count)
{
    T *d = arena.alloc<T>(count, false);
    MRL_HIP(hipMemcpy(d, data, count * sizeof(T), hipMemcpyHostToDevice));
    return d;
}
template <typename T> T *upload(mrl::DeviceArena &arena, const std::vector<T> &v) { return upload(arena, v.data(), v.size()); }

// A group's two tables in ONE allocation: the terrain offsets, then the holder table at a 4-byte aligned offset that depends
// on the number of terrain entries alone -- a kernel compiled for one layout size reaches both through the one pointer it
// is handed in registers (overcooked.hip, take_hot_args).
constexpr uint32_t hold_tab_offset(uint32_t terr_entries) { return (terr_entries * 2u + 3u) & ~3u; }
struct GroupTables {
    const uint16_t *terr_off;
    const uint32_t *hold_tab;
};
inline GroupTables upload_group_tables(mrl::DeviceArena &arena, const std::vector<uint16_t> &terr, const std::vector<uint32_t> &hold)
{
    const uint32_t at = hold_tab_offset((uint32_t)terr.size());
    std::vector<uint8_t> both(at + hold.size() * sizeof(uint32_t), 0);
    std::memcpy(both.data(), terr.data(), terr.size() * sizeof(uint16_t));
    std::memcpy(both.data() + at, hold.data(), hold.size() * sizeof(uint32_t));
    const uint8_t *d = upload(arena, both);
    return {reinterpret_cast<const uint16_t *>(d), reinterpret_cast<const uint32_t *>(d + at)};
}

// What a kitchen simulator is around its step kernels.  Params is the game's kernel-argument struct; this code reads its
// P, C, W, F, rows, block_bytes and the done / reward / players / cell_obj pointers, and never writes it: where a step
// writes its observations reaches the game through ring_changed.
template <class Params> struct KitchenSim : mrl_sim {
    Params params{};
    uint32_t H = 0, grid = 0, lds_bytes = 0;
    int32_t *action = nullptr, *active = nullptr, *mask = nullptr;
    int32_t *world_id = nullptr, *agent_id = nullptr, *loc_world_id = nullptr, *loc_id = nullptr;
    uint8_t *own_obs = nullptr;  // the OBS_WORLD_MAJOR buffer; the kernels' `obs` points elsewhere while the output is redirected

    // The kernels take the slab's address from the launch arguments and never read it back, so writing a step's
    // observations into a caller's slot (a rollout buffer) instead of the exported tensor is a different pointer in
    // the same launch: same bytes, same stores.
    uint64_t observation_bytes() const override { return (uint64_t)num_worlds * params.block_bytes; }
    uint64_t set_observation_output(void *out) override
    {
        set_observation_ring(out, 0, 1);
        return observation_bytes();
    }
    // a ring of slots: the step number `ring_pos` since this call writes slot ring_pos % slots (host-side count: a
    // launch captured in a HIP graph keeps the slot it was captured with)
    uint8_t *ring_base = nullptr;
    uint64_t ring_stride = 0;
    uint32_t ring_slots = 1;
    uint64_t ring_pos = 0;
    // Slots that do not start on 16-byte boundaries (a dense (T, N, P, H, W, F) buffer whose N x P x H x W x F is not a
    // multiple of 16: coordination_ring at 1001 worlds) are STAGED: the kernels stream a slab out in 16-byte chunks from a
    // 16-byte aligned base, so the step writes a slab of the simulator's (`staging`, allocated at the first such call; the
    // exported tensor stays untouched) and a device-to-device copy behind the launch moves it to the slot -- one more pass
    // over the slab per step, and the multi-step launches run one launch per step.  Aligned slots cost nothing.
    bool staged = false;
    uint8_t *staging = nullptr;
    // the game's params (all copies it keeps) take: obs, ring_stride, ring_slots as given, ring_first = 0
    virtual void ring_changed(uint8_t *obs, uint64_t stride, uint32_t slots) = 0;
    void set_observation_ring(void *base, uint64_t stride_bytes, uint32_t slots) override
    {
        ring_base = base ? static_cast<uint8_t *>(base) : own_obs;
        ring_stride = base ? stride_bytes : 0;
        ring_slots = base && slots > 1 ? slots : 1;
        ring_pos = 0;
        staged = base && ((reinterpret_cast<uintptr_t>(base) & 15u) != 0 || (ring_slots > 1 && (ring_stride & 15u) != 0));
        if (staged && !staging) staging = arena.alloc<uint8_t>(observation_bytes(), false);
        if (staged)
            ring_changed(staging, 0, 1);
        else
            ring_changed(ring_base, ring_stride, ring_slots);
    }
    const void *observation_source() const override
    {
        const uint64_t slot = ring_pos ? (ring_pos - 1) % ring_slots : 0;
        return ring_base + (size_t)slot * ring_stride;
    }
    ObservationRing observation_ring() const override
    {
        ObservationRing ring;
        ring.base = ring_base == own_obs ? nullptr : ring_base;
        ring.stride = ring_stride, ring.slots = ring_slots, ring.position = ring_pos;
        return ring;
    }
    void restore_observation_ring(const ObservationRing &ring) override
    {
        set_observation_ring(ring.base, ring.stride, ring.slots);
        ring_pos = ring.position;
    }
    // the slot(s) of the next `steps` steps: single-step launches get the slot as their `obs`, multi-step ones the first index
    uint8_t *take_slots(uint32_t steps, uint32_t *first)
    {
        const uint32_t at = (uint32_t)(ring_pos % ring_slots);
        ring_pos += steps;
        if (first) *first = at;
        return ring_base + (size_t)at * ring_stride;
    }
    // where a single step that was given slot `dest` writes
    uint8_t *step_obs(uint8_t *dest) const { return staged ? staging : dest; }
    // staged slots: the slab just written -> the caller's slot, behind the launch on the same stream
    void deliver(uint8_t *dest, hipStream_t stream)
    {
        if (staged && dest) MRL_HIP(hipMemcpyAsync(dest, staging, observation_bytes(), hipMemcpyDeviceToDevice, stream));
    }

    // mrl_reset_worlds: world 0 as construction left it, copied over the masked worlds (world_reset.hpp).  The observations go
    // where the most recent step wrote -- before any step since the output was set, where the next step will write.
    mrl::FreshWorldOwner fresh;
    void reset_worlds(const uint8_t *mask_dev, hipStream_t stream) override
    {
        if (staged)
            throw std::runtime_error("mrl_reset_worlds: the observation output is a staged slot (off a 16-byte boundary); a reset writes "
                                     "observations in place only -- use an aligned slot or the simulator's own tensor");
        const uint64_t slot = ring_pos ? (ring_pos - 1) % ring_slots : 0;
        fresh.launch(mask_dev, num_worlds, ring_base + (size_t)slot * ring_stride, stream);
    }

    // construction: the exported observation tensor (the output until a caller redirects it) and the per-agent tensors
    void alloc_outputs()
    {
        const size_t na = (size_t)num_worlds * params.P, nm = na * 6;
        own_obs = arena.alloc<uint8_t>(observation_bytes(), false);
        set_observation_ring(nullptr, 0, 1);
        action = arena.alloc<int32_t>(na);
        active = arena.alloc<int32_t>(na, false);
        mask = arena.alloc<int32_t>(nm, false);
        mrl::fill_i32(active, 1, na);
        mrl::fill_i32(mask, 1, nm);
    }
    void ensure_ids()
    {
        if (world_id) return;
        const uint32_t P = params.P, N = num_worlds, rows = params.rows;
        world_id = arena.alloc<int32_t>((size_t)P * N, false);
        agent_id = arena.alloc<int32_t>((size_t)P * N, false);
        loc_world_id = arena.alloc<int32_t>((size_t)rows * N, false);
        loc_id = arena.alloc<int32_t>((size_t)rows * N, false);
        mrl::fill_ids(world_id, agent_id, P, N);
        mrl::fill_ids(loc_world_id, loc_id, rows, N);
        MRL_HIP(hipDeviceSynchronize());
    }

    // the MRL_OVERCOOKED_* slots that are the same in both games
    bool common_tensor(int slot, mrl_tensor_desc *out)
    {
        const int64_t P = params.P, N = num_worlds, C = params.C, F = params.F, W = params.W;
        switch (slot) {
        case MRL_OVERCOOKED_DONE: *out = mrl::make_desc(params.done, MRL_INT32, device, {N}); return true;
        case MRL_OVERCOOKED_ACTIVE_AGENT: *out = mrl::make_desc(active, MRL_INT32, device, {P, N}); return true;
        case MRL_OVERCOOKED_ACTION: *out = mrl::make_desc(action, MRL_INT32, device, {P, N, 1}); return true;
        case MRL_OVERCOOKED_OBSERVATION:
            *out = mrl::make_desc(own_obs, MRL_INT8, device, {P * C, N, F}, {F, P * C * F, 1});
            return true;
        case MRL_OVERCOOKED_ACTION_MASK: *out = mrl::make_desc(mask, MRL_INT32, device, {P, N, 6}); return true;
        case MRL_OVERCOOKED_REWARD: *out = mrl::make_desc(params.reward, MRL_INT32, device, {P, N}); return true;
        case MRL_OVERCOOKED_WORLD_ID: ensure_ids(); *out = mrl::make_desc(world_id, MRL_INT32, device, {P, N}); return true;
        case MRL_OVERCOOKED_AGENT_ID: ensure_ids(); *out = mrl::make_desc(agent_id, MRL_INT32, device, {P, N}); return true;
        case MRL_OVERCOOKED_LOCATION_WORLD_ID:
            ensure_ids();
            *out = mrl::make_desc(loc_world_id, MRL_INT32, device, {P * C, N});
            return true;
        case MRL_OVERCOOKED_LOCATION_ID: ensure_ids(); *out = mrl::make_desc(loc_id, MRL_INT32, device, {P * C, N}); return true;
        case MRL_OVERCOOKED_OBS_WORLD_MAJOR:
            *out = mrl::make_desc(own_obs, MRL_INT8, device, {N, P, (int64_t)H, W, F});
            return true;
        case MRL_OVERCOOKED_STATE_PLAYERS: *out = mrl::make_desc(params.players, MRL_UINT8, device, {N, P, 8}); return true;
        case MRL_OVERCOOKED_STATE_OBJECTS: *out = mrl::make_desc(params.cell_obj, MRL_UINT8, device, {N, C, 4}); return true;
        default: return false;
        }
    }

    size_t action_elems() const override { return (size_t)params.P * num_worlds; }
    void phase2(const uint32_t *, hipStream_t) override {}
};

}  // namespace mrl_kitchen
